"""CPU: the restatement tests/subpix_oracle.py of matchinglib::getSubPixMatches -- its side arithmetic against the reference's literal form,
cvRound, the argument that the fit's zero-denominator branch is unreachable, what the refinement recovers on a shifted texture, and a
scene set where the float32 rounding of the sums decides the minimum."""
import numpy as np

import subpix_oracle as O
import subpix_scenes as S


def test_side_reduction_equals_the_literal_form():
    """matchers.cpp:1156-1165 uses cvRound(fs / 2.0f) only to tell even from odd: for every fs in 18..300 the literal form gives the side
    and the half side of the reduced form (even -> fs - 1; d1 = (side - 1) / 2)"""
    for fs in range(18, 301):
        assert O.side_literal(fs) == O.side_reduced(fs), fs
        side, d1 = O.side_reduced(fs)
        assert side % 2 == 1 and side in (fs, fs - 1) and 2 * d1 + 1 == side


def test_template_sides():
    nan = float("nan")
    s1 = [0, 11.9, 12, 13, 14, 31, 111.1, 249, 250, 250.9, 251, nan, -5, 40, 3, nan, 20, 1e30, float("inf")]
    s2 = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 40, 20, nan, 0, 0]
    exp = [17, 17, 17, 19, 19, 37, 117, 255, 255, 255, 0, 17, 17, 45, 45, 25, 17, 0, 0]
    # (NaN, 20): NaN > 20 is false -> 20; (20, NaN): 20 > NaN is false -> NaN -> the clamp
    assert O.template_sides(s1, s2).tolist() == exp


def test_cv_round_is_half_to_even():
    assert O.cv_round([10.5, 11.5, -0.5, -1.5, 2.5, 3.49999, 1e6 + 0.5]).tolist() == [10, 12, 0, -2, 2, 3, 1000000]


def _all_results():
    out = [S.texture(n, n % 5, sc)[1] for n, sc in S.count_cases()]
    out += [S.texture(400, 0)[1], S.texture(400, 0, noise=4.0)[1], S.constant()[1]]
    out += [S.rounding(seed)[1] for seed in S.ROUNDING_SEEDS]
    return out


def test_zero_denominator_is_unreachable():
    """with a FIRST-minimum argmin the left and the upper neighbour are strictly larger than the minimum, the right and the lower one not
    smaller: 2 c - xn - xp < 0 in float as well (2 c - xn is below zero by at least an ulp of the table and xp >= c >= 0 keeps it there).  No
    inlier of any scene has a zero denominator, so refined == inliers everywhere."""
    inliers = 0
    for r in _all_results():
        k = r["inlier"].astype(bool)
        inliers += int(k.sum())
        assert not (r["nx"][k] == 0).any() and not (r["ny"][k] == 0).any()
        assert (r["nx"][k] < 0).all() and (r["ny"][k] < 0).all()
        assert r["refined"].tobytes() == k.tobytes() and r["n_refined"] == int(k.sum())
    assert inliers > 1000


def test_both_sides_of_the_status_rule_are_hit():
    seen = set()
    for n, sc in S.count_cases():
        r = S.texture(n, n % 5, sc)[1]
        seen.add((r["n_refined"] < n // 3, r["n_refined"] < 2))
        assert r["status"] == (-1 if (r["n_refined"] < n // 3 or r["n_refined"] < 2) else 0)
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_shifted_texture_is_recovered():
    """synth.subpix_scene("texture", 400, seed 0): image 2 is the texture moved by (3.3, -2.6) px.  Measured with the oracle over the
    keypoints more than 20 px from the edge (282 without noise, 292 with sigma = 4 grey levels), all of them inliers: median error per
    coordinate 0.075 px / 0.084 px, maximum 0.525 px / 0.436 px.  The bounds are twice the measured maxima."""
    for noise, bound in ((0.0, 2 * 0.525), (4.0, 2 * 0.436)):
        s, r = S.texture(400, 0, noise=noise)
        k = s["kp1"]
        far = (k[:, 0] > 20) & (k[:, 0] < S.W - 20) & (k[:, 1] > 20) & (k[:, 1] < S.H - 20)
        assert far.sum() > 250 and r["inlier"][far].all() and r["status"] == 0
        err = np.abs(r["kp2"] - s["truth"])[far]
        print(f"noise {noise}: {int(far.sum())} keypoints, median error {np.median(err):.3f} px, maximum {err.max():.3f} px (bound {bound:.3f})")
        assert err.max() < bound and np.median(err) < 0.2
        assert (s["kp1"].tobytes() == S.texture(400, 0, noise=noise)[0]["kp1"].tobytes())


def test_float_rounding_decides_the_minimum():
    """sums above 2^29 (float32 steps by 64 there): in every scene of the set some inlier's first float32 minimum is not where the exact
    integers have theirs, and different integers share a float value"""
    for seed in S.ROUNDING_SEEDS:
        s, r = S.rounding(seed)
        t = r["table"].reshape(len(s["kp1"]), 121)
        assert r["info"] == [0, 0, 0, 117] and t.min() > 2 ** 29
        exact, as_float = t.argmin(axis=1), t.astype(np.float32).argmin(axis=1)
        differ = (exact != as_float) & r["inlier"].astype(bool)
        print(f"seed {seed}: inliers {int(r['inlier'].sum())} of {len(t)}, float minimum elsewhere for {int(differ.sum())}")
        assert differ.any()
        i = int(np.nonzero(differ)[0][0])
        assert np.float32(t[i, exact[i]]) == np.float32(t[i, as_float[i]]) and t[i, exact[i]] != t[i, as_float[i]] and as_float[i] < exact[i]


def test_constant_images_tie_everywhere():
    s, r = S.constant()
    assert (r["table"] == 0).all() and not r["inlier"].any() and r["status"] == -1 and r["kp2"].tobytes() == s["kp2"].tobytes()


def test_compose_last_writer_and_reverse_order():
    s, _ = S.texture(64, 4)
    m = np.zeros(6, O.DMATCH)
    m["queryIdx"] = [0, 1, 2, 3, 4, 5]
    m["trainIdx"] = [0, 1, 0, 3, 1, 70]          # train 0 and 1 named twice, 70 clamps to 63
    kp2 = s["kp2"].copy()
    kp2[0], kp2[1], kp2[63] = s["kp2"][2], s["kp2"][4], s["kp2"][5]   # so that the LATER match of each pair is the good one
    r = O.compose(s["img1"], s["img2"], m, s["kp1"], kp2)
    assert r["inlier"].tolist() == [0, 0, 1, 1, 1, 1] or r["inlier"][2:].all()
    single = O.subpix(s["img1"], s["img2"], s["kp1"][[0, 1, 2, 3, 4, 5]], kp2[[0, 1, 0, 3, 1, 63]])
    assert r["kp2_out"][0].tobytes() == single["kp2"][2].tobytes() and r["kp2_out"][1].tobytes() == single["kp2"][4].tobytes()
    assert r["kp2_out"][63].tobytes() == single["kp2"][5].tobytes() and r["kp2_out"][2].tobytes() == kp2[2].tobytes()
    on = O.compose(s["img1"], s["img2"], m, s["kp1"], kp2, rule=True)
    assert on["status"] == 0 and on["matches"].tobytes() == r["matches"][::-1].tobytes()
    # status -1 under the rule: list and keypoints pass through
    bad = kp2 + np.float32(7.0)
    off = O.compose(s["img1"], s["img2"], m, s["kp1"], bad, rule=True)
    assert off["status"] == -1 and off["matches"].tobytes() == m.tobytes() and off["kp2_out"].tobytes() == bad.tobytes()
