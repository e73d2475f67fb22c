"""CPU: the restatement tests/subpix_separate_oracle.py of matchinglib::getSubPixMatches_seperate_Imgs (cv::cornerSubPix on each image) checked
against what it must find -- the known corners of an anti-aliased checkerboard -- and against the rules of the contract in include/mlpl_c.h."""
import numpy as np
import pytest

import subpix_separate_oracle as O
import subpix_separate_scenes as S

EDGE_POINTS = [(0, 0), (319, 0), (0, 239), (319, 239), (0.4, 100.3), (1, 100), (318.6, 50.2), (160.5, 0), (160.2, 239), (160, 238.7), (-0.5, 20),
               (319.9, 30), (5, 5), (-3, -3), (325, 245), (-1e6, 50), (50, 1e7)]


def edge_scene(size):
    b1, b2 = S.boards()
    n = len(EDGE_POINTS)
    return S.with_points(dict(img1=b1["img"], img2=b2["img"]), EDGE_POINTS, EDGE_POINTS, None if size is None else np.full(n, size),
                         None if size is None else np.full(n, size))


def test_corner_scene_is_the_prototype():
    b1, b2 = S.boards()
    assert b1["img"].shape == (240, 320) and b1["img"].dtype == np.uint8 and len(b1["corners"]) == 106
    assert b1["img"].min() == 40 and b1["img"].max() == 210 and len(b2["corners"]) > 60
    c = b1["corners"]
    assert c.min() >= 14 and (c[:, 0] <= 319 - 14).all() and (c[:, 1] <= 239 - 14).all()


@pytest.mark.parametrize("w,size", [(3, 6.0), (5, 9.5), (10, 0.0)])
def test_jittered_corners_are_found(w, size):
    """keypoints up to 2 px from the corner: every refined point within 0.25 px of it.  A wrong sign, mask or window offset leaves errors
    of whole pixels; this restatement measures 0.120 / 0.081 / 0.064 px at w = 3 / 5 / 10."""
    s, exp = S.corners(106, 1, 2.0, 0.0, size, size)
    assert exp["info"] == [w, w, 0, 0] and exp["status"] == 0 and exp["inlier"].all()
    e1 = np.sqrt(((exp["kp1"] - s["truth1"]) ** 2).sum(axis=1))
    e2 = np.sqrt(((exp["kp2"] - s["truth2"]) ** 2).sum(axis=1))
    print(f"w {w}: max error {e1.max():.3f} / {e2.max():.3f} px, passes {exp['iters'].min()} .. {exp['iters'].max()}")
    assert e1.max() < 0.25 and e2.max() < 0.25
    assert 2 <= exp["iters"].min() and exp["iters"].max() <= 12


def test_three_pixels_of_jitter_make_outliers():
    """a point that moves by more than sqrt(12) is an outlier: neither keypoint of its match changes"""
    s, exp = S.corners(106, 2, 2.0, 0.7)
    out = exp["inlier"] == 0
    assert out.sum() > 60 and exp["status"] == -1 and exp["n_refined"] == int(exp["inlier"].sum()) < 106 // 3
    assert (out == s["scrambled"]).all()
    assert exp["kp1"][out].tobytes() == s["kp1"][out].tobytes() and exp["kp2"][out].tobytes() == s["kp2"][out].tobytes()
    moved = ((exp["raw2"] - s["kp2"]) ** 2).sum(axis=1)
    assert (moved[out] > 12).all() and (np.sqrt(((exp["raw2"] - s["truth2"]) ** 2).sum(axis=1)) < 0.25).all()
    assert (exp["kp2"][~out] != s["kp2"][~out]).any(axis=1).all()


def test_list_lengths_reach_both_sides_of_the_status_rule():
    seen = set()
    for n, sc in S.count_cases():
        _, exp = S.corners(n, 0, 2.0, sc)
        r = exp["n_refined"]
        assert exp["status"] == (-1 if (r < n // 3 or r < 2) else 0)
        seen.add((r < n // 3, r < 2))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_too_far_rule_singular_pass_and_edges():
    _, tex = S.texture()
    print(f"texture at w = 3: {tex['info'][3]} of 400 points reset")
    assert tex["info"][:2] == [3, 3] and tex["info"][3] > 200                  # a smooth texture has no corner to hold the iteration
    assert tex["far"].any() and (~tex["far"] & (tex["iters"] > 0)).any()       # both results of the rule
    s, exp = S.constant()
    assert exp["singular"].all() and (exp["iters"] == 0).all() and exp["inlier"].all() and exp["status"] == 0 and exp["n_refined"] == 6
    assert exp["kp1"].tobytes() == s["kp1"].tobytes() and exp["info"] == [10, 3, 0, 0]
    for size, w in ((6.0, 3), (None, 10)):
        e = S.oracle(edge_scene(size))
        assert e["info"][:3] == [w, w, 0]
        assert e["left"].any() and e["far"].any() and (e["iters"] == 40).any() == (w == 3)
    # the replicated edge: a board continued beyond the image by its edge pixels gives the same result
    s, exp = S.corners(65, 3)
    pad = 16
    big = dict(s, img1=np.pad(s["img1"], pad, mode="edge"), img2=np.pad(s["img2"], pad, mode="edge"))
    pts = np.array([[2.2, 30.1], [317.5, 100.0], [100.3, 1.0], [200.0, 238.2], [0.0, 0.0]], np.float32)
    a = O.subpix(s["img1"], s["img2"], pts, pts, None, None)
    b = O.subpix(big["img1"], big["img2"], pts + np.float32(pad), pts + np.float32(pad), None, None)
    assert a["iters"].tolist() == b["iters"].tolist() and np.abs((b["raw1"] - np.float32(pad)) - a["raw1"]).max() < 1e-3


def test_dropped_and_non_finite_points():
    b1, b2 = S.boards()
    nan, inf = float("nan"), float("inf")
    c = b1["corners"][:6] + np.float32(0.4)
    kp1 = c.copy()
    kp2 = b2["corners"][:6] + np.float32(0.4)
    kp1[1, 0], kp1[3, 1] = nan, 3e9
    kp2[3, 0], kp2[4, 1], kp2[5, 0] = -inf, 2147483648.0, -2147483648.0
    s = S.with_points(dict(img1=b1["img"], img2=b2["img"]), kp1, kp2)
    e = S.oracle(s)
    assert e["inlier"].tolist() == [1, 0, 1, 0, 0, 1] and e["info"][2] == 4      # match 3 loses both points; -2^31 fits an int
    assert e["kp1"].tobytes() == np.where(e["inlier"][:, None] == 1, e["raw1"], s["kp1"]).tobytes()
    assert e["iters"][1].tolist()[0] == 0 and e["iters"][1].tolist()[1] > 0      # the partner of a dropped point is still iterated


def test_window_helper_and_mask_profiles():
    nan = float("nan")
    sizes = [(0.0, 3), (1e-3, 3), (5.9, 3), (6.0, 3), (6.1, 4), (8.0, 4), (9.5, 5), (10.0, 5), (10.5, 6), (13.0, 7), (14.1, 8), (16.1, 9), (18.0, 9),
             (18.1, 10), (20.0, 10), (31.0, 10), (3.4e38, 10), (-5.0, 3), (nan, 10)]
    assert [O.window(a) for a, _ in sizes] == [w for _, w in sizes]
    assert O.list_window(None) == 10 and O.list_window([]) == 10 and O.list_window([0.0, nan, -3.0]) == 10
    assert O.list_window([31.0, nan, 13.0, -1.0, 0.0]) == 7 and O.list_window([9.5, 6.0]) == 3
    for w in range(3, 11):
        g = O.profile(w)
        y = (np.arange(2 * w + 1, dtype=np.float64) - w).astype(np.float32) / np.float32(w)
        want = np.exp(-(y.astype(np.float64) ** 2)).astype(np.float32)       # float32 y, its square as a float32, exp in float64
        sq = (y * y).astype(np.float64)
        assert g.dtype == np.float32 and len(g) == 2 * w + 1 and g[w] == 1.0 and g.tobytes() == np.exp(-sq).astype(np.float32).tobytes()
        assert np.abs(g - want).max() <= 6e-8 and g.tobytes() == g[::-1].tobytes()


def test_summation_order():
    """step 3c written lane by lane in plain Python floats"""
    rng = np.random.default_rng(0)
    for K in (49, 64, 121, 441):
        t = rng.normal(size=K) * 10.0 ** rng.integers(-6, 6, K)
        v = [0.0] * 64
        seen = [False] * 64
        for k in range(K):
            v[k % 64] = float(t[k]) if not seen[k % 64] else v[k % 64] + float(t[k])
            seen[k % 64] = True
        for s in (32, 16, 8, 4, 2, 1):
            for l in range(s):
                v[l] = v[l] + v[l + s]
        assert O.wave_sum(t[None, :])[0] == v[0]
    z = O.wave_sum(np.full((1, 49), -0.0))
    assert z[0] == 0.0 and not np.signbit(z[0])          # the idle lanes hold +0.0
