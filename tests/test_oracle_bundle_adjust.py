"""CPU only: pins tests/ba_oracle.py, the float64 restatement of poselib::refineStereoBA that the device is held to.  No build of the
reference's SBA stands behind it, so it is held to what can be checked without one: its Jacobian against finite differences of its own
projection, convergence on exact data, the wrapper's rules, the permutation study that the device tolerances come from, and -- scene by
scene -- that it takes the exit or branch each scene of ba_scenes.BRANCH_SCENES is named for."""
import numpy as np
import pytest

import ba_oracle as BAO
import ba_scenes as S


def test_jacobian_equals_central_differences():
    """The analytic Jacobian against a central difference of the UN-weighted projection.  Step h = 1e-6: the truncation term is h^2 / 6 times
    a third derivative (below 100 for image coordinates below 1 and depths of 4 and more: 2e-11), the rounding term eps |f| / h with
    |f| <= 1 and a few operations behind it (about 2e-10 each side); ten times their sum is the bound."""
    s = S.scene("n64")
    r0 = BAO.mat_to_quat(s["R"])
    v, t, M = np.array([0.01, -0.02, 0.015]), s["t"], s["Q"]
    h = 1e-6
    tol = 10 * (h * h / 6 * 100 + 2 * np.finfo(float).eps * 1.0 / h)
    A, B = BAO.jacobian(r0, v, t, M)

    def f(v, t, M):
        return BAO.project(BAO.quat_mult_fast(BAO.local_quat(v), r0), t, M)

    assert np.abs(f(v, t, M)).max() < 1.0
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        assert np.abs((f(v + d, t, M) - f(v - d, t, M)) / (2 * h) - A[:, :, k]).max() < tol
        assert np.abs((f(v, t + d, M) - f(v, t - d, M)) / (2 * h) - A[:, :, 3 + k]).max() < tol
        assert np.abs((f(v, t, M + d) - f(v, t, M - d)) / (2 * h) - B[:, :, k]).max() < tol
    assert tol < 1e-8 and np.abs(A).max() > 1.0       # the bound means something


@pytest.mark.parametrize("rot_err_deg", (0.3, 3.0))
def test_exact_data_converges_to_the_truth(rot_err_deg):
    """Noise-free measurements, the start a perturbed pose and perturbed points, the Huber threshold far above every residual (th = 1 in
    camera units, the quadratic end of the cost; with the facade's default, 1e-5, the cost is linear in the residual while the Jacobian stays
    the plain one, and the optimiser stops on its relative-reduction test long before).  A residual below about 1e-8 th is flushed to
    exactly zero by sqrt(1 + r^2) - 1, and the optimiser stops at a relative step of 1e-12, so the final ||e||^2 is bounded by 480 residuals
    of 1e-9: 1e-15.  The pose comes back up to the gauge (the scale of t): a residual of 1e-8 at depths up to 20 over a baseline of 1 moves
    the pose by at most 1e-8 * 20^2 = 4e-6; 1e-5 is asserted."""
    s = S.make_scene(120, seed=5, rot_err_deg=rot_err_deg, noise_px=0.0, outlier_frac=0.0)
    o = BAO.ba_oracle(s["p1"], s["p2"], s["R"], s["t"], s["Q"], 1.0, None, 1e9, 1e9)
    assert o["accepted"] and o["info"][6] in (2, 5) and o["info"][0] > 1e-3
    assert o["info"][1] <= 1e-15
    assert np.abs(s["R"] - s["R_true"]).max() > 1e-3
    assert np.abs(o["R"] - s["R_true"]).max() < 1e-5
    assert np.abs(o["t"] / np.linalg.norm(o["t"]) - s["t_true"]).max() < 1e-5
    scale = np.sum(o["Q"] * s["X"]) / np.sum(s["X"] * s["X"])     # the gauge: the points carry the scale the start gave them
    assert abs(scale - 1) < 0.1 and np.abs(o["Q"] / scale - s["X"]).max() < 1e-5 * 20 * 20


def test_rejection_rule_leaves_everything_untouched():
    s, o = S.scene("rejected"), S.oracle_result("rejected")
    assert not o["accepted"] and o["info"][6] <= 5 and o["info"][5] > 0          # the optimiser ran and ended normally: the difference rule refused
    assert o["R"].tobytes() == s["R"].tobytes() and o["t"].tobytes() == s["t"].tobytes() and o["Q"].tobytes() == s["Q"].tobytes()
    wide = BAO.ba_oracle(s["p1"], s["p2"], s["R"], s["t"], s["Q"], s["th"], s["mask"], 10.0, 1.0)
    assert wide["accepted"] and wide["info"].tobytes() == o["info"].tobytes() and not np.array_equal(wide["R"], s["R"])
    cosang = (np.trace(wide["R"] @ s["R"].T) - 1) / 2
    assert np.degrees(np.arccos(cosang)) > 1.1 * S.ANGLE_THRESH                   # well beyond the threshold, not at it


def test_threshold_reads_fy_and_the_one():
    """(1,1) + (2,2) of both camera matrices: fy and the 1.0, not fx and fy."""
    K1 = np.array([[650.0, 0, 320], [0, 700.0, 240], [0, 0, 1]])
    K2 = np.array([[640.0, 0, 320], [0, 720.0, 240], [0, 0, 1]])
    th = BAO.convert_threshold(K1, K2, 0.8)
    assert th == 4.0 * 0.8 / (np.sqrt(2.0) * (700.0 + 1.0 + 720.0 + 1.0))
    assert abs(th - 4.0 * 0.8 / (np.sqrt(2.0) * (650.0 + 700.0 + 640.0 + 720.0))) > 0.4 * th
    s = S.scene("n65")
    a = BAO.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], K1, K2, huber_thresh=0.8)
    b = BAO.ba_oracle(s["p1"], s["p2"], s["R"], s["t"], s["Q"], th)
    assert a["info"].tobytes() == b["info"].tobytes() and a["R"].tobytes() == b["R"].tobytes()


def test_negative_threshold_selects_the_default():
    s = S.scene("n65")
    assert S.TH == BAO.convert_threshold(S.K, S.K, -1.0) == BAO.convert_threshold(S.K, S.K, 0.005) == 4.0 * 0.005 / (np.sqrt(2.0) * 1402.0)
    a = BAO.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], S.K, S.K)
    b = BAO.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], S.K, S.K, huber_thresh=0.005)
    c = BAO.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], S.K, S.K, huber_thresh=0.01)
    assert a["info"].tobytes() == b["info"].tobytes() == S.oracle_result("n65")["info"].tobytes()
    assert c["info"][1] != a["info"][1]


def test_mask_compacts_and_scatters():
    s, o = S.scene("n1000_masked"), S.oracle_result("n1000_masked")
    keep = s["mask"] != 0
    assert keep.sum() == 1000 and 0.55 < keep.mean() < 0.65 and set(np.unique(s["mask"])) == {0, 1, 255}
    c = BAO.ba_oracle(s["p1"][keep], s["p2"][keep], s["R"], s["t"], s["Q"][keep], s["th"])
    assert o["accepted"] and c["info"].tobytes() == o["info"].tobytes() and c["R"].tobytes() == o["R"].tobytes()
    assert o["Q"][keep].tobytes() == c["Q"].tobytes() and o["Q"][~keep].tobytes() == s["Q"][~keep].tobytes()
    assert not np.array_equal(o["Q"][keep], s["Q"][keep])


def test_too_few_points_and_empty_inputs_fail():
    s, o = S.scene("n7"), S.oracle_result("n7")          # 28 measurements, 33 unknowns: the optimiser refuses
    assert not o["accepted"] and not o["info"].any() and o["R"].tobytes() == s["R"].tobytes() and o["Q"].tobytes() == s["Q"].tobytes()
    big = S.scene("n64")
    z = BAO.ba_oracle(big["p1"], big["p2"], big["R"], big["t"], big["Q"], big["th"], np.zeros(64, np.uint8))
    assert not z["accepted"] and not z["info"].any() and z["Q"].tobytes() == big["Q"].tobytes()
    e = BAO.ba_oracle(np.zeros((0, 2)), np.zeros((0, 2)), big["R"], big["t"], np.zeros((0, 3)), big["th"])
    assert not e["accepted"]


def test_scenes_are_what_the_device_test_needs():
    for name, (n_valid, rows, _, _) in S.SCENES.items():
        s, o = S.scene(name), S.oracle_result(name)
        assert s["p1"].shape == (rows, 2) and (s["mask"] is None) == (rows == n_valid)
        assert (np.count_nonzero(s["mask"]) if s["mask"] is not None else rows) == n_valid
        if n_valid >= 12:
            assert 3 <= o["info"][5] < BAO.MAXITER and o["info"][6] in (2, 4) and o["info"][1] < o["info"][0], name
    assert [S.oracle_result(k)["accepted"] for k in S.SCENES] == [False, True, True, True, True, False]
    assert any(not step[2] for step in S.oracle_result("n257")["trace"])       # one scene walks the damping loop's rejected attempts


def test_tolerances_come_from_the_permutation_study():
    """The device differs from the oracle only in the association of its sums; permuting the points changes the order of every sum in the
    oracle and nothing else.  Every scene must keep its verdict, iteration count, stop reason and counts under all 20 permutations, and the
    committed tolerances are 10 x the largest spread (at most 100 x)."""
    sp = S.permutation_spread()
    assert sp["stable"], "a scene changes its integers under a permutation: choose another seed"
    for const, key in ((S.TOL_POSE, "pose"), (S.TOL_Q, "q"), (S.TOL_INFO, "info"), (S.TOL_MU, "mu")):
        assert sp[key] > 0 and 10 * sp[key] <= const <= 100 * sp[key], (key, sp[key], const)
    # the scenes of BRANCH_SCENES: the same rule, each scene on its own study; a spread of exactly 0 asks for a constant of exactly 0
    for name, row in S.BRANCH_SCENES.items():
        sp = S.branch_spread(name)
        assert sp["stable"], (name, "changes its integers under a permutation: choose another seed")
        for key, const in row["tol"].items():
            assert np.isfinite(sp[key]) and 10 * sp[key] <= const <= 100 * sp[key], (name, key, sp[key], const)
        if row["kind"] == "refused":
            assert row["tol"]["pose"] == 0 and row["tol"]["q"] == 0, name       # the inputs come back byte for byte


# sha256 over info, R, t, Q of ba_oracle on SCENES as they were BEFORE the oracle learnt to report its branches (attempts, branch) and to pass
# over a NaN in ||J^T e||_inf: neither may move a bit of the existing results
PINNED = {
    "n7": "7639f689f0a90176aba7cf9376ceef75520a1b70bd2d225886969423969c2182",
    "n64": "9cabadd646d72111c06c5db5cf38491090d365f7cc43703fc693e868fa3f1020",
    "n65": "50a4e49d1d26bcfb49f2b7b0df929e7c34d1d7ac035c73fa4216c315b8fd43c6",
    "n257": "bd2c0b5da89bf4de8eeb0dade50211155d92a7e66788375d51d8931e9f3477fd",
    "n1000_masked": "d9a3ccb4d5155fc2b3149d9122d32965def56bd4ec2557eaef65df42f97bae0f",
    "rejected": "a8546d1c1fc94abae7afefbb56b46315c7de3dde5d095179043bd5977af4f869",
}


def test_existing_results_are_pinned_bit_for_bit():
    import hashlib

    assert set(PINNED) == set(S.SCENES)
    for name, want in PINNED.items():
        o = S.oracle_result(name)
        assert hashlib.sha256(o["info"].tobytes() + o["R"].tobytes() + o["t"].tobytes() + o["Q"].tobytes()).hexdigest() == want, name


def test_make_scene_defaults_are_the_old_scenes():
    """The parameters added to make_scene do nothing at their defaults, spelled out or not."""
    a = S.make_scene(65, 65, 13, 0.3)
    b = S.make_scene(65, 65, 13, 0.3, rot_axis=(0.2, 0.9, 0.1), rot_deg=5.0, t_true=None, t_err=0.01, start_rot_deg=None, t_scale=None,
                     q_rows=None, th=S.TH)
    for k in ("p1", "p2", "R", "t", "Q"):
        assert a[k].tobytes() == b[k].tobytes() == S.scene("n65")[k].tobytes(), k
    o = BAO.ba_oracle(a["p1"], a["p2"], a["R"], a["t"], a["Q"], a["th"])
    assert o["info"].tobytes() == S.oracle_result("n65")["info"].tobytes()


PLANTED = S.PLANTED_ROW


def _longest_rejected_run(attempts):
    """The most consecutive attempts of one outer iteration that did not end accepted."""
    best = run = 0
    last = None
    for itno, _, _, accepted in attempts:
        if itno != last:
            run = 0
        run = 0 if accepted else run + 1
        last = itno
        best = max(best, run)
    return best


def test_longest_rejected_run_counts_within_one_iteration():
    A = [(0, -1, False, False), (0, -1, True, False), (0, -1, False, True), (1, -1, False, False), (2, 3, False, False), (2, -1, False, False),
         (2, -1, False, False), (2, -1, False, True)]
    assert _longest_rejected_run(A) == 3 and _longest_rejected_run(A[:4]) == 2 and _longest_rejected_run([]) == 0


@pytest.mark.parametrize("name", list(S.BRANCH_SCENES))
def test_branch_scene_takes_its_branch(name):
    """Every scene of BRANCH_SCENES runs, in the oracle, through the exit or branch it is named for.  A scene that drifts off fails here, on
    the CPU, and not silently on the device."""
    row, s, o = S.BRANCH_SCENES[name], S.scene(name), S.oracle_result(name)
    ex, br, att = row["expect"], o["branch"], o["attempts"]
    n_valid = s["p1"].shape[0] if s["mask"] is None else np.count_nonzero(s["mask"])
    assert (s["mask"] is None) == (not name.endswith("_of_40")) and o["accepted"] == ex["accepted"] == (row["kind"] == "accepted"), name
    assert not br.get("almost_singular", False)
    for key, at in (("itno", 5), ("stop", 6)):
        if key in ex:
            assert int(o["info"][at]) == ex[key], (name, key, o["info"])
    if "min_rejected" in ex:
        assert _longest_rejected_run(att) >= ex["min_rejected"] >= 2, (name, _longest_rejected_run(att))
    if "min_refused_solves" in ex:
        assert sum(1 for a in att if a[2]) >= ex["min_refused_solves"] >= 1, name
    if "first_bad" in ex:
        bad = [a[1] for a in att]
        assert len(bad) == 30 and bad[0] == ex["first_bad"] and min(bad) >= 0 and int(o["info"][9]) == 0, (name, bad)   # no attempt got to a solve
        assert 0 < PLANTED < n_valid - 1
        if ex["first_bad"] == PLANTED:       # valid points before (they take their new inverse's diagonal) and after (untouched)
            assert bad.count(PLANTED) >= 2 and set(bad) <= {0, PLANTED}, (name, bad)
    for key in ("pivot", "r0_flipped", "qn_flipped", "t_case", "refused_by"):
        if key in ex:
            assert br[key] == ex[key], (name, key, br)
    if o["accepted"]:
        assert br["refused_by"] == () and int(o["info"][6]) in (1, 2, 3, 4, 5)
        if ex.get("itno") != 0:
            assert not np.array_equal(o["Q"], s["Q"]), name
        t_len = np.sqrt(o["t"] @ o["t"])
        if br["t_case"] == "kept_tiny":
            assert t_len < 1e-3
        elif ex.get("t_out_is_unit") is False:
            assert 1e-9 < abs(t_len - 1) <= 1e-4                      # kept although it is measurably not 1
        else:
            assert abs(t_len - 1) < 1e-15
        assert np.abs(o["R"] @ o["R"].T - np.eye(3)).max() < 1e-14
    else:
        assert o["R"].tobytes() == s["R"].tobytes() and o["t"].tobytes() == s["t"].tobytes() and o["Q"].tobytes() == s["Q"].tobytes(), name
        if int(o["info"][6]) == 7 or n_valid < 12:
            assert "refused_by" not in br                               # the wrapper never got to its rules
    if name == "qn_flip_across_180":          # the refined rotation is on the other side of 180 degrees
        assert (s["R"][1, 0] - s["R"][0, 1]) * (o["R"][1, 0] - o["R"][0, 1]) < 0
    if name.startswith("stop7_start"):
        assert not np.isfinite(o["info"][0]) and not np.isfinite(o["info"][1]) and (s["Q"][PLANTED, 2] == 0 or np.isnan(s["Q"][PLANTED]).any())
    if name.startswith("stop7_midrun"):
        assert np.isfinite(o["info"][:5]).all() and np.isfinite(s["Q"]).all()
    if name in ("n11", "n11_of_40"):
        assert n_valid == 11 and not o["info"].any() and o["mu"] == 0.0
    if name in ("n12", "n12_of_40"):
        assert n_valid == 12 and o["info"][5] > 0


def test_branch_scenes_cover_every_exit_and_branch():
    R = {name: S.oracle_result(name) for name in S.BRANCH_SCENES}
    assert {int(o["info"][6]) for o in R.values()} == {0, 1, 2, 3, 4, 5, 6, 7}                       # 0: the optimiser refused to start
    ran = [o["branch"] for o in R.values() if "refused_by" in o["branch"]]
    assert {o["branch"]["pivot"] for o in R.values()} == {-1, 0, 1, 2} and {b["t_case"] for b in ran} == {"kept_unit", "kept_tiny", "normalised"}
    assert {b["qn_flipped"] for b in ran} == {False, True}
    assert {(o["branch"]["pivot"] >= 0, o["branch"]["r0_flipped"]) for o in R.values()} >= {(True, True), (True, False), (False, False)}
    alone = {b["refused_by"] for b in ran} | {S.oracle_result("rejected")["branch"]["refused_by"]}
    assert alone >= {("angle",), ("t_norm",), ("stop",), ()}                                          # each rule refuses on its own somewhere
    sizes = {(s["p1"].shape[0] if s["mask"] is None else int(np.count_nonzero(s["mask"]))) for s in map(S.scene, S.BRANCH_SCENES)}
    assert sizes >= {11, 12, 13, 255, 256, 512, 513} and max(sizes) == 513
    mid = sorted(int(R[k]["info"][5]) for k in R if k.startswith("stop7_midrun"))
    assert mid[0] > 0 and len(set(mid)) == 2


def test_nan_in_jte_is_passed_over_as_the_reference_does():
    """sba_levmar.c:943-944: `if(eab_inf < tmp) eab_inf = tmp`, from 0, never takes a NaN.  No scene reaches this with a finite ||e||^2 (a
    Jacobian entry that is not finite makes the residual of the same point not finite first), so the reduction is pinned on its own."""
    ea, eb = np.array([1.0, -3.0, 2.0, 0.5, 0.0, 1.0]), np.array([[np.nan, 7.0, -2.0], [1.0, np.nan, -9.0]])
    assert BAO.jte_inf_norm(ea, eb) == 9.0 and BAO.jte_inf_norm(np.array([np.nan] * 6), eb[:, :1]) == 1.0
    assert BAO.jte_inf_norm(np.full(6, np.nan), np.full((2, 3), np.nan)) == 0.0 and BAO.jte_inf_norm(ea, np.zeros((2, 3))) == 3.0
