"""CPU only: pins tests/ba_oracle.py, the float64 restatement of poselib::refineStereoBA that the device is held to.  No build of the
reference's SBA stands behind it, so it is held to what can be checked without one: its Jacobian against finite differences of its own
projection, convergence on exact data, the wrapper's rules, and the permutation study that the device tolerances come from."""
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
