"""CPU-only: tests/ba_multicam_oracle.py, the float64 restatement of poselib::refineMultCamBA (pointsInImgCoords == false) that the device is
held to -- its Jacobian against central differences, a noise-free four-camera scene with partial visibility, its two-camera reduction to
ba_oracle.py bit for bit, its refusals, and the permutation study that sets the tolerances of ba_multicam_scenes.py."""
import numpy as np
import pytest

import ba_multicam_oracle as BMO
import ba_multicam_scenes as S
import ba_oracle as BAO
import ba_scenes as BAS


def test_jacobian_against_central_differences():
    """A_ij, B_ij of a camera at a general pose and a non-zero local rotation, as the optimiser uses them for every camera."""
    rng = np.random.default_rng(5)
    s = S.scene("cam0_not_identity")
    M = s["X"][:12]
    for j in range(s["m"]):
        q = BAO.mat_to_quat(s["R"][j])
        r0 = q * ((1.0 if q[0] >= 0 else -1.0) / np.sqrt(q @ q))
        v, t = rng.normal(0, 0.01, 3), s["t"][j]
        A, B = BAO.jacobian(r0, v, t, M)
        f = lambda vv, tt, MM: BAO.project(BAO.quat_mult_fast(BAO.local_quat(vv), r0), tt, MM)
        h = 1e-6
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            np.testing.assert_allclose(A[:, :, k], (f(v + d, t, M) - f(v - d, t, M)) / (2 * h), rtol=0, atol=2e-8)
            np.testing.assert_allclose(A[:, :, 3 + k], (f(v, t + d, M) - f(v, t - d, M)) / (2 * h), rtol=0, atol=2e-8)
            np.testing.assert_allclose(B[:, :, k], (f(v, t, M + d) - f(v, t, M - d)) / (2 * h), rtol=0, atol=2e-8)


def test_noise_free_scene_converges_to_the_truth():
    """m = 4, partial visibility, a perturbed start, the Huber threshold far above every residual: the cost is the plain squared error and
    its minimum is the truth, up to the gauge that camera 0 fixes (its pose; the scale stays where the other cameras' start leaves it, so
    the comparison is made after a scaling about camera 0's centre, the origin).  The bounds are those of test_oracle_bundle_adjust.py's
    twin: sqrt(1 + r^2) - 1 flushes a residual below about 1e-8 th to exactly zero, so the final ||e||^2 is at most 1e-15, and a residual of
    1e-8 at depths up to 20 over a baseline of 1 moves a pose by at most 1e-8 * 20^2 = 4e-6; 1e-5 is asserted, and 1e-5 * 20^2 for a point."""
    s = S.make_scene(4, 60, seed=31, vis=S.vis_frac(0.7), noise_px=0.0, outlier_frac=0.0, th=1.0)
    o = BMO.ba_multicam_oracle(s["p"], s["vis"], s["R"], s["t"], s["Q"], s["th"], 180.0, 10.0)
    assert o["accepted"] and o["info"][6] in (2, 5) and o["info"][1] <= 1e-15 and o["info"][0] > 1e-3
    assert np.abs(s["R"] - s["R_true"]).max() > 1e-3
    scale = np.linalg.norm(o["t"][1]) / np.linalg.norm(s["t_true"][1])
    assert abs(scale - 1.0) < 0.1
    assert np.abs(o["R"] - s["R_true"]).max() < 1e-5
    assert np.abs(o["t"] / scale - s["t_true"]).max() < 1e-5
    assert np.abs(o["Q"] / scale - s["X"]).max() < 1e-5 * 20 * 20


def test_two_camera_reduction_is_ba_oracle_bit_for_bit():
    """m = 2, every point in both cameras, camera 0 at the identity, the same camera-unit threshold: the optimiser's output equals
    ba_oracle's bit for bit.  The wrappers differ in two stated places only: the old t is normalised before getRTQuality (ba_scenes starts
    from a unit t, so both wrappers see the same old t here and both accept), and the new t comes back as the optimiser left it where
    ba_oracle normalises it."""
    s = BAS.scene("n65")
    assert s["mask"] is None
    p = np.stack([s["p1"], s["p2"]])
    R = np.stack([np.eye(3), s["R"]])
    t = np.stack([np.zeros(3), s["t"]])
    a = BAO.ba_oracle(s["p1"], s["p2"], s["R"], s["t"], s["Q"], s["th"], None, BAS.ANGLE_THRESH, BAS.T_NORM_THRESH)
    b = BMO.ba_multicam_oracle(p, np.ones((2, 65), np.uint8), R, t, s["Q"], s["th"], BAS.ANGLE_THRESH, BAS.T_NORM_THRESH)
    assert a["accepted"] and b["accepted"]
    assert np.array_equal(a["info"], b["info"]) and a["mu"] == b["mu"]
    assert a["trace"] == b["trace"] and a["attempts"] == b["attempts"] and len(a["trace"]) > 5
    assert np.array_equal(a["Q"], b["Q"]) and np.array_equal(a["R"], b["R"][1])
    # the stated differences, and nothing else: t un-normalised here, normalised there; camera 0 back through the quaternion round trip
    t_opt = b["t"][1]
    t_norm = np.sqrt(t_opt[0] * t_opt[0] + t_opt[1] * t_opt[1] + t_opt[2] * t_opt[2])
    assert abs(t_norm - 1.0) > 1e-4, "the scene must exercise the normalisation"
    assert np.array_equal(a["t"], t_opt / t_norm) and not np.array_equal(a["t"], t_opt)
    assert np.array_equal(b["R"][0], np.eye(3)) and np.array_equal(b["t"][0], np.zeros(3))
    # the optimiser alone, on the same arguments
    r0 = np.array([[1.0, 0, 0, 0], BAO.mat_to_quat(s["R"]) * (1.0 / np.sqrt(BAO.mat_to_quat(s["R"]) @ BAO.mat_to_quat(s["R"])))])
    assert r0[1, 0] > 0
    oa = BAO.sba_motstr(s["p1"], s["p2"], r0[1], s["t"], s["Q"], s["th"])
    ob = BMO.sba_motstr_multicam(p, np.ones((2, 65), bool), r0, t, s["Q"], s["th"])
    assert np.array_equal(oa["v"], ob["v"][1]) and np.array_equal(oa["t"], ob["t"][1]) and np.array_equal(oa["M"], ob["M"])
    assert np.array_equal(ob["v"][0], np.zeros(3)) and np.array_equal(ob["t"][0], np.zeros(3))
    assert np.array_equal(oa["info"], ob["info"]) and oa["mu"] == ob["mu"] and oa["trace"] == ob["trace"]


@pytest.mark.parametrize("name", list(BAS.BRANCH_SCENES))
def test_two_camera_reduction_over_the_branch_scenes(name):
    """The same reduction at every exit of the optimiser, branch of the wrapper and edge size: each scene of ba_scenes.BRANCH_SCENES as a
    two-camera problem (S.two_camera) gives info and mu bit for bit as ba_oracle does on the scene itself, and the same verdict.  So what
    test_oracle_bundle_adjust.py finds in each scene (the stop, the rejected attempts, the refused solves, first_bad) and the scene's
    permutation tolerances stand behind ba_multicam_oracle at m = 2, which is what test_gpu_ba_multicam.py holds the device to."""
    a, b = BAS.oracle_result(name), S.two_camera_oracle_result(name)
    print(name, BAS.integers(a), BAS.integers(b))
    assert a["accepted"] == b["accepted"]
    assert np.asarray(a["info"]).tobytes() == np.asarray(b["info"]).tobytes()
    assert np.array([a["mu"]]).tobytes() == np.array([b["mu"]]).tobytes()


def test_refusals():
    # fewer measurements than unknowns: the optimiser refuses, info stays zero, everything comes back
    s, o = S.scene("m3_n15_short"), S.oracle_result("m3_n15_short")
    assert 2 * int(s["vis"].sum()) == 60 < 6 * 3 + 3 * 15
    assert not o["accepted"] and not o["info"].any() and o["mu"] == 0.0
    assert np.array_equal(o["R"], s["R"]) and np.array_equal(o["t"], s["t"]) and np.array_equal(o["Q"], s["Q"])
    # one measurement more than the boundary needs is taken
    s2 = S.make_scene(3, 15, seed=2, vis=S.vis_frac(0.8))
    assert 2 * int(s2["vis"].sum()) >= 63
    assert BMO.ba_multicam_oracle(s2["p"], s2["vis"], s2["R"], s2["t"], s2["Q"], s2["th"])["info"][7] > 0
    # fewer than 15 points: the facade's rule
    s3 = S.make_scene(3, 14, seed=2, vis=S.vis_all)
    ps, maps = S.compacted(s3)
    assert BMO.refine_mult_cam_ba(ps, maps, s3["R"], s3["t"], s3["Q"], [S.K] * 3) is None
    # a start far beyond angleThresh: the optimiser runs, the wrapper refuses, everything is restored
    s4, o4 = S.scene("rejected"), S.oracle_result("rejected")
    assert not o4["accepted"] and o4["info"][5] > 0 and o4["info"][6] <= 5 and o4["refused_by"] == (("angle", 2),)
    assert np.array_equal(o4["R"], s4["R"]) and np.array_equal(o4["t"], s4["t"]) and np.array_equal(o4["Q"], s4["Q"])
    assert not np.array_equal(o4["t_opt"], s4["t"])


def test_unseen_point_keeps_its_coordinates():
    s, o = S.scene("unseen_point"), S.oracle_result("unseen_point")
    assert not s["vis"][:, S.UNSEEN_ROW].any() and s["vis"][:, S.CAM0_ONLY_ROW].tolist() == [1, 0, 0]
    assert o["accepted"]
    assert np.array_equal(o["Q"][S.UNSEEN_ROW], s["Q"][S.UNSEEN_ROW])
    assert not np.array_equal(o["Q"][S.CAM0_ONLY_ROW], s["Q"][S.CAM0_ONLY_ROW])        # it moves, without a W
    moved = np.any(o["Q"] != s["Q"], axis=1)
    assert moved.sum() == s["n"] - 1


def test_scenes_are_what_their_names_say():
    for name, row in S.SCENES.items():
        s = S.scene(name)
        assert s["vis"].shape == (row["m"], row["n"])
    per_point = lambda name: S.scene(name)["vis"].sum(axis=0)
    assert set(per_point("m3_n15_short")) == {2}
    assert per_point("m3_n64").min() >= 2 and per_point("m16_n128").min() >= 2
    assert {2, 3, 4} <= set(per_point("m4_n257"))
    assert S.scene("m5_sparse_cam")["vis"][4].sum() == 7
    v = S.scene("m5_disjoint")["vis"]
    assert not (v[1] & v[3]).any() and v[1].sum() > 20 and v[3].sum() > 20
    assert abs(S.scene("m8_n1000")["vis"].mean() - 0.5) < 0.05 and abs(S.scene("m16_n128")["vis"].mean() - 0.4) < 0.05
    assert not np.allclose(S.scene("cam0_not_identity")["R"][0], np.eye(3), atol=0.1)
    o = S.oracle_result("cam0_not_identity")
    s = S.scene("cam0_not_identity")
    assert o["accepted"] and np.array_equal(o["t"][0], s["t"][0])
    assert not np.array_equal(o["R"][0], s["R"][0]) and np.abs(o["R"][0] - s["R"][0]).max() < 1e-15      # the quaternion round trip
    for name in S.SCENES:
        assert S.oracle_result(name)["accepted"] == (name not in S.REFUSED), name


def test_threshold_conversion():
    Ks = [S.K, S.K * np.array([[1.0, 1, 1], [1, 1.2, 1], [1, 1, 1]])]
    assert BMO.convert_threshold_multicam(Ks) == 0.005 / (((700.0 + 1.0) / 2.0 + (840.0 + 1.0) / 2.0) / 2.0)
    assert BMO.convert_threshold_multicam(Ks, 0.5) == 0.5 / (((700.0 + 1.0) / 2.0 + (840.0 + 1.0) / 2.0) / 2.0)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_permutation_study_sets_the_tolerances(name):
    """The device differs from the oracle only in the association of its sums over points; permuting the points changes the order of every
    such sum inside the oracle.  The verdict and every integer must not move; each constant lies between 10 x and 100 x the measured spread."""
    sp, tol = S.spread(name), S.tol(name)
    print(name, {k: sp[k] for k in ("pose", "q", "info", "mu")}, tol)
    assert sp["stable"], "a permutation changed the verdict, the iteration count, the stop reason or a count: pick another seed"
    for key in ("pose", "q", "info", "mu"):
        if sp[key] == 0.0:
            assert tol[key] == 0.0, (name, key)
        else:
            assert 10 * sp[key] <= tol[key] <= 100 * sp[key], (name, key, sp[key], tol[key])
