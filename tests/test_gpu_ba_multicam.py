"""poselib::refineMultCamBA on the MI355X (mlpl_refine_multicam_ba, its device and batch forms, the Python surfaces and the C++ drop-in)
against the float64 restatement in ba_multicam_oracle.py.  The verdict, the iteration count, the stop reason and the evaluation / solve counts
are compared exactly -- test_oracle_ba_multicam.py shows that they do not depend on the order of the sums for these scenes --, R, t, Q,
info[0..1] and mu to each scene's tolerances in ba_multicam_scenes.py, which come from that same study."""
import os
import subprocess

import numpy as np
import pytest

import ba_multicam_oracle as BMO
import ba_multicam_scenes as S
import ba_scenes as BAS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "ba_multicam_facade")

_single = {}


def _gpu_single(ctx, name):
    from matchinglib_poselib_amd import pose

    if name not in _single:
        s = S.scene(name)
        _single[name] = pose.refine_multicam_ba(s["p"], s["vis"], s["R"], s["t"], s["Q"], s["th"], S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    return _single[name]


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(S.SCENES))
def test_single_host_and_device(ctx, name):
    import torch
    from matchinglib_poselib_amd import pose

    s, o, tol = S.scene(name), S.oracle_result(name), S.tol(name)
    vis_before = s["vis"].copy()
    r = _gpu_single(ctx, name)
    got = (bool(r["accepted"]),) + tuple(int(x) for x in r["info"][5:10])
    d_pose = max(np.abs(r["R"] - o["R"]).max(), np.abs(r["t"] - o["t"]).max())
    d_q = np.abs(r["Q"] - o["Q"]).max()
    d_info = max(S.rel_diff(r["info"][i], o["info"][i]) for i in (0, 1))
    d_mu = S.rel_diff(r["mu"], o["mu"])
    print(name, "integers", got, "dpose %.3g dQ %.3g info %.3g mu %.3g" % (d_pose, d_q, d_info, d_mu), tol)
    assert got == S.integers(o), name
    assert d_pose <= tol["pose"] and d_q <= tol["q"] and d_info <= tol["info"] and d_mu <= tol["mu"], name
    assert _same_bits(s["vis"], vis_before)
    if name in S.REFUSED:
        assert not r["accepted"]
        assert _same_bits(r["R"], s["R"]) and _same_bits(r["t"], s["t"]) and _same_bits(r["Q"], s["Q"])
    else:
        assert r["accepted"] and not np.array_equal(r["Q"], s["Q"])
    if name == "unseen_point":
        assert _same_bits(r["Q"][S.UNSEEN_ROW], s["Q"][S.UNSEEN_ROW]) and not np.array_equal(r["Q"][S.CAM0_ONLY_ROW], s["Q"][S.CAM0_ONLY_ROW])
    if name == "cam0_not_identity":       # camera 0: fixed at its pose, its R back through the quaternion round trip, its t as it came
        assert _same_bits(r["t"][0], s["t"][0]) and np.abs(r["R"][0] - s["R"][0]).max() < 1e-15
    dp, dv, dq = torch.from_numpy(s["p"]).cuda(), torch.from_numpy(s["vis"].copy()).cuda(), torch.from_numpy(s["Q"].copy()).cuda()
    d = pose.refine_multicam_ba_device(dp, dv, s["R"], s["t"], dq, s["th"], S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    torch.cuda.synchronize()
    assert d["accepted"] == r["accepted"] and _same_bits(d["R"], r["R"]) and _same_bits(d["t"], r["t"])
    assert _same_bits(d["info"], r["info"]) and d["mu"] == r["mu"] and _same_bits(dq.cpu().numpy(), r["Q"])
    assert _same_bits(dv.cpu().numpy(), s["vis"])


@pytest.mark.gpu
def test_two_cameras_against_the_stereo_entry(ctx):
    """m2_full_n65 through the new entry and through pose.refine_stereo_ba on the same data and camera-unit threshold: the stereo kernel fixes
    camera 0 at the identity, which is where the scene puts it.  Verdict and integers equal; R and Q within the two kernels' tolerances
    added; t equal after normalising the new entry's."""
    from matchinglib_poselib_amd import pose

    s, tol = S.scene("m2_full_n65"), S.tol("m2_full_n65")
    assert np.array_equal(s["R"][0], np.eye(3)) and not s["t"][0].any() and s["vis"].all()
    r = _gpu_single(ctx, "m2_full_n65")
    st = pose.refine_stereo_ba(s["p"][0], s["p"][1], s["R"][1], s["t"][1], s["Q"], s["th"], None, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    assert r["accepted"] and st["accepted"]
    assert [int(x) for x in r["info"][5:10]] == [int(x) for x in st["info"][5:10]]
    t_new = r["t"][1] / np.sqrt(r["t"][1][0] * r["t"][1][0] + r["t"][1][1] * r["t"][1][1] + r["t"][1][2] * r["t"][1][2])
    print("dR %.3g dt %.3g dQ %.3g" % (np.abs(r["R"][1] - st["R"]).max(), np.abs(t_new - st["t"]).max(), np.abs(r["Q"] - st["Q"]).max()))
    assert np.abs(r["R"][1] - st["R"]).max() <= BAS.TOL_POSE + tol["pose"]
    assert np.abs(t_new - st["t"]).max() <= BAS.TOL_POSE + tol["pose"]
    assert np.abs(r["Q"] - st["Q"]).max() <= BAS.TOL_Q + tol["q"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BAS.BRANCH_SCENES))
def test_branch_scene_as_two_cameras(ctx, name):
    """Every exit of the optimiser (stops 1 to 7, rejected attempts, refused solves, both first_bad repairs) and the edge sizes through THIS
    kernel: the scenes of ba_scenes.BRANCH_SCENES at m = 2 (S.two_camera) against ba_multicam_oracle on the same arguments.
    test_oracle_ba_multicam.py shows that this oracle gives there what ba_oracle gives on the stereo scene, so the scene's own tolerances
    hold; they were derived for entries of R and t of size at most 1 and this entry returns t un-normalised, hence tol * max(1, |t|)."""
    from matchinglib_poselib_amd import pose

    row, s, o = BAS.BRANCH_SCENES[name], S.two_camera(name), S.two_camera_oracle_result(name)
    tol, kind = row["tol"], row["kind"]
    r = pose.refine_multicam_ba(s["p"], s["vis"], s["R"], s["t"], s["Q"], s["th"], s["angle_thresh"], s["t_norm_thresh"], ctx=ctx)
    got = (bool(r["accepted"]),) + tuple(int(x) for x in r["info"][5:10])
    d_info = [S.rel_diff(r["info"][i], o["info"][i]) for i in BAS.INFO_COMPARED[kind]]
    d_mu = S.rel_diff(r["mu"], o["mu"])
    print(name, "integers", got, "info", d_info, "(%.3g)" % tol["info"], "mu %.3g (%.3g)" % (d_mu, tol["mu"]))
    assert got == S.integers(o), name
    assert max(d_info) <= tol["info"] and d_mu <= tol["mu"], name
    if o["accepted"]:
        t_size = max(1.0, np.sqrt(o["t"][1] @ o["t"][1]))
        d_R, d_t, d_q = np.abs(r["R"][1] - o["R"][1]).max(), np.abs(r["t"][1] - o["t"][1]).max(), np.abs(r["Q"] - o["Q"]).max()
        print(name, "dR %.3g dt %.3g (%.3g, |t| %.3g) dQ %.3g (%.3g)" % (d_R, d_t, tol["pose"], t_size, d_q, tol["q"]))
        assert d_R <= tol["pose"] and d_t <= tol["pose"] * t_size and d_q <= tol["q"], name
        assert np.abs(r["R"][0] - np.eye(3)).max() < 1e-15 and _same_bits(r["t"][0], s["t"][0]), name
    else:
        assert _same_bits(r["R"], s["R"]) and _same_bits(r["t"], s["t"]) and _same_bits(r["Q"], s["Q"]), name


BATCH = ("m2_full_n65", "m3_n15_short", "m4_n257", None, "m16_n128", "rejected", "m5_sparse_cam")
CAMS_STRIDE, STRIDE = 16, 320


def _batch_arrays():
    B = len(BATCH)
    P, V = np.full((B, CAMS_STRIDE, STRIDE, 2), 0.25), np.full((B, CAMS_STRIDE, STRIDE), 5, np.uint8)
    Q = np.full((B, STRIDE, 3), -7.0)
    R, t = np.full((B, CAMS_STRIDE, 3, 3), 3.0), np.full((B, CAMS_STRIDE, 3), -2.0)
    n_cams, counts, th = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
    for b, name in enumerate(BATCH):
        s = S.scene(name or "m3_n64")
        m, n = s["m"], s["n"]
        th[b] = s["th"]
        n_cams[b], counts[b] = (m, 0) if name is None else (m, n)
        R[b, :m], t[b, :m] = s["R"], s["t"]
        if name is not None:
            P[b, :m, :n], V[b, :m, :n], Q[b, :n] = s["p"], s["vis"], s["Q"]
    return n_cams, counts, th, P, V, Q, R, t


@pytest.mark.gpu
def test_batch_equals_single(ctx):
    import torch
    from matchinglib_poselib_amd import pose

    n_cams, counts, th, P, V, Q0, R, t = _batch_arrays()
    assert STRIDE > counts.max()
    dp, dv = torch.from_numpy(P).cuda(), torch.from_numpy(V.copy()).cuda()
    runs = []
    for _ in range(2):
        dq = torch.from_numpy(Q0.copy()).cuda()
        res = pose.refine_multicam_ba_batch(dp, dv, n_cams, counts, R, t, dq, th, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
        torch.cuda.synchronize()
        runs.append((res, dq.cpu().numpy()))
    (res, Qb), (res2, Qb2) = runs
    for k in ("accepted", "R", "t", "info", "mu"):
        assert _same_bits(res[k], res2[k]), k                                    # two identical calls give identical bits
    assert _same_bits(Qb, Qb2) and _same_bits(dv.cpu().numpy(), V)
    assert list(res["accepted"]) == [True, False, True, False, True, False, True]
    for b, name in enumerate(BATCH):
        n, m = counts[b], n_cams[b]
        assert _same_bits(Qb[b, n:], Q0[b, n:]), "points beyond counts[b] are untouched"
        assert _same_bits(res["R"][b, m:], R[b, m:]) and _same_bits(res["t"][b, m:], t[b, m:]), "cameras beyond n_cams[b] are untouched"
        if name is None:
            assert not res["info"][b].any() and _same_bits(res["R"][b], R[b]) and _same_bits(res["t"][b], t[b])
            continue
        r = _gpu_single(ctx, name)
        assert bool(res["accepted"][b]) == r["accepted"] and _same_bits(res["R"][b, :m], r["R"]) and _same_bits(res["t"][b, :m], r["t"]), name
        assert _same_bits(res["info"][b], r["info"]) and res["mu"][b] == r["mu"] and _same_bits(Qb[b, :n], r["Q"]), name
    # fewer than two cameras: not accepted, info zero, nothing touched
    n1 = n_cams.copy()
    n1[0] = 1
    dq = torch.from_numpy(Q0.copy()).cuda()
    one = pose.refine_multicam_ba_batch(dp, dv, n1, counts, R, t, dq, th, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    torch.cuda.synchronize()
    assert not one["accepted"][0] and not one["info"][0].any() and _same_bits(one["R"][0], R[0]) and _same_bits(one["t"][0], t[0])
    assert _same_bits(dq.cpu().numpy()[0], Q0[0]) and _same_bits(dq.cpu().numpy()[1:], Qb[1:])


@pytest.mark.gpu
def test_camera_count_limits(ctx):
    """m = 17 is not built (MLPL_E_UNSUPPORTED) and writes nothing; m = 1 is bad input."""
    import matchinglib_poselib_amd as mpa
    from matchinglib_poselib_amd import _lib, pose

    n = 40
    rng = np.random.default_rng(3)
    for m, code in ((17, _lib.MLPL_E_UNSUPPORTED), (1, _lib.MLPL_E_BAD_INPUT)):
        p, vis = rng.normal(size=(m, n, 2)), np.ones((m, n), np.uint8)
        R, t, Q = np.tile(np.eye(3), (m, 1, 1)), rng.normal(size=(m, 3)), rng.normal(size=(n, 3)) + [0, 0, 8]
        Rh, th_, Qh, info = R.reshape(m, 9).copy(), t.copy(), Q.copy(), np.full(10, 9.0)
        rc = ctx.lib.mlpl_refine_multicam_ba(ctx.handle, p.ctypes.data, vis.ctypes.data, m, n, Rh.ctypes.data, th_.ctypes.data, Qh.ctypes.data,
                                             1e-5, 1.25, 0.05, info.ctypes.data)
        assert rc == code, (m, rc)
        assert _same_bits(Rh, R) and _same_bits(th_, t) and _same_bits(Qh, Q) and (info == 9.0).all()
        with pytest.raises(mpa.MlplError) as e:
            pose.refine_multicam_ba(p, vis, R, t, Q, 1e-5, ctx=ctx)
        assert e.value.code == code


@pytest.mark.gpu
def test_facade(ctx, tmp_path):
    """poselib::refineMultCamBA(ps, map3D, Rs, ts, Qs, Ks) with compacted ps[j] equals the Python entry with ba_threshold_multicam(Ks) bit for
    bit, the un-normalised t and camera 0's round-tripped R included; every refusal returns false with its arguments untouched."""
    from matchinglib_poselib_amd import pose

    assert os.path.exists(FACADE_EXE), "built by the facade Makefile's check target"
    s = S.scene("m4_n257")
    m, n = s["m"], s["n"]
    Ks = [np.array([[650.0 + 10 * j, 0, 320], [0, 700.0 + 5 * j, 240], [0, 0, 1]]) for j in range(m)]
    th = pose.ba_threshold_multicam(Ks)
    assert th == BMO.convert_threshold_multicam(Ks) == 0.005 / ((2830.0 + 4.0) / 2.0 / 4.0)
    ps, maps = S.compacted(s)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([m, n], np.int32).tofile(f)
        for j in range(m):
            Ks[j].tofile(f)
            np.ascontiguousarray(s["R"][j]).tofile(f)
            s["t"][j].tofile(f)
            maps[j].tofile(f)
            np.array([ps[j].shape[0]], np.int32).tofile(f)
            ps[j].tofile(f)
        s["Q"].tofile(f)
    out = subprocess.run([FACADE_EXE, str(src), str(dst)], check=True, timeout=120, stdout=subprocess.PIPE).stdout.decode()
    rec = np.dtype([("ret", np.int32), ("R", np.float64, (m, 9)), ("t", np.float64, (m, 3)), ("Q", np.float64, (n, 3))])
    recs = np.frombuffer(dst.read_bytes(), rec)
    assert len(recs) == 11
    want = pose.refine_multicam_ba(s["p"], s["vis"], s["R"], s["t"], s["Q"], th, ctx=ctx)
    assert want["accepted"] and abs(np.linalg.norm(want["t"][1]) - 1.0) > 1e-4      # a t that a normalising wrapper would have changed
    # defaults; all-ones masks; optimFocalOnly; fixCamMat
    for r in recs[:4]:
        assert r["ret"] == 1 and _same_bits(r["R"], want["R"]) and _same_bits(r["t"], want["t"]) and _same_bits(r["Q"], want["Q"])
    # pointsInImgCoords, optimMotionOnly, a zero in masks | 14 points, a map whose count disagrees, a CV_8UC1 map, vectors of differing length
    for r in recs[4:]:
        assert r["ret"] == 0 and _same_bits(r["R"], s["R"]) and _same_bits(r["t"], s["t"]) and _same_bits(r["Q"], s["Q"])
    assert out.count("is not built.") == 3
