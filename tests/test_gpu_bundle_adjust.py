"""poselib::refineStereoBA on the MI355X (mlpl_refine_stereo_ba, its device and batch forms, the Python surfaces, the C++ drop-in and
StereoRefine's BART = 1 / BART_CorrPool = 1) against the float64 restatement in ba_oracle.py.  The verdict, the iteration count, the stop
reason and the evaluation / solve counts are compared exactly -- test_oracle_bundle_adjust.py shows that they do not depend on the order of
the sums for these scenes --, R, t, Q, info[0..1] and mu to the tolerances of ba_scenes.py, which come from that same study."""
import os
import subprocess

import numpy as np
import pytest

import ba_oracle as BAO
import ba_scenes as S
import triang_pts3d_oracle as TPO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "bundle_adjust_facade")
SR_EXE = os.path.join(ROOT, "tests", "cpp", "stereo_refine_ba_driver")

_single = {}


def _gpu_single(ctx, name):
    from matchinglib_poselib_amd import pose

    if name not in _single:
        s = S.scene(name)
        _single[name] = pose.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], s["th"], s["mask"], S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    return _single[name]


def _close(r, o, what):
    """r: device result, o: oracle result."""
    got = (bool(r["accepted"]),) + tuple(int(x) for x in r["info"][5:10])
    print(what, "integers", got, "dR %.3g dt %.3g" % (np.abs(r["R"] - o["R"]).max(), np.abs(r["t"] - o["t"]).max()),
          "info", [abs(r["info"][i] - o["info"][i]) / abs(o["info"][i]) if o["info"][i] else 0.0 for i in (0, 1)],
          "mu", abs(r["mu"] - o["mu"]) / abs(o["mu"]) if o["mu"] else 0.0)
    assert got == S.integers(o), what
    assert np.abs(r["R"] - o["R"]).max() <= S.TOL_POSE and np.abs(r["t"] - o["t"]).max() <= S.TOL_POSE, what
    for i in (0, 1):
        assert abs(r["info"][i] - o["info"][i]) <= S.TOL_INFO * abs(o["info"][i]), (what, i)
    assert abs(r["mu"] - o["mu"]) <= S.TOL_MU * abs(o["mu"]), what
    if "Q" in r:
        print(what, "dQ %.3g" % np.abs(r["Q"] - o["Q"]).max())
        assert np.abs(r["Q"] - o["Q"]).max() <= S.TOL_Q, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(S.SCENES))
def test_single_host_and_device(ctx, name):
    import torch
    from matchinglib_poselib_amd import pose

    s, o = S.scene(name), S.oracle_result(name)
    r = _gpu_single(ctx, name)
    _close(r, o, name)
    if s["mask"] is not None:
        out = s["mask"] == 0
        assert out.any() and r["Q"][out].tobytes() == s["Q"][out].tobytes(), "rows outside the mask are untouched"
    if not o["accepted"]:
        assert r["R"].tobytes() == s["R"].tobytes() and r["t"].tobytes() == s["t"].tobytes() and r["Q"].tobytes() == s["Q"].tobytes()
    else:
        assert not np.array_equal(r["Q"], s["Q"])
    d1, d2, dq = torch.from_numpy(s["p1"]).cuda(), torch.from_numpy(s["p2"]).cuda(), torch.from_numpy(s["Q"].copy()).cuda()
    dm = None if s["mask"] is None else torch.from_numpy(s["mask"].copy()).cuda()
    d = pose.refine_stereo_ba_device(d1, d2, s["R"], s["t"], dq, s["th"], dm, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    torch.cuda.synchronize()
    assert d["accepted"] == r["accepted"] and d["R"].tobytes() == r["R"].tobytes() and d["t"].tobytes() == r["t"].tobytes()
    assert d["info"].tobytes() == r["info"].tobytes() and d["mu"] == r["mu"] and dq.cpu().numpy().tobytes() == r["Q"].tobytes()
    if dm is not None:
        assert dm.cpu().numpy().tobytes() == s["mask"].tobytes()


@pytest.mark.gpu
def test_all_zero_mask_returns_zero_and_touches_nothing(ctx):
    from matchinglib_poselib_amd import pose

    s = S.scene("n64")
    r = pose.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], s["th"], np.zeros(64, np.uint8), S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    assert not r["accepted"] and not r["info"].any()
    assert r["R"].tobytes() == s["R"].tobytes() and r["t"].tobytes() == s["t"].tobytes() and r["Q"].tobytes() == s["Q"].tobytes()


BATCH = ("n7", "n65", "rejected", "n1000_masked", None, "n64")      # valid points 7, 65, 257, 1000, 0, 64


def _batch_arrays():
    stride = 1700
    B = len(BATCH)
    P1, P2 = np.full((B, stride, 2), 0.25), np.full((B, stride, 2), 0.25)
    Q, M = np.full((B, stride, 3), -7.0), np.full((B, stride), 5, np.uint8)
    R, t, counts = np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros(B, np.int32)
    for b, name in enumerate(BATCH):
        s = S.scene(name or "n64")
        n = 0 if name is None else s["p1"].shape[0]
        counts[b], R[b], t[b] = n, s["R"], s["t"]
        P1[b, :n], P2[b, :n], Q[b, :n] = s["p1"][:n], s["p2"][:n], s["Q"][:n]
        M[b, :n] = 1 if s["mask"] is None else s["mask"][:n]
    return stride, counts, P1, P2, Q, M, R, t


@pytest.mark.gpu
def test_batch_equals_single(ctx):
    import torch
    from matchinglib_poselib_amd import pose

    stride, counts, P1, P2, Q0, M, R, t = _batch_arrays()
    d1, d2, dm = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda(), torch.from_numpy(M.copy()).cuda()
    runs = []
    for _ in range(2):
        dq = torch.from_numpy(Q0.copy()).cuda()
        res = pose.refine_stereo_ba_batch(d1, d2, counts, R, t, dq, S.TH, dm, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
        torch.cuda.synchronize()
        runs.append((res, dq.cpu().numpy()))
    (res, Qb), (res2, Qb2) = runs
    for k in ("accepted", "R", "t", "info", "mu"):
        assert res[k].tobytes() == res2[k].tobytes(), k                          # two identical calls give identical bits
    assert Qb.tobytes() == Qb2.tobytes() and dm.cpu().numpy().tobytes() == M.tobytes()
    assert list(res["accepted"]) == [False, True, False, True, False, True]
    for b, name in enumerate(BATCH):
        n = counts[b]
        assert Qb[b, n:].tobytes() == Q0[b, n:].tobytes(), "points beyond counts[b] are untouched"
        if name is None:
            assert not res["info"][b].any() and res["R"][b].tobytes() == R[b].tobytes() and res["t"][b].tobytes() == t[b].tobytes()
            continue
        r = _gpu_single(ctx, name)
        assert bool(res["accepted"][b]) == r["accepted"] and res["R"][b].tobytes() == r["R"].tobytes() and res["t"][b].tobytes() == r["t"].tobytes(), name
        assert res["info"][b].tobytes() == r["info"].tobytes() and res["mu"][b] == r["mu"] and Qb[b, :n].tobytes() == r["Q"].tobytes(), name


@pytest.mark.gpu
def test_chain_behind_triang_pts3d(ctx, oracle):
    """mlpl_triang_pts3d_batch_dev -> mlpl_refine_stereo_ba_batch_dev on the same device buffers, no host copy of points or masks in between.
    Bit for bit it equals the single entry fed with the triangulated points; against the two restatements in a row the bar is wider than
    ba_scenes' constants, because the triangulation itself is only held to rtol = atol = 1e-9 (test_gpu_triang_pts3d.py): 10 x the largest
    change that five random perturbations of that size of the oracle's triangulated points make in ba_oracle's result (and they must leave
    its integers alone, as the permutations must)."""
    import torch
    from matchinglib_poselib_amd import pose

    names = ("n64", "n257", "n65")
    stride, B = 300, len(names)
    P1, P2, M = np.zeros((B, stride, 2)), np.zeros((B, stride, 2)), np.full((B, stride), 5, np.uint8)
    R, t, counts = np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros(B, np.int32)
    for b, name in enumerate(names):
        s = S.scene(name)
        n = s["p1"].shape[0]
        counts[b], R[b], t[b] = n, s["R"], s["t"]
        P1[b, :n], P2[b, :n], M[b, :n] = s["p1"], s["p2"], 1
    d1, d2, dm = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda(), torch.from_numpy(M.copy()).cuda()
    dq = torch.full((B, stride, 3), -7.0, dtype=torch.float64, device="cuda")
    good = pose.triang_pts3d_batch(d1, d2, counts, R, t, dm, dq, 50.0, ctx=ctx)
    Qt, Mt = dq.cpu().numpy(), dm.cpu().numpy()                                 # read for the checks only; the chain runs on dq / dm
    res = pose.refine_stereo_ba_batch(d1, d2, counts, R, t, dq, S.TH, dm, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    torch.cuda.synchronize()
    Qb = dq.cpu().numpy()
    assert dm.cpu().numpy().tobytes() == Mt.tobytes()
    for b, name in enumerate(names):
        s, n = S.scene(name), counts[b]
        one = pose.refine_stereo_ba(s["p1"], s["p2"], R[b], t[b], Qt[b, :n], S.TH, Mt[b, :n], S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
        assert bool(res["accepted"][b]) == one["accepted"] and res["R"][b].tobytes() == one["R"].tobytes() and res["t"][b].tobytes() == one["t"].tobytes()
        assert res["info"][b].tobytes() == one["info"].tobytes() and Qb[b, :n].tobytes() == one["Q"].tobytes() and Qb[b, n:].tobytes() == Qt[b, n:].tobytes()
        ot = TPO.triang_pts3d(oracle, R[b], t[b], s["p1"], s["p2"], M[b, :n], 50.0)
        assert ot["margin"] > 1e-9 and good[b] == ot["n_good"] and Mt[b, :n].tobytes() == ot["mask"].tobytes() and ot["n_good"] >= 0.7 * n
        ob = BAO.ba_oracle(s["p1"], s["p2"], R[b], t[b], ot["Q"], S.TH, ot["mask"], S.ANGLE_THRESH, S.T_NORM_THRESH)
        assert ob["accepted"]
        rng = np.random.default_rng(77 + b)
        keep = ot["mask"] != 0
        spread = dict(pose=0.0, q=0.0, info=0.0)
        for _ in range(5):
            Qp = ot["Q"] * (1.0 + 1e-9 * rng.uniform(-1, 1, ot["Q"].shape)) + 1e-9 * rng.uniform(-1, 1, ot["Q"].shape)
            op = BAO.ba_oracle(s["p1"], s["p2"], R[b], t[b], Qp, S.TH, ot["mask"], S.ANGLE_THRESH, S.T_NORM_THRESH)
            assert S.integers(op) == S.integers(ob), "pick another scene"
            spread["pose"] = max(spread["pose"], np.abs(op["R"] - ob["R"]).max(), np.abs(op["t"] - ob["t"]).max())
            spread["q"] = max(spread["q"], np.abs(op["Q"][keep] - ob["Q"][keep]).max())
            spread["info"] = max(spread["info"], max(abs(op["info"][i] - ob["info"][i]) / abs(ob["info"][i]) for i in (0, 1)))
        got = (bool(res["accepted"][b]),) + tuple(int(x) for x in res["info"][b][5:10])
        dq_, dp_ = np.abs(Qb[b, :n][keep] - ob["Q"][keep]).max(), max(np.abs(res["R"][b] - ob["R"]).max(), np.abs(res["t"][b] - ob["t"]).max())
        print(name, got, "dQ %.3g (10 x spread %.3g) dpose %.3g (%.3g)" % (dq_, 10 * spread["q"], dp_, 10 * spread["pose"]))
        assert got == S.integers(ob), name
        assert dq_ <= 10 * spread["q"] and dp_ <= 10 * spread["pose"], name
        for i in (0, 1):
            assert abs(res["info"][b][i] - ob["info"][i]) <= 10 * spread["info"] * abs(ob["info"][i]), name


@pytest.mark.gpu
def test_facade(ctx, tmp_path):
    """poselib::refineStereoBA(p1, p2, R, t, Q, K1, K2, false, mask) equals the C entry with the converted threshold; every refused option
    returns false with its arguments untouched."""
    from matchinglib_poselib_amd import pose

    assert os.path.exists(FACADE_EXE), "built by the facade Makefile's check target"
    s = S.scene("n1000_masked")
    n = s["p1"].shape[0]
    K1 = np.array([[650.0, 0, 320], [0, 700.0, 240], [0, 0, 1]])
    K2 = np.array([[640.0, 0, 320], [0, 720.0, 240], [0, 0, 1]])
    th = pose.ba_threshold(K1, K2)
    assert th == BAO.convert_threshold(K1, K2) == 4.0 * 0.005 / (np.sqrt(2.0) * 1422.0)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.array([n], np.int32).tobytes() + K1.tobytes() + K2.tobytes() + np.ascontiguousarray(s["R"]).tobytes() + s["t"].tobytes() +
                    s["p1"].tobytes() + s["p2"].tobytes() + s["Q"].tobytes() + s["mask"].tobytes())
    out = subprocess.run([FACADE_EXE, str(src), str(dst)], check=True, timeout=120, stdout=subprocess.PIPE).stdout.decode()
    rec = np.dtype([("ret", np.int32), ("R", np.float64, 9), ("t", np.float64, 3), ("Q", np.float64, (n, 3))])
    raw = dst.read_bytes()
    recs = np.frombuffer(raw[:7 * rec.itemsize], rec)
    tail = np.frombuffer(raw[7 * rec.itemsize:], np.int32)
    masked = pose.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], th, s["mask"], ctx=ctx)
    plain = pose.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], th, None, ctx=ctx)
    for r, want in ((recs[0], masked), (recs[1], plain)):
        assert r["ret"] == int(want["accepted"]) and r["R"].tobytes() == want["R"].tobytes() and r["t"].tobytes() == want["t"].tobytes()
        assert r["Q"].tobytes() == want["Q"].tobytes()
    assert masked["accepted"] and not np.array_equal(masked["Q"], plain["Q"])
    for r in recs[2:]:
        assert r["ret"] == 0 and r["R"].tobytes() == np.ascontiguousarray(s["R"]).tobytes() and r["t"].tobytes() == s["t"].tobytes()
        assert r["Q"].tobytes() == s["Q"].tobytes()
    assert out.count("is not built.") == 5 and list(tail) == [0, 0]


# ---- StereoRefine -----------------------------------------------------------------------------------------------------------------------------
def _run_stereo_refine(tmp_path, tag, cfg_kw, frames, bart, bart_pool, seed=777):
    from stereo_refine_linear_oracle import LinearCfg
    from test_gpu_stereo_refine import K

    cfg = LinearCfg(**cfg_kw)
    fin, fout = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    with open(fin, "wb") as f:
        np.array([len(frames), 0], np.int32).tofile(f)
        np.array([seed], np.uint32).tofile(f)
        K.tofile(f)
        K.tofile(f)
        np.zeros(16).tofile(f)
        cfg.as_doubles().tofile(f)
        cfg.linear_ints().tofile(f)
        np.array([bart, bart_pool], np.int32).tofile(f)
        for kp1, kp2, dd in frames:
            np.array([len(dd)], np.int32).tofile(f)
            kp1.tofile(f)
            kp2.tofile(f)
            dd.tofile(f)
    text = subprocess.run([SR_EXE, str(fin), str(fout)], check=True, timeout=300, stdout=subprocess.PIPE).stdout.decode()
    raw, at, out = fout.read_bytes(), 0, []
    head = np.dtype([("st", np.int32, 10), ("E", np.float64, 9), ("R", np.float64, 9), ("t", np.float64, 3), ("Eml", np.float64, 9), ("ba", np.int32, 3)])
    for _ in frames:
        h = np.frombuffer(raw, head, 1, at)[0]
        at += head.itemsize
        m = int(h["ba"][2])
        fr = dict(st=h["st"].copy(), E=h["E"].reshape(3, 3).copy(), R=h["R"].reshape(3, 3).copy(), t=h["t"].copy(), calls=int(h["ba"][0]),
                  accepted=bool(h["ba"][1]))
        if m:
            body = np.frombuffer(raw, np.float64, 12 + 7 * m, at)
            at += 8 * (12 + 7 * m)
            fr.update(ba_R=body[:9].reshape(3, 3), ba_t=body[9:12], p1=body[12:12 + 2 * m].reshape(m, 2), p2=body[12 + 2 * m:12 + 4 * m].reshape(m, 2),
                      Q=body[12 + 4 * m:].reshape(m, 3), mask=np.frombuffer(raw, np.uint8, m, at))
            at += m
        out.append(fr)
    assert at == len(raw)
    return out, text


def _e_from_rt(R, t):
    tn = t / np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    Sx = np.array([[0, -tn[2], tn[1]], [tn[2], 0, -tn[0]], [-tn[1], tn[0], 0]])
    return Sx @ R


def _expect_frame(ctx, fr, K):
    """The pose a frame must hold after its bundle adjustment: the single entry on what the adjustment was called with."""
    from matchinglib_poselib_amd import pose

    K3 = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    r = pose.refine_stereo_ba(fr["p1"], fr["p2"], fr["ba_R"], fr["ba_t"], fr["Q"], pose.ba_threshold(K3, K3), fr["mask"], ctx=ctx)
    assert r["accepted"] == fr["accepted"]
    t = r["t"] / np.sqrt(r["t"][0] * r["t"][0] + r["t"][1] * r["t"][1] + r["t"][2] * r["t"][2])
    assert fr["R"].tobytes() == r["R"].tobytes() and fr["t"].tobytes() == t.tobytes()
    assert np.abs(fr["E"] - _e_from_rt(r["R"], r["t"])).max() <= 4 * np.finfo(float).eps      # E = [t]x R of the refined pose
    return r


@pytest.mark.gpu
def test_stereo_refine_bart_after_the_robust_estimate(ctx, tmp_path):
    """The first frame with BART = 1 equals the first frame with BART = 0 followed by refine_stereo_ba on that frame's points, pose, 3-D points
    and mask."""
    from test_gpu_stereo_refine import POSE_A, K, frame

    rng = np.random.default_rng(41)
    frames = [frame(rng, 450, POSE_A, 0.25)]
    kw = dict(checkPoolPoseRobust=1)
    off, text0 = _run_stereo_refine(tmp_path, "bart0", kw, frames, 0, 0)
    on, text1 = _run_stereo_refine(tmp_path, "bart1", kw, frames, 1, 0)
    assert off[0]["calls"] == 0 and on[0]["calls"] == 1 and on[0]["st"][0] == off[0]["st"][0] == 0
    assert "is not built" not in text1 and "is not built" not in text0
    f0, f1 = off[0], on[0]
    # what the adjustment was called with is what BART = 0 ends with (t there is stored normalised)
    tn = f1["ba_t"] / np.sqrt(f1["ba_t"][0] * f1["ba_t"][0] + f1["ba_t"][1] * f1["ba_t"][1] + f1["ba_t"][2] * f1["ba_t"][2])
    assert f1["ba_R"].tobytes() == f0["R"].tobytes() and tn.tobytes() == f0["t"].tobytes()
    assert f1["p1"].shape[0] == 450 and 100 < np.count_nonzero(f1["mask"]) < 450
    r = _expect_frame(ctx, f1, K)
    assert r["accepted"] and not np.array_equal(f1["R"], f0["R"]) and ("Bundle adjustment failed!" in text1) == (not r["accepted"])


@pytest.mark.gpu
def test_stereo_refine_bart_on_the_pool(ctx, tmp_path):
    """BART_CorrPool = 1: the first refinement on the pool ends with the single entry's pose on the pool's points."""
    from test_gpu_stereo_refine import POSE_A, K, frame

    rng = np.random.default_rng(42)
    frames = [frame(rng, 400, POSE_A, 0.2) for _ in range(4)]
    kw = dict(checkPoolPoseRobust=3, refineMethod_CorrPool=0x23)
    on, text = _run_stereo_refine(tmp_path, "pool1", kw, frames, 0, 1)
    first = next((k for k, fr in enumerate(on) if fr["calls"] == 1), None)
    assert first is not None and first >= 1 and on[first - 1]["calls"] == 0, [fr["calls"] for fr in on]
    fr = on[first]
    assert fr["p1"].shape[0] > 400                                           # the pool, not the frame's own matches
    _expect_frame(ctx, fr, K)
    v2, text2 = _run_stereo_refine(tmp_path, "pool2", kw, frames[:2], 2, 2)
    assert all(f["calls"] == 0 for f in v2) and text2.count("BART = 2") == 1   # value 2 is announced as not built and skipped
