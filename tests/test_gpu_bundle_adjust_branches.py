"""refineStereoBA on the MI355X at every exit of the optimiser, every branch of the wrapper and the edge sizes: the scenes of
ba_scenes.BRANCH_SCENES against ba_oracle.py.  test_oracle_bundle_adjust.py shows on the CPU that the oracle takes, in each scene, the branch
the scene is named for, and that its six integers do not depend on the order of the sums; here the device must give those integers exactly and
the values to the scene's OWN tolerances (10 x its own permutation spread; 0 = bit for bit).  A scene the oracle refuses or fails must come back
byte for byte as it went in."""
import numpy as np
import pytest

import ba_scenes as S

_single = {}


def _gpu_single(ctx, name, own_thresholds=True):
    from matchinglib_poselib_amd import pose

    key = (name, own_thresholds)
    if key not in _single:
        s = S.scene(name)
        at, tt = (s["angle_thresh"], s["t_norm_thresh"]) if own_thresholds else (S.ANGLE_THRESH, S.T_NORM_THRESH)
        if (at, tt) == (S.ANGLE_THRESH, S.T_NORM_THRESH):
            key = (name, False)
        if key not in _single:
            _single[key] = pose.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], s["th"], s["mask"], at, tt, ctx=ctx)
    return _single[key]


def _hold(r, name):
    """r: the device's result on scene `name`, held to the oracle's by the scene's kind."""
    row, s, o = S.BRANCH_SCENES[name], S.scene(name), S.oracle_result(name)
    tol, kind = row["tol"], row["kind"]
    got = (bool(r["accepted"]),) + tuple(int(x) for x in r["info"][5:10])
    d_pose = max(np.abs(r["R"] - o["R"]).max(), np.abs(r["t"] - o["t"]).max()) if np.isfinite(o["R"]).all() else 0.0
    d_info = [S.rel_diff(r["info"][i], o["info"][i]) for i in S.INFO_COMPARED[kind]]
    d_mu = S.rel_diff(r["mu"], o["mu"])
    with np.errstate(invalid="ignore"):
        d_q = np.nanmax(np.abs(r["Q"] - o["Q"]))
    print(name, "integers", got, "dpose %.3g (%.3g) dQ %.3g (%.3g)" % (d_pose, tol["pose"], d_q, tol["q"]), "info", d_info, "(%.3g)" % tol["info"],
          "mu %.3g (%.3g)" % (d_mu, tol["mu"]))
    assert got == S.integers(o), name
    if kind == "accepted":
        assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all() and np.isfinite(r["Q"]).all(), name
        assert d_pose <= tol["pose"] and d_q <= tol["q"], name
        assert not np.array_equal(r["Q"], s["Q"]) or int(o["info"][5]) == 0, name
    else:
        assert r["R"].tobytes() == s["R"].tobytes() and r["t"].tobytes() == s["t"].tobytes() and r["Q"].tobytes() == s["Q"].tobytes(), name
    assert max(d_info) <= tol["info"] and d_mu <= tol["mu"], name
    if s["mask"] is not None:
        out = s["mask"] == 0
        assert out.any() and r["Q"][out].tobytes() == s["Q"][out].tobytes(), "rows outside the mask are untouched"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(S.BRANCH_SCENES))
def test_scene_host_and_device(ctx, name):
    import torch
    from matchinglib_poselib_amd import pose

    s = S.scene(name)
    r = _gpu_single(ctx, name)
    _hold(r, name)
    d1, d2, dq = torch.from_numpy(s["p1"]).cuda(), torch.from_numpy(s["p2"]).cuda(), torch.from_numpy(s["Q"].copy()).cuda()
    dm = None if s["mask"] is None else torch.from_numpy(s["mask"].copy()).cuda()
    d = pose.refine_stereo_ba_device(d1, d2, s["R"], s["t"], dq, s["th"], dm, s["angle_thresh"], s["t_norm_thresh"], ctx=ctx)
    torch.cuda.synchronize()
    assert d["accepted"] == r["accepted"] and d["R"].tobytes() == r["R"].tobytes() and d["t"].tobytes() == r["t"].tobytes()
    assert d["info"].tobytes() == r["info"].tobytes() and np.array([d["mu"]]).tobytes() == np.array([r["mu"]]).tobytes()
    assert dq.cpu().numpy().tobytes() == r["Q"].tobytes()
    if dm is not None:
        assert dm.cpu().numpy().tobytes() == s["mask"].tobytes()


@pytest.mark.gpu
def test_refusal_boundary(ctx):
    """11 valid points: 44 measurements, 45 unknowns -- nothing is touched and info stays zero; 12: the optimiser runs.  With and without a mask."""
    for few, enough, rows in (("n11", "n12", None), ("n11_of_40", "n12_of_40", 40)):
        s, r = S.scene(few), _gpu_single(ctx, few)
        assert (s["p1"].shape[0], s["mask"] is None) == (11, True) if rows is None else (s["p1"].shape[0], np.count_nonzero(s["mask"])) == (40, 11)
        assert not r["accepted"] and not r["info"].any() and r["mu"] == 0.0
        assert r["R"].tobytes() == s["R"].tobytes() and r["t"].tobytes() == s["t"].tobytes() and r["Q"].tobytes() == s["Q"].tobytes()
        s, r = S.scene(enough), _gpu_single(ctx, enough)
        assert (s["p1"].shape[0], s["mask"] is None) == (12, True) if rows is None else (s["p1"].shape[0], np.count_nonzero(s["mask"])) == (40, 12)
        valid = slice(None) if s["mask"] is None else s["mask"] != 0
        assert r["accepted"] and r["info"][5] > 0 and r["info"][8] == r["info"][5] and not np.array_equal(r["Q"][valid], s["Q"][valid])


# every scene in one launch; a 150-iteration problem, an empty one, an 11-point one and a 0-iteration one sit side by side
BATCH = [k for k in S.BRANCH_SCENES if k not in ("stop3_n12", "n11", "stop1_at_truth")] + ["stop3_n12", None, "n11", "stop1_at_truth"]
BATCH = BATCH[-4:] + BATCH[:-4]


@pytest.mark.gpu
def test_ragged_batch_equals_single(ctx):
    """One thresholds pair per call, so every problem is held to its single run AT THE BATCH'S thresholds (three scenes carry their own).  A
    workgroup that left state behind for its neighbour, or a short problem that read a long one's workspace, would differ from its single
    run."""
    import torch
    from matchinglib_poselib_amd import pose

    stride, B = 600, len(BATCH)
    assert stride > max(S.scene(k)["p1"].shape[0] for k in S.BRANCH_SCENES) == 513
    assert [int(S.oracle_result(k)["info"][5]) if k else None for k in BATCH[:4]] == [150, None, 0, 0]
    rng = np.random.default_rng(99)
    P1, P2 = rng.uniform(-1, 1, (B, stride, 2)), rng.uniform(-1, 1, (B, stride, 2))             # garbage beyond counts[b]
    Q0, M = rng.uniform(-50, 50, (B, stride, 3)), rng.integers(0, 256, (B, stride)).astype(np.uint8)
    Q0[:, -1] = np.nan
    R, t, th, counts = np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros(B), np.zeros(B, np.int32)
    for b, name in enumerate(BATCH):
        s = S.scene(name or "n12")
        n = 0 if name is None else s["p1"].shape[0]
        counts[b], R[b], t[b], th[b] = n, s["R"], s["t"], s["th"]
        P1[b, :n], P2[b, :n], Q0[b, :n] = s["p1"][:n], s["p2"][:n], s["Q"][:n]
        M[b, :n] = 1 if s["mask"] is None else s["mask"][:n]
    assert sum(1 for k in BATCH if k and S.scene(k)["mask"] is not None) >= 2
    d1, d2, dm = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda(), torch.from_numpy(M.copy()).cuda()
    runs = []
    for _ in range(2):
        dq = torch.from_numpy(Q0.copy()).cuda()
        res = pose.refine_stereo_ba_batch(d1, d2, counts, R, t, dq, th, dm, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
        torch.cuda.synchronize()
        runs.append((res, dq.cpu().numpy()))
    (res, Qb), (res2, Qb2) = runs
    for k in ("accepted", "R", "t", "info", "mu"):
        assert res[k].tobytes() == res2[k].tobytes(), k                          # two identical calls give identical bits
    assert Qb.tobytes() == Qb2.tobytes() and dm.cpu().numpy().tobytes() == M.tobytes()
    for b, name in enumerate(BATCH):
        n = counts[b]
        assert Qb[b, n:].tobytes() == Q0[b, n:].tobytes(), "points beyond counts[b] are untouched"
        if name is None:
            assert not res["accepted"][b] and not res["info"][b].any() and res["mu"][b] == 0.0
            assert res["R"][b].tobytes() == R[b].tobytes() and res["t"][b].tobytes() == t[b].tobytes()
            continue
        r, s = _gpu_single(ctx, name, own_thresholds=False), S.scene(name)
        assert bool(res["accepted"][b]) == r["accepted"] and res["R"][b].tobytes() == r["R"].tobytes() and res["t"][b].tobytes() == r["t"].tobytes(), name
        assert res["info"][b].tobytes() == r["info"].tobytes() and res["mu"][b:b + 1].tobytes() == np.array([r["mu"]]).tobytes(), name
        assert Qb[b, :n].tobytes() == r["Q"].tobytes(), name
        if s["mask"] is not None:
            out = s["mask"] == 0
            assert Qb[b, :n][out].tobytes() == s["Q"][out].tobytes(), name
    # the verdicts are the oracle's wherever the batch's thresholds are the scene's own
    for b, name in enumerate(BATCH):
        if name and (S.scene(name)["angle_thresh"], S.scene(name)["t_norm_thresh"]) == (S.ANGLE_THRESH, S.T_NORM_THRESH):
            assert bool(res["accepted"][b]) == S.oracle_result(name)["accepted"], name
