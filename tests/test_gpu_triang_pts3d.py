"""poselib::triangPts3D on the MI355X (mlpl_triang_pts3d, its device and batch forms, the Python surfaces and the C++ drop-in) against the
CPU restatement in triang_pts3d_oracle.py.  Counts and mask bytes are compared exactly -- the scenes keep every compared quantity away from
its threshold (`margin`, checked here on the CPU) -- and the points to rtol = atol = 1e-9 on the rows where the oracle's point is finite
and below 1e6, the bar of test_gpu_pose.py; at most 5 % of a case's rows may be excluded that way."""
import os
import struct
import subprocess

import numpy as np
import pytest

import kneip_refine_oracle as KRO
import triang_pts3d_oracle as TPO
from matchinglib_poselib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "triang_pts3d_facade")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)   # one wave not full / full / one over; a wave's 256-point share likewise; a second workgroup (1024 points each) is the batch test's business below -- 1000 walks all four waves
VARIANTS = ("true", "neg_t", "dist9", "infinity")
MASKS = ("none", "half", "zero", "ones")
MARGIN = 1e-9
SEED = 20261019

_cases, _oracle = {}, {}


def _case(n, variant):
    """-> p1, p2, R, t, dist"""
    if (n, variant) not in _cases:
        p1, p2, R, t, _, _ = synth.pose_scene(n, 0.8, seed=SEED + n)
        p2, dist = p2.copy(), 50.0
        if variant == "neg_t":
            t = -t                      # nearly every point lands behind a camera
        elif variant == "dist9":
            dist = 9.0                  # the scene is 4 .. 12 deep
        elif variant == "infinity":
            k = int(round(0.02 * n))    # the same image point in both views
            idx = np.random.default_rng(n).permutation(n)[:k]
            p2[idx] = p1[idx]
        _cases[(n, variant)] = (p1, p2, R, t, dist)
    return _cases[(n, variant)]


def _mask(n, kind):
    rng = np.random.default_rng(n + 7)
    if kind == "none":
        return None
    if kind == "half":
        return (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(2, 256, n).astype(np.uint8)   # any nonzero byte counts
    if kind == "zero":
        return np.zeros(n, np.uint8)
    return np.ones(n, np.uint8)        # 0 / 1 as StereoRefine holds it: 1 & 255 stays 1


def _ora(oracle, n, variant, kind):
    if (n, variant, kind) not in _oracle:
        p1, p2, R, t, dist = _case(n, variant)
        _oracle[(n, variant, kind)] = TPO.triang_pts3d(oracle, R, t, p1, p2, _mask(n, kind), dist)
    return _oracle[(n, variant, kind)]


def _comparable(Q):
    return np.all(np.isfinite(Q), axis=1) & (np.abs(Q).max(axis=1) < 1e6)


def _check_points(Q, o):
    rows = _comparable(o["Q"])
    assert np.allclose(Q[rows], o["Q"][rows], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", SIZES)
def test_oracle_cases_are_decidable(oracle, n, variant):
    """CPU only: no compared quantity within 1e-9 of its threshold, at most 5 % of the rows outside the point comparison, and the
    variants do what they are for."""
    o = _ora(oracle, n, variant, "none")
    assert o["margin"] > MARGIN, "pick another seed"
    assert np.count_nonzero(~_comparable(o["Q"])) <= 0.05 * n, "pick another seed"
    assert o["n_good"] == np.count_nonzero(o["mask"]) and set(np.unique(o["mask"])) <= {0, 255}
    base = _ora(oracle, n, "true", "none")
    if variant == "true":
        assert o["n_good"] >= 0.75 * n
    elif variant == "neg_t":
        assert o["n_good"] <= 0.1 * n
    elif variant == "dist9" and n >= 63:
        assert o["n_good"] < base["n_good"]
    elif variant == "infinity" and n >= 63:
        assert o["n_good"] <= base["n_good"] and not np.array_equal(o["Q"], base["Q"])
    ones = _ora(oracle, n, variant, "ones")
    assert set(np.unique(ones["mask"])) <= {0, 1} and ones["n_good"] == o["n_good"]
    assert _ora(oracle, n, variant, "zero")["n_good"] == 0
    half = _ora(oracle, n, variant, "half")
    assert np.array_equal(half["mask"], _mask(n, "half") & o["mask"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", SIZES)
def test_single_host_and_device(ctx, oracle, n, variant):
    import torch
    from matchinglib_poselib_amd import pose

    p1, p2, R, t, dist = _case(n, variant)
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    for kind in MASKS:
        o, m = _ora(oracle, n, variant, kind), _mask(n, kind)
        good, Q, mo = pose.triangPts3D(R, t, p1, p2, m, dist, ctx=ctx)
        assert good == o["n_good"], (kind, good, o["n_good"])
        if m is None:
            assert mo is None
        else:
            assert mo.tobytes() == o["mask"].tobytes(), kind
        _check_points(Q, o)
        # device entry: with the points, and without them (masked-out points are then not triangulated at all)
        for with_q in (True, False):
            dm = None if m is None else torch.from_numpy(m.copy()).cuda()
            dq = torch.full((n, 3), -7.0, dtype=torch.float64, device="cuda") if with_q else None
            gd = pose.triangPts3D_device(R, t, d1, d2, dm, dist, Q_out=dq, ctx=ctx)
            torch.cuda.synchronize()
            assert gd == good
            if dm is not None:
                assert dm.cpu().numpy().tobytes() == mo.tobytes()
            if with_q:
                assert dq.cpu().numpy().tobytes() == Q.tobytes(), "host and device entries run the same kernel"


def _batch_problems():
    counts = (0, 1, 64, 257, 300)
    probs = []
    for b, n in enumerate(counts):
        p1, p2, R, t, _, _ = synth.pose_scene(max(n, 1), 0.8, seed=SEED + 100 + b)
        if b == 2:
            t = -t
        if b == 3:
            R = synth._rot((0.3, 0.1, 0.9), 2.0) @ R
        m = (np.random.default_rng(b).random(max(n, 1)) < 0.6).astype(np.uint8)
        probs.append(dict(n=n, p1=p1[:n], p2=p2[:n], R=R, t=t, m=m[:n]))
    return counts, probs


@pytest.mark.gpu
@pytest.mark.parametrize("with_masks", (True, False), ids=("masks", "all_points"))
@pytest.mark.parametrize("with_q", (True, False), ids=("points", "no_points"))
def test_batch_equals_single(ctx, with_q, with_masks):
    import torch
    from matchinglib_poselib_amd import pose

    stride, dist = 300, 9.0
    counts, probs = _batch_problems()
    B = len(probs)
    P1, P2, M = np.zeros((B, stride, 2)), np.zeros((B, stride, 2)), np.full((B, stride), 5, np.uint8)
    Q0 = np.full((B, stride, 3), -7.0)
    for b, q in enumerate(probs):
        P1[b, :q["n"]], P2[b, :q["n"]], M[b, :q["n"]] = q["p1"], q["p2"], q["m"]
    d1, d2 = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda()
    dm = torch.from_numpy(M.copy()).cuda() if with_masks else None
    dq = torch.from_numpy(Q0.copy()).cuda() if with_q else None
    good = pose.triang_pts3d_batch(d1, d2, counts, np.stack([q["R"] for q in probs]), np.stack([q["t"] for q in probs]), dm, dq, dist, ctx=ctx)
    torch.cuda.synchronize()
    masks = None if dm is None else dm.cpu().numpy()
    Qb = None if dq is None else dq.cpu().numpy()
    for b, q in enumerate(probs):
        n = q["n"]
        g, Q, mo = pose.triangPts3D(q["R"], q["t"], q["p1"], q["p2"], q["m"] if with_masks else None, dist, ctx=ctx)
        assert good[b] == g, b
        if with_masks:
            assert masks[b, :n].tobytes() == mo.tobytes() and masks[b, n:].tobytes() == M[b, n:].tobytes(), b
        if with_q:
            assert Qb[b, :n].tobytes() == Q.tobytes() and Qb[b, n:].tobytes() == Q0[b, n:].tobytes(), b
    assert good[0] == 0 and good[4] > 0


@pytest.mark.gpu
def test_chain_behind_the_kneip_refinement(ctx, oracle):
    """mlpl_refine_essential_linear_rt_batch_dev -> mlpl_triang_pts3d_batch_dev on 4 problems x 300 equals the two restatements in a row."""
    import torch
    from matchinglib_poselib_amd import pose

    stride, B = 300, 4
    scenes = [KRO.make_scene(n_list, seed=50 + b) for b, n_list in enumerate((100, 150, 200, 230))]
    P1, P2, M = np.zeros((B, stride, 2)), np.zeros((B, stride, 2)), np.full((B, stride), 5, np.uint8)
    for b, (p1, p2, E0, m0, Rt, th) in enumerate(scenes):
        n = p1.shape[0]
        assert n <= stride
        P1[b, :n], P2[b, :n], M[b, :n] = p1, p2, m0
    counts = np.array([s[0].shape[0] for s in scenes], np.int32)
    d1, d2, dm = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda(), torch.from_numpy(M.copy()).cuda()
    dq = torch.zeros((B, stride, 3), dtype=torch.float64, device="cuda")
    res = pose.refine_essential_linear_rt_batch(d1, d2, counts, np.stack([s[2].reshape(9) for s in scenes]), dm, [s[5] for s in scenes], 0x24,
                                                seeds=[7 + b for b in range(B)], ctx=ctx)
    assert np.all(res["status"] == 0) and np.all(res["rt_valid"] == 1)
    good = pose.triang_pts3d_batch(d1, d2, counts, res["R"], res["t"], dm, dq, 50.0, ctx=ctx)
    torch.cuda.synchronize()
    masks, Qb = dm.cpu().numpy(), dq.cpu().numpy()
    for b, (p1, p2, E0, m0, Rt, th) in enumerate(scenes):
        n = counts[b]
        o = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x24, R=None, th=th, seed=7 + b)
        assert o["rc"] == 0 and o["rt_valid"] and o["margin"] > 1e-6, "pick another scene"
        assert res["R"][b].tobytes() == o["R"].tobytes() and res["t"][b].tobytes() == o["t"].tobytes()
        ot = TPO.triang_pts3d(oracle, o["R"], o["t"], p1, p2, o["mask"], 50.0)
        assert ot["margin"] > MARGIN, "pick another scene"
        assert good[b] == ot["n_good"] and masks[b, :n].tobytes() == ot["mask"].tobytes() and masks[b, n:].tobytes() == M[b, n:].tobytes()
        assert set(np.unique(ot["mask"])) <= {0, 1} and ot["n_good"] >= 0.9 * o["n_inliers"]
        rows = _comparable(ot["Q"])
        assert rows.sum() >= 0.95 * n and np.allclose(Qb[b, :n][rows], ot["Q"][rows], rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
def test_facade(ctx, oracle, tmp_path):
    from matchinglib_poselib_amd import pose

    assert os.path.exists(FACADE_EXE), "built by the facade Makefile's check target"
    n = 257
    p1, p2, R, t, dist = _case(n, "dist9")
    m = _mask(n, "ones")
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<id", n, dist) + np.ascontiguousarray(R, np.float64).tobytes() + np.ascontiguousarray(t, np.float64).tobytes() +
                    p1.tobytes() + p2.tobytes() + m.tobytes())
    subprocess.run([FACADE_EXE, str(src), str(dst)], check=True, timeout=120)
    raw = dst.read_bytes()
    good, Q, mo = pose.triangPts3D(R, t, p1, p2, m, dist, ctx=ctx)
    o = _ora(oracle, n, "dist9", "ones")
    assert good == o["n_good"] and mo.tobytes() == o["mask"].tobytes()
    at = 0
    (ret,) = struct.unpack_from("<i", raw, at)
    at += 4
    assert ret == good and raw[at:at + 24 * n] == Q.tobytes() and raw[at + 24 * n:at + 25 * n] == mo.tobytes()   # the normal case
    at += 25 * n
    assert struct.unpack_from("<iii", raw, at) == (-1, 1, 1)    # an empty point set: -1, the mask untouched, no points
    at += 12
    (ret,) = struct.unpack_from("<i", raw, at)
    at += 4
    assert ret == -1 and raw[at:at + n] == mo.tobytes()         # Q3D not requested: the mask updated, then -1
    at += n
    (ret,) = struct.unpack_from("<i", raw, at)
    at += 4
    # no mask and the default distance (50): all points of the same scene
    assert ret == _ora(oracle, n, "true", "none")["n_good"] and raw[at:at + 24 * n] == Q.tobytes()
    assert at + 24 * n == len(raw)
