"""refineEssentialLinear on the MI355X (mlpl_refine_essential_linear, its batch form, mlpl_recover_pose_batch_dev and the C++ drop-in) against
the float64 restatement in linear_refine_oracle.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import linear_refine_oracle as LRO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "linear_refine_facade")
METHODS = [s | w for s in (0x1, 0x2, 0x3) for w in (0x10, 0x20, 0x30)]
SCENES = [(200, 0.9), (500, 0.3), (1000, 0.6), (2000, 0.5), (3000, 0.8), (4096, 0.5), (6000, 0.4), (8192, 0.7)]


def _scene(oracle, seed, n, frac):
    from matchinglib_poselib_amd import synth

    p1, p2, _, _, _, th = synth.pose_scene(n, frac, seed=1000 + seed, noise_px=0.3)
    r = oracle.ransac_essential(p1, p2, th, seed=seed + 1)
    assert r["ok"]
    return p1, p2, r["E"], r["mask"], th


@pytest.fixture(scope="module")
def scenes(oracle):
    return [_scene(oracle, k, n, f) for k, (n, f) in enumerate(SCENES)]


def _close_up_to_sign(A, B, tol):
    a = np.asarray(A).reshape(9) / np.linalg.norm(A)
    b = np.asarray(B).reshape(9) / np.linalg.norm(B)
    return min(np.abs(a - b).max(), np.abs(a + b).max()) <= tol


def _single(ctx, p1, p2, E, mask, method, th, **kw):
    from matchinglib_poselib_amd import pose

    return pose.refine_essential_linear(p1, p2, E, mask, method, th=th, ctx=ctx, **kw)


def _check_vs_oracle(g, o, E0, mask0):
    assert g["ok"] == (o["rc"] == 0)
    if not g["ok"]:
        assert g["E"].tobytes() == np.asarray(E0, np.float64).reshape(3, 3).tobytes()
        return
    assert g["steps_done"] == o["steps_done"] and g["n_inliers"] == o["n_inliers"]
    assert g["mask"].tobytes() == o["mask"].tobytes()
    assert _close_up_to_sign(g["E"], o["E"], 1e-8)


@pytest.mark.parametrize("method", METHODS)
def test_methods_match_restatement(ctx, scenes, method):
    refined = 0
    for p1, p2, E0, m0, th in scenes:
        o = LRO.refine_essential_linear(p1, p2, E0, m0, method, th=th)
        assert o["margin"] > 1e-9, "an error lies on a step threshold: pick another seed"
        g = _single(ctx, p1, p2, E0, m0, method, th)
        _check_vs_oracle(g, o, E0, m0)
        refined += g["ok"] and g["steps_done"] > 0
    assert refined >= len(scenes) - 1


def _ragged_batch(oracle, B=64, stride=3000):
    rng = np.random.default_rng(7)
    P1, P2, E, M, counts, th = np.zeros((B, stride, 2)), np.zeros((B, stride, 2)), np.zeros((B, 9)), np.zeros((B, stride), np.uint8), [], []
    from matchinglib_poselib_amd import synth

    for b in range(B):
        n = int(rng.integers(200, stride + 1))
        p1, p2, _, _, _, t = synth.pose_scene(n, float(rng.uniform(0.3, 0.9)), seed=5000 + b, noise_px=0.3)
        r = oracle.ransac_essential(p1, p2, t, seed=b + 11)
        m = r["mask"].copy()
        if b % 8 == 3:      # fewer than 6 inliers: rejected
            m[:] = 0
            m[:5] = 1
        elif b % 8 == 5:    # every point flagged: the first step loses too many
            m[:] = 1
        P1[b, :n], P2[b, :n], E[b], M[b, :n] = p1, p2, r["E"].reshape(9), m
        counts.append(n)
        th.append(t)
    return P1, P2, E, M, np.array(counts, np.int32), np.array(th)


@pytest.mark.parametrize("steps", [4, 0])
def test_batch_equals_single(ctx, oracle, steps):
    import torch
    from matchinglib_poselib_amd import pose

    P1, P2, E, M, counts, th = _ragged_batch(oracle)
    B = len(counts)
    d1, d2 = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda()
    dm = torch.from_numpy(M).cuda()
    res = pose.refine_essential_linear_batch(d1, d2, counts, E, dm, th, 0x21, num_iterative_steps=steps, ctx=ctx)
    torch.cuda.synchronize()
    masks = dm.cpu().numpy()
    kinds = set()
    for b in range(B):
        n = counts[b]
        g = _single(ctx, P1[b, :n], P2[b, :n], E[b], M[b, :n], 0x21, th[b], num_iterative_steps=steps)
        assert (res["status"][b] == 0) == g["ok"]
        assert res["E"][b].tobytes() == g["E"].tobytes()
        assert masks[b, :n].tobytes() == g["mask"].tobytes()
        assert res["n_inliers"][b] == g["n_inliers"] and res["steps_done"][b] == g["steps_done"]
        assert masks[b, n:].tobytes() == M[b, n:].tobytes()
        if not g["ok"]:
            assert res["E"][b].reshape(9).tobytes() == E[b].tobytes() and masks[b, :n].tobytes() == M[b, :n].tobytes()
        kinds.add("rejected" if not g["ok"] else ("refined" if g["steps_done"] else "unchanged"))
    assert kinds == ({"rejected", "refined"} if steps else {"rejected", "unchanged"})


def test_edge_cases(ctx, scenes):
    from matchinglib_poselib_amd import pose
    from matchinglib_poselib_amd._lib import MlplError

    p1, p2, E0, m0, th = scenes[3]
    few = np.zeros_like(m0)
    few[np.flatnonzero(m0)[:5]] = 1
    g = _single(ctx, p1, p2, E0, few, 0x21, th)
    assert not g["ok"] and g["mask"].tobytes() == few.tobytes()
    allm = np.ones_like(m0)
    o = LRO.refine_essential_linear(p1, p2, E0, allm, 0x21, th=th)
    g = _single(ctx, p1, p2, E0, allm, 0x21, th)
    assert o["rc"] == LRO.MLPL_E_FAILED and not g["ok"] and g["mask"].tobytes() == allm.tobytes()
    m7 = (m0 * 7).astype(np.uint8)  # nonzero = inlier; out: 0 / 1
    for method, kw in [(0x21, dict(num_iterative_steps=0)), (0x00, {}), (0x20, {}), (0x05, {}), (0x3F, {})]:
        g = _single(ctx, p1, p2, E0, m7, method, th, **kw)
        assert g["ok"] and g["steps_done"] == 0 and g["E"].tobytes() == E0.tobytes()
        assert g["mask"].tobytes() == (m0 != 0).astype(np.uint8).tobytes() and g["n_inliers"] == int(np.count_nonzero(m0))
    for method, rc in [(0x04, -2), (0x24, -2), (0x01, -1), (0x41, -1)]:
        with pytest.raises(MlplError) as ei:
            _single(ctx, p1, p2, E0, m0, method, th)
        assert ei.value.code == rc
    for solver in (0x2, 0x3):
        ref = _single(ctx, p1, p2, E0, m0, solver | 0x30, th)
        for w in (0x00, 0x40):
            g = _single(ctx, p1, p2, E0, m0, solver | w, th)
            assert g["E"].tobytes() == ref["E"].tobytes() and g["mask"].tobytes() == ref["mask"].tobytes()


def test_large_problem(ctx, oracle):
    from matchinglib_poselib_amd import synth

    p1, p2, _, _, _, th = synth.pose_scene(65536, 0.5, seed=77, noise_px=0.3)
    r = oracle.ransac_essential(p1, p2, th, seed=3)
    for method in (0x21, 0x23):
        o = LRO.refine_essential_linear(p1, p2, r["E"], r["mask"], method, th=th)
        assert o["margin"] > 1e-9
        _check_vs_oracle(_single(ctx, p1, p2, r["E"], r["mask"], method, th), o, r["E"], r["mask"])


def test_harness_chain(ctx, oracle):
    """estimate -> refine 0x21 -> cheirality at batch speed == the same chain of single entries == the CPU chain."""
    import torch
    from matchinglib_poselib_amd import batch, pose

    B, stride = 64, 2048
    rng = np.random.default_rng(11)
    P1, P2, counts = np.zeros((B, stride, 2)), np.zeros((B, stride, 2)), []
    from matchinglib_poselib_amd import synth

    th = None
    for b in range(B):
        n = int(rng.integers(300, stride + 1))
        p1, p2, _, _, _, th = synth.pose_scene(n, float(rng.uniform(0.4, 0.9)), seed=9000 + b, noise_px=0.3)
        P1[b, :n], P2[b, :n] = p1, p2
        counts.append(n)
    counts = np.array(counts, np.int32)
    seeds = np.arange(B) + 100
    d1, d2 = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda()
    dm = torch.zeros((B, stride), dtype=torch.uint8, device="cuda")
    rs = batch.ransac_pose_batched(ctx, d1, d2, counts, seeds, th, recover_pose=False, masks_out=dm)
    E = np.stack([r["E"].reshape(9) for r in rs])
    ref = pose.refine_essential_linear_batch(d1, d2, counts, E, dm, th, 0x21, ctx=ctx)
    pb = pose.recover_pose_batch(d1, d2, counts, ref["E"], dm, ctx=ctx)
    torch.cuda.synchronize()
    masks = dm.cpu().numpy()
    for b in range(B):
        n = counts[b]
        assert rs[b]["status"] == 0
        # the same chain through the single-problem entries
        s = pose.ransac_essential_device(d1[b, :n].contiguous(), d2[b, :n].contiguous(), th, refit=False, seed=int(seeds[b]), ctx=ctx)
        m_single = s["mask"].cpu().numpy()
        g = _single(ctx, P1[b, :n], P2[b, :n], s["E"], m_single, 0x21, th)
        assert g["ok"] and ref["status"][b] == 0
        assert ref["E"][b].tobytes() == g["E"].tobytes()
        dmask = torch.from_numpy(g["mask"].copy()).cuda()
        good, R, t = pose.getPoseTriangPts_device(g["E"], d1[b, :n].contiguous(), d2[b, :n].contiguous(), mask=dmask, ctx=ctx)
        assert pb["n_good"][b] == good and pb["R"][b].tobytes() == R.tobytes() and pb["t"][b].tobytes() == t.reshape(3).tobytes()
        assert masks[b, :n].tobytes() == dmask.cpu().numpy().tobytes()
        # the CPU chain
        r = oracle.ransac_essential(P1[b, :n], P2[b, :n], th, seed=int(seeds[b]))
        o = LRO.refine_essential_linear(P1[b, :n], P2[b, :n], r["E"], r["mask"], 0x21, th=th)
        assert o["rc"] == 0 and o["mask"].tobytes() == g["mask"].tobytes()
        assert _close_up_to_sign(o["E"], g["E"], 1e-8)
        og, oR, ot, _, _ = oracle.recover_pose(o["E"], P1[b, :n], P2[b, :n], mask=o["mask"])
        assert og == good
        assert np.abs(oR - R).max() <= 1e-6 and np.abs(ot.reshape(3) - t.reshape(3)).max() <= 1e-6


def test_facade(ctx, scenes, tmp_path):
    assert os.path.exists(FACADE_EXE), "built by the facade Makefile's check target"
    p1, p2, E0, m0, th = scenes[2]
    n = p1.shape[0]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<id", n, th) + p1.tobytes() + p2.tobytes() + np.asarray(E0, np.float64).tobytes() + m0.astype(np.uint8).tobytes())
    subprocess.run([FACADE_EXE, str(src), str(dst)], check=True, timeout=120)
    raw = dst.read_bytes()
    at = 0
    for method in (0x21, 0x23):
        g = _single(ctx, p1, p2, E0, m0, method, th)
        ok, nr = struct.unpack_from("<iq", raw, at)
        at += 12
        E = np.frombuffer(raw, np.float64, 9, at)
        at += 72
        mask = np.frombuffer(raw, np.uint8, n, at)
        at += n
        assert bool(ok) == g["ok"] and nr == g["n_inliers"]
        assert E.tobytes() == g["E"].tobytes() and mask.tobytes() == g["mask"].tobytes()
    flags = struct.unpack_from("<4i", raw, at)
    assert flags == (1, 1, 1, 1), "R cleared, t untouched, Kneip returns false and leaves E / mask alone"
