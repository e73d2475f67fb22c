"""Pose recovery on the MI355X (mlpl_recover_pose, its translation, device and batch forms through pose.getPoseTriangPts,
pose.getPoseTriangPts_device and pose.recover_pose_batch) against the restatement of recover_pose_oracle.py on the cases of
recover_pose_scenes.py: ten motions, so that each of the four candidates wins somewhere, E / -E / 2.5 E, dist 50 and 9, coincident rows, five
kinds of incoming mask, sizes either side of a wave, of a wave's 256-point share and of a workgroup's 1024, and the ties of the selection
chain.  test_oracle_recover_pose.py shows on the CPU that every case is decidable (no compared quantity within 1e-9 of its threshold, a
strict winner outside the ties), so counts and mask bytes are compared exactly; R and t to 1e-12 (the bar of test_gpu_pose.py) and the
points to rtol = atol = 1e-9 on the rows where the oracle's point is finite and below 1e6."""
import numpy as np
import pytest

import recover_pose_oracle as RPO
import recover_pose_scenes as S

pytestmark = pytest.mark.gpu

CASES = [(name, n) for name in S.MOTIONS for n in S.sizes(name)]
PAD = 64           # rows behind the n a device entry is given: they keep their sentinel


def _check_pose(R, t, o, what):
    assert np.abs(R - o["R"]).max() < 1e-12 and np.abs(np.ravel(t) - o["t"]).max() < 1e-12, what


def _check_host(res, o, m, what):
    good, R, t, Q, mo = res
    assert good == o["n_good"], (what, good, o["n_good"], o["counts"])
    _check_pose(R, t, o, what)
    if m is None:
        assert mo is None
    else:
        assert mo.tobytes() == o["mask"].tobytes(), what
    rows = S.comparable(o["Q"])
    assert Q.shape == o["Q"].shape and np.allclose(Q[rows], o["Q"][rows], rtol=1e-9, atol=1e-9), what


def _device(pose, ctx, E, d1, d2, m, dist, with_q):
    """-> good, R, t, mask bytes or None, Q or None; the rows behind n must keep their sentinel."""
    import torch

    n = d1.shape[0]
    dm = dq = None
    if m is not None:
        dm = torch.full((n + PAD,), S.SENTINEL, dtype=torch.uint8, device="cuda")
        dm[:n] = torch.from_numpy(m.copy()).cuda()
    if with_q:
        dq = torch.full((n + PAD, 3), -7.0, dtype=torch.float64, device="cuda")
    good, R, t = pose.getPoseTriangPts_device(E, d1, d2, None if dm is None else dm[:n], dist, Q_out=None if dq is None else dq[:n], ctx=ctx)
    torch.cuda.synchronize()
    mo = Q = None
    if dm is not None:
        h = dm.cpu().numpy()
        assert np.all(h[n:] == S.SENTINEL), "mask bytes behind n"
        mo = h[:n]
    if dq is not None:
        h = dq.cpu().numpy()
        assert np.all(h[n:] == -7.0), "points behind n"
        Q = h[:n]
    return good, R, t, mo, Q


def _check_device_equals_host(dev, host, what):
    good, R, t, mo, Q = dev
    hg, hR, ht, hQ, hm = host
    assert good == hg and R.tobytes() == hR.tobytes() and t.tobytes() == ht.tobytes(), what
    if mo is not None:
        assert mo.tobytes() == hm.tobytes(), what
    if Q is not None:
        assert Q.tobytes() == hQ.tobytes(), what


@pytest.mark.parametrize("name,n", CASES)
def test_host_and_device_entries(ctx, oracle, name, n):
    import torch
    from matchinglib_poselib_amd import pose

    for variant in S.variants(name, n):
        scale, dist, coincident = variant
        p1, p2 = S.scene(name, n, coincident)
        d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
        E = S.E_of(name, scale)
        for kind in S.MASKS:
            what = (variant, kind)
            o, m = S.expected(oracle, name, n, variant, kind), S.mask(n, kind)
            host = pose.getPoseTriangPts(E, p1, p2, m, dist, ctx=ctx)
            _check_host(host, o, m, what)
            if kind == "zero" or n == 0:
                assert host[0] == 0 and (m is None or not host[4].any())
            for with_q in (True, False):
                _check_device_equals_host(_device(pose, ctx, E, d1, d2, m, dist, with_q), host, what + (with_q,))


@pytest.mark.parametrize("tie", S.TIES, ids=str)
def test_ties_host_and_device(ctx, oracle, tie):
    """Two (or all four) candidates with the same count: the first of them in the chain's order wins; only the last one nonzero: the tail."""
    import torch
    from matchinglib_poselib_amd import pose

    p1, p2 = S.scene("forward", S.TIE_N)
    E = S.E_of("forward", "pos")
    cand = S.cand(oracle, "forward", S.TIE_N, "pos")
    m, k = S.tie_mask(oracle, tie)
    o = RPO.decide(cand, m, 50.0)
    pick = S.tie_expected_pick(tie)
    assert o["pick"] == pick and o["n_good"] == k
    host = pose.getPoseTriangPts(E, p1, p2, m, 50.0, ctx=ctx)
    _check_host(host, o, m, tie)
    for c in range(4):   # the pick is told by R and t: no other candidate is near
        near = np.abs(host[1] - cand["R"][c]).max() < 1e-12 and np.abs(host[2].ravel() - cand["t"][c]).max() < 1e-12
        assert near == (c == pick), (tie, c)
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    for with_q in (True, False):
        _check_device_equals_host(_device(pose, ctx, E, d1, d2, m, 50.0, with_q), host, (tie, with_q))


def _run_batch(pose, ctx, problems, stride, dist=50.0):
    """problems: (p1, p2, E, mask or None) each, all with a mask or none -> the batch entry's result and the masks [B, stride] (or None)."""
    import torch

    B = len(problems)
    P1, P2 = np.zeros((B, stride, 2)), np.zeros((B, stride, 2))
    M = np.full((B, stride), S.SENTINEL, np.uint8)
    counts = np.array([q[0].shape[0] for q in problems], np.int32)
    for b, (p1, p2, E, m) in enumerate(problems):
        P1[b, :counts[b]], P2[b, :counts[b]] = p1, p2
        if m is not None:
            M[b, :counts[b]] = m
    with_masks = problems[0][3] is not None
    d1, d2 = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda()
    dm = torch.from_numpy(M.copy()).cuda() if with_masks else None
    res = pose.recover_pose_batch(d1, d2, counts, np.stack([q[2] for q in problems]), dm, dist, ctx=ctx)
    torch.cuda.synchronize()
    return res, (dm.cpu().numpy() if with_masks else None)


def _check_batch(pose, ctx, problems, expected, res, masks, dist=50.0):
    import torch

    for b, ((p1, p2, E, m), o) in enumerate(zip(problems, expected)):
        n = p1.shape[0]
        # the restatement
        assert res["n_good"][b] == o["n_good"], (b, res["n_good"][b], o["counts"])
        _check_pose(res["R"][b], res["t"][b], o, b)
        # the single device entry
        good, R, t, mo, _ = _device(pose, ctx, E, torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), m, dist, False)
        assert res["n_good"][b] == good and res["R"][b].tobytes() == R.tobytes() and res["t"][b].tobytes() == t.tobytes(), b
        if m is not None:
            assert masks[b, :n].tobytes() == o["mask"].tobytes() == mo.tobytes(), b
            assert np.all(masks[b, n:] == S.SENTINEL), b


def test_ties_in_one_batch(ctx, oracle):
    from matchinglib_poselib_amd import pose

    p1, p2 = S.scene("forward", S.TIE_N)
    E = S.E_of("forward", "pos")
    cand = S.cand(oracle, "forward", S.TIE_N, "pos")
    problems = [(p1, p2, E, S.tie_mask(oracle, tie)[0]) for tie in S.TIES]
    expected = [RPO.decide(cand, q[3], 50.0) for q in problems]
    assert [o["pick"] for o in expected] == [S.tie_expected_pick(tie) for tie in S.TIES]
    res, masks = _run_batch(pose, ctx, problems, S.TIE_N + 7)
    _check_batch(pose, ctx, problems, expected, res, masks)


@pytest.mark.parametrize("kind", S.BATCH_MASKS)
def test_batch_of_eight(ctx, oracle, kind):
    """Counts either side of every boundary in one launch, each problem another motion or sign, every pick among them."""
    from matchinglib_poselib_amd import pose

    problems, expected = [], []
    for n, (name, scale) in zip(S.BATCH_COUNTS, S.BATCH_MOTIONS):
        problems.append(S.scene(name, n) + (S.E_of(name, scale), S.mask(n, kind)))
        expected.append(S.expected(oracle, name, n, (scale, 50.0, False), kind))
    assert {o["pick"] for o in expected if max(o["counts"]) > 0} == {0, 1, 2, 3}
    res, masks = _run_batch(pose, ctx, problems, S.BATCH_STRIDE)
    assert (masks is None) == (kind == "none")
    _check_batch(pose, ctx, problems, expected, res, masks)
    assert res["n_good"][0] == 0


@pytest.mark.parametrize("n", S.TRANS_SIZES)
def test_translation_only(ctx, oracle, n):
    """translatE: [I|t] and [I|-t] alone; R is exactly I."""
    from matchinglib_poselib_amd import pose

    p1, p2 = S.scene("norot", n)
    cases = [(scale, kind, dist, S.mask(n, kind)) for scale in S.TRANS_PICKS for kind in ("none", "half", "ones") for dist in (50.0, 9.0)]
    if n == S.TIE_N:
        cases.append(("pos", "tie", 50.0, S.tie_mask(oracle, (0, 2), "norot", translation=True)[0]))
    for scale, kind, dist, m in cases:
        o = RPO.decide(S.cand(oracle, "norot", n, scale, translation=True), m, dist)
        if kind == "none" and dist == 50.0:
            assert o["pick"] == S.TRANS_PICKS[scale]
        if kind == "tie":
            assert o["pick"] == 0 and o["counts"][0] == o["counts"][2] > 0
        host = pose.getPoseTriangPts(S.E_of("norot", scale), p1, p2, m, dist, translatE=True, ctx=ctx)
        _check_host(host, o, m, (scale, kind, dist))
        assert np.array_equal(host[1], np.eye(3)) and np.abs(host[2].ravel() - o["t"]).max() < 1e-12
