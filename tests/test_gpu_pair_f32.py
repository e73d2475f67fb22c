"""The pair entries on CV_32F descriptors -- mlpl_pair_pose_f32_dev, mlpl_pair_pose_batch_f32_dev, mlpl_pair_pose_batch_usac_f32_dev,
mlpl_pair_pose_batch_arrsac_f32_dev -- against the composition of the single-problem entries (mlpl_match_l2_dev ->
mlpl_gather_match_points_dev -> estimator -> mlpl_recover_pose_dev) bit for bit, and against the oracle pipeline (LINEAR float matching,
matchinglib/source/matchers.cpp:632-707 -> ImgToCamCoordTrans -> RANSAC / USAC / ARRSAC oracle -> recoverPose) at the project's bars.
Integer-valued SIFT-like rows (the int8 matrix-core path) and RootSIFT rows (the exact and fp16 paths)."""
import ctypes as C

import numpy as np
import pytest

from option_guard import options

pytestmark = pytest.mark.gpu

TH = lambda K: 0.8 * 4.0 / (np.sqrt(2.0) * (2 * K[0] + 2 * K[1]))  # noqa: E731   (stereo_pose_refinement.h:280-286)


def e_dist(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


def _cam(p, K):
    return np.stack([((p[:, 0].astype(np.float64) - K[2]) / K[0]).astype(np.float32),
                     ((p[:, 1].astype(np.float64) - K[3]) / K[1]).astype(np.float32)], axis=1).astype(np.float64)


def _pairs(B, nk, seed0, rootsift, unmatched=0.3):
    from matchinglib_poselib_amd import synth
    return [synth.stereo_pair_f32(nk, seed0 + i, unmatched_frac=unmatched + 0.02 * (i % 5), rootsift=rootsift) for i in range(B)]


def _stack(sps):
    import torch
    return [torch.from_numpy(np.stack([sp[k] for sp in sps])).cuda() for k in ("desc1", "desc2", "kp1", "kp2")]


def _single_raw(ctx, dq, dt, k1, k2, K, seed, refit=False, max_iters=1000):
    """mlpl_pair_pose_f32_dev's whole record."""
    import torch
    from matchinglib_poselib_amd import batch
    from matchinglib_poselib_amd._lib import check
    res = batch._PairResult()
    k4 = (C.c_double * 4)(*K)
    check(ctx.lib.mlpl_pair_pose_f32_dev(ctx.handle, dq.data_ptr(), dq.shape[0], dt.data_ptr(), dt.shape[0], dq.shape[1], k1.data_ptr(), k2.data_ptr(), k4, k4,
                                         float(TH(K)), int(max_iters), 0.999, 1 if refit else 0, int(seed), 50.0, C.addressof(res),
                                         torch.cuda.current_stream().cuda_stream), "mlpl_pair_pose_f32_dev")
    return np.frombuffer(bytes(res), batch._PAIR_RESULT_DTYPE, count=1)[0].copy()


def _batch_raw(ctx, stk, K, seeds, refit=False, matches_out=None):
    import torch
    from matchinglib_poselib_amd import batch
    from matchinglib_poselib_amd._lib import check
    B = stk[0].shape[0]
    res = (batch._PairResult * B)()
    k4 = (C.c_double * 4)(*K)
    sd = np.ascontiguousarray(seeds, np.uint32)
    check(ctx.lib.mlpl_pair_pose_batch_f32_dev(ctx.handle, B, stk[0].data_ptr(), stk[0].shape[1], stk[1].data_ptr(), stk[1].shape[1], stk[0].shape[2],
                                               stk[2].data_ptr(), stk[3].data_ptr(), k4, k4, float(TH(K)), 1000, 0.999, 1 if refit else 0, sd.ctypes.data, 50.0,
                                               C.addressof(res), matches_out.data_ptr() if matches_out is not None else None,
                                               torch.cuda.current_stream().cuda_stream), "mlpl_pair_pose_batch_f32_dev")
    return np.frombuffer(bytes(res), batch._PAIR_RESULT_DTYPE, count=B).copy()


def _match_and_gather(ctx, dq, dt, k1, k2, K):
    """mlpl_match_l2_dev + mlpl_gather_match_points_dev on one pair -> (count, matches [count, 4] int32 on the host, p1, p2 on the device)."""
    import torch
    from matchinglib_poselib_amd.matching import match_l2_device
    m = match_l2_device(dq, dt, ctx=ctx)
    cnt = int(m["count"][0].item())
    mm = m["matches"][0, :cnt].contiguous()
    d1 = torch.empty((max(cnt, 1), 2), dtype=torch.float64, device="cuda")[:cnt]
    d2 = torch.empty((max(cnt, 1), 2), dtype=torch.float64, device="cuda")[:cnt]
    k4 = (C.c_double * 4)(*K)
    if cnt:
        assert ctx.lib.mlpl_gather_match_points_dev(ctx.handle, mm.data_ptr(), cnt, k1.data_ptr(), k2.data_ptr(), k4, k4, d1.data_ptr(), d2.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return cnt, mm.cpu().numpy(), d1, d2


@pytest.mark.parametrize("rootsift", [False, True])
@pytest.mark.parametrize("refit", [False, True])
def test_single_entry_equals_the_composition_of_existing_entries(ctx, rootsift, refit):
    """mlpl_pair_pose_f32_dev field for field against mlpl_match_l2_dev -> mlpl_gather_match_points_dev -> mlpl_ransac_essential_dev ->
    mlpl_recover_pose_dev."""
    import torch
    from matchinglib_poselib_amd import pose
    for i, sp in enumerate(_pairs(3, 2048, 20260410, rootsift)):
        K = sp["K"]
        dq, dt, k1, k2 = (torch.from_numpy(sp[k]).cuda() for k in ("desc1", "desc2", "kp1", "kp2"))
        for rep in range(2):   # (RootSIFT, auto mode: the first call runs the exact kernel, the second the fp16 path)
            raw = _single_raw(ctx, dq, dt, k1, k2, K, seed=50 + i, refit=refit)
            cnt, mm, d1, d2 = _match_and_gather(ctx, dq, dt, k1, k2, K)
            r = pose.ransac_essential_device(d1, d2, TH(K), confidence=0.999, max_iters=1000, refit=refit, seed=50 + i, ctx=ctx)
            assert raw["status"] == 0 and r["ok"] and raw["pad"] == 0
            assert raw["n_matches"] == cnt and raw["iters"] == r["iters"] and raw["n_inliers"] == r["n_inliers"], (i, rep, raw, r)
            assert np.array_equal(raw["E"].view(np.uint64), np.asarray(r["E"]).ravel().view(np.uint64)), (i, rep)
            ng, R, t = pose.getPoseTriangPts_device(r["E"], d1, d2, mask=r["mask"], ctx=ctx)
            assert raw["n_good"] == ng and np.array_equal(raw["R"].view(np.uint64), R.ravel().view(np.uint64)), (i, rep)
            assert np.array_equal(raw["t"].view(np.uint64), t.ravel().view(np.uint64)), (i, rep)
            assert np.abs(raw["R"].reshape(3, 3) - sp["R"]).max() < 2e-2


@pytest.mark.parametrize("rootsift", [False, True])
@pytest.mark.parametrize("B", [1, 2, 8, 40])
def test_batch_records_equal_the_single_entry_and_the_matchers_list(ctx, rootsift, B):
    """Every record of mlpl_pair_pose_batch_f32_dev equals mlpl_pair_pose_f32_dev's byte for byte; d_matches_out equals mlpl_match_l2_dev's
    list; one pair of the larger batches matches nothing (status -1); refit != 0 falls back to the single entry (B = 2)."""
    import torch
    sps = _pairs(B, 1024, 20260500 + 100 * B, rootsift)
    if B >= 8:
        sps[3]["desc2"] = np.ascontiguousarray(sps[3]["desc2"][::-1] * 0 + sps[3]["desc2"][:1])   # every train row the same: d0 == d1, nothing passes
    K = sps[0]["K"]
    stk = _stack(sps)
    seeds = [900 + 7 * i for i in range(B)]
    mout = torch.zeros((B, 1024, 4), dtype=torch.int32, device="cuda")
    bat = _batch_raw(ctx, stk, K, seeds, matches_out=mout)
    mh = mout.cpu().numpy()
    for i in range(B):
        one = _single_raw(ctx, stk[0][i], stk[1][i], stk[2][i], stk[3][i], K, seeds[i])
        assert bat[i].tobytes() == one.tobytes(), (i, bat[i], one)
        cnt, mm, d1, d2 = _match_and_gather(ctx, stk[0][i], stk[1][i], stk[2][i], stk[3][i], K)
        assert cnt == bat["n_matches"][i] and mh[i, :cnt].tobytes() == mm.tobytes(), i
    if B >= 8:
        assert bat["status"][3] == -1 and bat["n_matches"][3] < 16
    assert (np.delete(bat["status"], 3 if B >= 8 else []) == 0).all()
    if B == 2:
        refit = _batch_raw(ctx, stk, K, seeds, refit=True)
        for i in range(B):
            assert refit[i].tobytes() == _single_raw(ctx, stk[0][i], stk[1][i], stk[2][i], stk[3][i], K, seeds[i], refit=True).tobytes(), i


@pytest.mark.parametrize("rootsift", [False, True])
@pytest.mark.parametrize("prosac,refine", [(False, 0), (True, 0), (True, 5)])
def test_usac_batch_equals_the_single_problem_entries_and_does_not_depend_on_the_feed(ctx, rootsift, prosac, refine):
    """mlpl_pair_pose_batch_usac_f32_dev per pair against match -> gather -> mlpl_usac_essential_dev -> mlpl_recover_pose_dev (uniform sampling,
    PROSAC in the order of the float matching costs, refine = 5); several cohorts (hub_cohort = 8) with the cohort feed and without it
    (pair_batch_feed = 0) byte for byte."""
    import torch
    from matchinglib_poselib_amd import batch, pose
    B, nk = 20, 1024
    sps = _pairs(B, nk, 20260700, rootsift)
    K = sps[0]["K"]
    stk = _stack(sps)
    seeds = [300 + 7 * i for i in range(B)]
    kw = dict(estimator=2, refine=refine, sprt_ms=6.0, sprt_tm=2736.0)
    rec, raw = batch.process_pairs_batched_usac(ctx, *stk, K, K, seeds, prosac=prosac, **kw)
    with options(ctx, hub_cohort=8):
        fed = batch.process_pairs_batched_usac(ctx, *stk, K, K, seeds, prosac=prosac, **kw)[1]
        with options(ctx, pair_batch_feed=0):
            unfed = batch.process_pairs_batched_usac(ctx, *stk, K, K, seeds, prosac=prosac, **kw)[1]
    assert fed.tobytes() == unfed.tobytes() == raw.tobytes()
    for i in range(B):
        cnt, mm, d1, d2 = _match_and_gather(ctx, stk[0][i], stk[1][i], stk[2][i], stk[3][i], K)
        assert raw["n_matches"][i] == cnt and cnt >= 16
        order = None
        if prosac:
            mh = np.ascontiguousarray(mm)
            order = np.zeros(cnt, np.uint32)
            assert ctx.lib.mlpl_sorted_match_idx(mh.ctypes.data, cnt, order.ctypes.data) == 0
            assert (np.diff(mh[:, 3].view(np.float32)[order]) >= 0).all()
        one = pose.usac_essential(d1.cpu().numpy(), d2.cpu().numpy(), TH(K), seeds[i], sorted_idx=order, prosac_beta=0.05, th_pixels=0.8,
                                  focal_length=float((2 * K[0] + 2 * K[1]) / 4.0), ctx=ctx, **kw)
        assert raw["status"][i] == 0 and one["ok"], i
        assert raw["iters"][i] == int(one["final"][1]) and raw["n_inliers"][i] == int(one["final"][5]), (i, raw[i], one["final"])
        assert np.array_equal(raw["E"][i].view(np.uint64), one["E"].view(np.uint64)), i
        ng, R, t = pose.getPoseTriangPts_device(one["E"].reshape(3, 3), d1, d2, mask=torch.from_numpy(one["flags"]).cuda(), ctx=ctx)
        assert raw["n_good"][i] == ng and np.array_equal(raw["R"][i].view(np.uint64), R.ravel().view(np.uint64)), i
        assert np.array_equal(raw["t"][i].view(np.uint64), t.ravel().view(np.uint64)), i


@pytest.mark.parametrize("rootsift", [False, True])
def test_arrsac_batch_equals_the_single_problem_entries_and_does_not_depend_on_the_feed(ctx, rootsift):
    import torch
    from matchinglib_poselib_amd import batch, pose
    B, nk = 16, 1024
    sps = _pairs(B, nk, 20260800, rootsift)
    K = sps[0]["K"]
    stk = _stack(sps)
    states = np.array([[0xFFFFFFFF + 11 * b, 0xFFFFFFFF + 5 * b] for b in range(B)], np.uint64)
    st_batch = states.copy()
    rec, raw = batch.process_pairs_batched_arrsac(ctx, *stk, K, K, refine=True, rng_states=st_batch)
    with options(ctx, hub_cohort=8):
        st2, st3 = states.copy(), states.copy()
        fed = batch.process_pairs_batched_arrsac(ctx, *stk, K, K, refine=True, rng_states=st2)[1]
        with options(ctx, pair_batch_feed=0):
            unfed = batch.process_pairs_batched_arrsac(ctx, *stk, K, K, refine=True, rng_states=st3)[1]
    assert fed.tobytes() == unfed.tobytes() == raw.tobytes() and np.array_equal(st2, st_batch) and np.array_equal(st3, st_batch)
    for i in range(B):
        cnt, mm, d1, d2 = _match_and_gather(ctx, stk[0][i], stk[1][i], stk[2][i], stk[3][i], K)
        assert raw["n_matches"][i] == cnt and cnt >= 16
        st = states[i].copy()
        one = pose.arrsac_essential(d1.cpu().numpy(), d2.cpu().numpy(), TH(K), refine=True, rng_state=st, ctx=ctx)
        assert np.array_equal(st, st_batch[i]), i
        if not one["ok"]:
            assert raw["status"][i] == -2
            continue
        assert raw["status"][i] == 0 and raw["n_inliers"][i] == one["n_inliers"], (i, raw[i])
        assert np.array_equal(raw["E"][i].view(np.uint64), one["E"].ravel().view(np.uint64)), i
        ng, R, t = pose.getPoseTriangPts_device(one["E"], d1, d2, mask=torch.from_numpy(one["mask"]).cuda(), ctx=ctx)
        assert raw["n_good"][i] == ng and np.array_equal(raw["R"][i].view(np.uint64), R.ravel().view(np.uint64)), i
        assert np.array_equal(raw["t"][i].view(np.uint64), t.ravel().view(np.uint64)), i


def _oracle_pair(oracle, sp):
    n = len(sp["desc1"])
    rc, mm = oracle.get_matches_linear(n, n, sp["desc1"], sp["desc2"])
    assert rc == 0
    K = sp["K"]
    return mm, _cam(sp["kp1"][mm["queryIdx"]], K), _cam(sp["kp2"][mm["trainIdx"]], K)


@pytest.mark.parametrize("rootsift", [False, True])
def test_ransac_batch_at_4096_keypoints_against_the_oracle_pipeline(ctx, oracle, rootsift):
    """4 pairs of 4096 keypoints: match count, iterations, inliers and n_good exact; E to 1e-8; R, t to 1e-6."""
    B, nk = 4, 4096
    sps = _pairs(B, nk, 20260400, rootsift)
    K = sps[0]["K"]
    seeds = [100 + i for i in range(B)]
    raw = _batch_raw(ctx, _stack(sps), K, seeds)
    for i in range(B):
        mm, p1, p2 = _oracle_pair(oracle, sps[i])
        o = oracle.ransac_essential(p1, p2, TH(K), confidence=0.999, max_iters=1000, lesqu=False, seed=seeds[i])
        print(f"pair {i}: matches {len(mm)} / {raw['n_matches'][i]}, iters {o['iters']} / {raw['iters'][i]}, inliers {o['n_inliers']} / {raw['n_inliers'][i]}, "
              f"E {e_dist(o['E'], raw['E'][i]):.3g}")
        assert raw["status"][i] == 0 and o["ok"] and len(mm) == raw["n_matches"][i], i
        assert o["iters"] == raw["iters"][i] and o["n_inliers"] == raw["n_inliers"][i], (i, o["iters"], o["n_inliers"], raw[i])
        assert e_dist(o["E"], raw["E"][i]) < 1e-8, i
        good, R, t, Q, mk = oracle.recover_pose(o["E"], p1, p2, 50.0, o["mask"])
        assert good == raw["n_good"][i], i
        assert np.abs(raw["R"][i].reshape(3, 3) - R).max() < 1e-6 and np.abs(raw["t"][i] - np.asarray(t).ravel()).max() < 1e-6, i


@pytest.mark.parametrize("rootsift", [False, True])
def test_usac_prosac_batch_at_4096_keypoints_against_the_oracle_pipeline(ctx, oracle, rootsift):
    """4 pairs of 4096 keypoints, USAC with PROSAC in the order of the float matching costs (the harness' cfgUSAC): match count,
    hypotheses, inliers and n_good exact; E to 1e-7; R, t to 1e-6."""
    from matchinglib_poselib_amd import batch
    B, nk = 4, 4096
    sps = _pairs(B, nk, 20260400, rootsift)
    K = sps[0]["K"]
    seeds = [100 + i for i in range(B)]
    rec, raw = batch.process_pairs_batched_usac(ctx, *_stack(sps), K, K, seeds, prosac=True, refine=0)
    for i in range(B):
        mm, p1, p2 = _oracle_pair(oracle, sps[i])
        assert raw["status"][i] == 0 and len(mm) == raw["n_matches"][i], i
        order = np.zeros(len(mm), np.uint32)
        mmc = np.ascontiguousarray(mm)
        assert ctx.lib.mlpl_sorted_match_idx(mmc.ctypes.data, len(mm), order.ctypes.data) == 0
        assert (np.diff(mm["distance"][order]) >= 0).all() and sorted(order.tolist()) == list(range(len(mm)))
        o = oracle.usac_essential(p1, p2, TH(K), seeds[i], refine=0, sorted_idx=order, prosac_beta=0.05, sprt_ms=6.0, sprt_tm=2736.0)
        print(f"pair {i}: matches {len(mm)}, hypotheses {int(o['final'][1])} / {raw['iters'][i]}, inliers {int(o['final'][5])} / {raw['n_inliers'][i]}, "
              f"E {e_dist(o['E'], raw['E'][i]):.3g}")
        assert o["ok"], i
        assert int(o["final"][1]) == raw["iters"][i] and int(o["final"][5]) == raw["n_inliers"][i], (i, o["final"][:8], raw[i])
        assert e_dist(o["E"], raw["E"][i]) < 1e-7, i
        good, R, t, Q, mk = oracle.recover_pose(o["E"], p1, p2, 50.0, o["flags"])
        assert good == raw["n_good"][i], i
        assert np.abs(raw["R"][i].reshape(3, 3) - R).max() < 1e-6 and np.abs(raw["t"][i] - np.asarray(t).ravel()).max() < 1e-6, i


@pytest.mark.parametrize("rootsift", [False, True])
def test_arrsac_batch_at_4096_keypoints_against_the_oracle_pipeline(ctx, oracle, rootsift):
    """4 pairs of 4096 keypoints with ARRSAC + robustEssentialRefine: match count, inliers and n_good exact; E to 1e-7; R, t to 1e-6.  A pair
    whose sampler streams end elsewhere (one first-stage hypothesis more or less: DESIGN section 8) is skipped, at most 1 of 4, as the
    uint8 test allows."""
    from matchinglib_poselib_amd import batch, pose
    B, nk = 4, 4096
    sps = _pairs(B, nk, 20260400, rootsift)
    K = sps[0]["K"]
    states = np.tile(np.array(pose.ARRSAC_RNG_FRESH, np.uint64), (B, 1))
    rec, raw = batch.process_pairs_batched_arrsac(ctx, *_stack(sps), K, K, refine=True, rng_states=states)
    skipped = 0
    for i in range(B):
        mm, p1, p2 = _oracle_pair(oracle, sps[i])
        assert len(mm) == raw["n_matches"][i], i
        o = oracle.arrsac_essential(p1, p2, TH(K), refine=True)
        same_stream = np.array_equal(o["rng_state"], states[i])
        print(f"pair {i}: matches {len(mm)}, streams equal {same_stream}, inliers {o['n_inliers']} / {raw['n_inliers'][i]}, E {e_dist(o['E'], raw['E'][i]):.3g}")
        if not same_stream:
            skipped += 1
            continue
        assert o["ok"] and raw["status"][i] == 0 and o["n_inliers"] == raw["n_inliers"][i], (i, o["n_inliers"], raw[i])
        assert e_dist(o["E"], raw["E"][i]) < 1e-7, i
        good, R, t, Q, mk = oracle.recover_pose(o["E"], p1, p2, 50.0, o["mask"])
        assert good == raw["n_good"][i], i
        assert np.abs(raw["R"][i].reshape(3, 3) - R).max() < 1e-6 and np.abs(raw["t"][i] - np.asarray(t).ravel()).max() < 1e-6, i
    assert skipped <= 1


@pytest.mark.parametrize("rootsift", [False, True])
@pytest.mark.parametrize("B", [1, 8])
def test_f32_entries_as_the_first_call_of_a_fresh_context(B, rootsift):
    """Each _f32 entry as the very first call on a fresh context (workspaces, pinned blocks, hint word and flag block all created inside
    the call, the nested matcher included) against the same entry on a warmed-up context, byte for byte."""
    import matchinglib_poselib_amd as mpa
    from matchinglib_poselib_amd import batch
    sps = _pairs(B, 4096, 20260900, rootsift)
    K = sps[0]["K"]
    stk = _stack(sps)
    seeds = [5 + i for i in range(B)]

    def run(c, which):
        if which == "single":
            return _single_raw(c, stk[0][0], stk[1][0], stk[2][0], stk[3][0], K, seeds[0])
        if which == "ransac":
            return _batch_raw(c, stk, K, seeds)
        if which == "arrsac":
            return batch.process_pairs_batched_arrsac(c, *stk, K, K, refine=True)[1]
        return batch.process_pairs_batched_usac(c, *stk, K, K, seeds, prosac=(which == "usac_prosac"))[1]

    names = ("single", "ransac", "usac", "usac_prosac", "arrsac")
    warm = mpa.Context(0)
    try:
        for _ in range(2):
            ref = {w: run(warm, w).copy() for w in names}
    finally:
        warm.close()
    for w in names:
        fresh = mpa.Context(0)
        try:
            got = run(fresh, w)
            assert (np.atleast_1d(got["status"]) == 0).all() and got.tobytes() == ref[w].tobytes(), (w, B)
        finally:
            fresh.close()


def test_fewer_than_16_matches_gives_status_minus_1(ctx):
    import torch
    from matchinglib_poselib_amd import batch, synth
    sp = synth.stereo_pair_f32(512, 3, unmatched_frac=0.3)
    sp["desc2"] = np.repeat(sp["desc2"][:1], 512, axis=0)      # every train row the same: d0 == d1, the ratio test passes nobody
    K = sp["K"]
    dq, dt, k1, k2 = (torch.from_numpy(sp[k]).cuda() for k in ("desc1", "desc2", "kp1", "kp2"))
    one = _single_raw(ctx, dq, dt, k1, k2, K, 1)
    assert one["status"] == -1 and one["n_matches"] == 0
    stk = [x[None].contiguous() for x in (dq, dt, k1, k2)]
    assert _batch_raw(ctx, stk, K, [1])["status"][0] == -1
    assert batch.process_pairs_batched_usac(ctx, *stk, K, K, [1])[1]["status"][0] == -1
    assert batch.process_pairs_batched_arrsac(ctx, *stk, K, K)[1]["status"][0] == -1


def test_python_entries_dispatch_on_the_descriptor_dtype(ctx):
    """float32 tensors reach the _f32 entries (same records as the C entry called directly); float64 is refused loudly."""
    import torch
    from matchinglib_poselib_amd import batch
    sps = _pairs(3, 1024, 20261000, False)
    K = sps[0]["K"]
    stk = _stack(sps)
    seeds = [1, 2, 3]
    raw = _batch_raw(ctx, stk, K, seeds)
    rec = batch.process_pairs_batched(ctx, *stk, K, K, seeds)
    assert np.array_equal(rec["n_matches"], raw["n_matches"]) and np.array_equal(rec["n_inliers"], raw["n_inliers"]) and np.array_equal(rec["E"], raw["E"])
    one = batch.process_pair_on_device(ctx, stk[0][1], stk[1][1], stk[2][1], stk[3][1], K, K, seed=2, pair_id=1)[0]
    assert one["n_matches"] == raw["n_matches"][1] and np.array_equal(one["E"], raw["E"][1])
    bad = [stk[0].double(), stk[1].double(), stk[2], stk[3]]
    for call in (lambda: batch.process_pairs_batched(ctx, *bad, K, K, seeds), lambda: batch.process_pairs_batched_usac(ctx, *bad, K, K, seeds),
                 lambda: batch.process_pairs_batched_arrsac(ctx, *bad, K, K),
                 lambda: batch.process_pair_on_device(ctx, bad[0][0], bad[1][0], stk[2][0], stk[3][0], K, K)):
        with pytest.raises(TypeError, match="float64"):
            call()
    with pytest.raises(TypeError):
        batch.process_pairs_batched(ctx, stk[0], stk[1].to(torch.uint8), stk[2], stk[3], K, K, seeds)
    lanes = batch.BatchLanes(0, lanes=2, first_ctx=ctx)
    try:
        with pytest.raises(AssertionError):      # the lanes entry stays uint8-only
            lanes.process(*stk, K, K, seeds)
    finally:
        lanes.close()
