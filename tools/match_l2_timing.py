"""Device-event timing of the float match and pair entries.

  match  mlpl_match_l2_dev with l2_fold_counts = 1 and 0 against the two-call chain mlpl_knn2_l2sq_f32_dev + mlpl_ratio_compact_f32_dev (the
         baseline: what a caller had before the entry existed) on BASELINE config 4's shape, 4096 x 4096 x 128, integer-valued and RootSIFT
         rows, batch 1 and 64.  The variants alternate call by call in one process; every call sits between two device events.
  pairs  mlpl_pair_pose_batch_f32_dev / mlpl_pair_pose_batch_usac_f32_dev (PROSAC) on 64 and 512 pairs of 4096 keypoints against the composition
         of existing entries (batched match chain, count read-back, a gather per pair, mlpl_ransac_essential_batch_dev /
         mlpl_usac_essential_batch_dev + mlpl_recover_pose_batch_dev), and the uint8 entries at the same keypoint count.
The whole measurement is repeated `runs` times: the spread of a variant's medians over the runs is its run-to-run spread.
usage: python tools/match_l2_timing.py [match|pairs|all] [calls=200] [runs=3] [pair_calls=calls]   (prints; tee it into profiles/match_l2_timing.txt)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import batch, pose, synth
from matchinglib_poselib_amd._lib import check
from matchinglib_poselib_amd.matching import match_l2_device

what = sys.argv[1] if len(sys.argv) > 1 else "all"
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
pair_calls = int(sys.argv[4]) if len(sys.argv) > 4 else calls
ctx = mpa.Context(0)
dev = torch.device("cuda:0")


def alternate(variants, n):
    """variants: {name: fn}; n calls of each, round robin, each between two device events -> {name: microseconds [n]}."""
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for k in variants}
    for i in range(n):
        for k, fn in variants.items():
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
        if i % 16 == 15:
            torch.cuda.synchronize()   # keep the queue of pending events short
    torch.cuda.synchronize()
    return {k: np.array([a.elapsed_time(b) * 1e3 for a, b in ev[k]]) for k in variants}


def report(title, variants, n, unit_pairs=0):
    for fn in variants.values():   # warm up every shape and variant
        fn(), fn()
    torch.cuda.synchronize()
    med = {k: [] for k in variants}
    for r in range(runs):
        ts = alternate(variants, n)
        for k in variants:
            med[k].append(float(np.median(ts[k])))
    print(title, flush=True)
    for k in variants:
        m = np.array(med[k])
        extra = f", {unit_pairs / (np.median(m) * 1e-6):.0f} pairs/s" if unit_pairs else ""
        print(f"    {k:34s} median {np.median(m):10.1f} us  (medians of the {runs} runs: {', '.join(f'{v:.1f}' for v in m)}; spread {m.max() - m.min():.1f} us; "
              f"{n} calls per run){extra}", flush=True)
    return {k: (float(np.median(med[k])), float(np.max(med[k]) - np.min(med[k]))) for k in variants}


def match_section():
    nq = nt = 4096
    for kind in ("integer", "rootsift", "rootsift, l2_float_mfma = 0"):
        for B in (1, 64):
            sps = [synth.stereo_pair_f32(nq, 20260400 + b, unmatched_frac=0.3, rootsift=kind != "integer") for b in range(min(B, 8))]
            q = torch.from_numpy(np.stack([sps[b % len(sps)]["desc1"] for b in range(B)])).to(dev)
            t = torch.from_numpy(np.stack([sps[b % len(sps)]["desc2"] for b in range(B)])).to(dev)
            out = {"idx": torch.empty((B, nq, 2), dtype=torch.int32, device=dev), "dist": torch.empty((B, nq, 2), dtype=torch.float32, device=dev),
                   "matches": torch.empty((B, nq, 4), dtype=torch.int32, device=dev), "count": torch.empty((B,), dtype=torch.int32, device=dev)}
            st = torch.cuda.current_stream(dev).cuda_stream
            ctx.set_option("l2_float_mfma", 0 if kind.endswith("= 0") else 1)

            def entry(fold):
                ctx.set_option("l2_fold_counts", fold)
                match_l2_device(q, t, ctx=ctx, out=out, stream=st)

            def chain():
                check(ctx.lib.mlpl_knn2_l2sq_f32_dev(ctx.handle, q.data_ptr(), nq, 128, nq * 128, t.data_ptr(), nt, 128, nt * 128, 128, 2, B, out["idx"].data_ptr(),
                                                     out["dist"].data_ptr(), st), "knn")
                check(ctx.lib.mlpl_ratio_compact_f32_dev(ctx.handle, out["idx"].data_ptr(), out["dist"].data_ptr(), nq, 2, B, 0.75, out["matches"].data_ptr(),
                                                         out["count"].data_ptr(), st), "ratio")

            res = report(f"match 4096 x 4096 x 128, {kind}, batch {B}:", {"two-call chain (baseline)": chain, "match_l2_dev, l2_fold_counts = 1": lambda: entry(1),
                                                                         "match_l2_dev, l2_fold_counts = 0": lambda: entry(0)}, calls)
            entry(1)
            torch.cuda.synchronize()
            base, on = res["two-call chain (baseline)"], res["match_l2_dev, l2_fold_counts = 1"]
            print(f"    last call: path / splits / fold counts / launches = {ctx.last_l2_match()}, {int(out['count'][0].item())} matches in pair 0; "
                  f"option on - baseline = {on[0] - base[0]:+.1f} us against the baseline's spread of {base[1]:.1f} us -> "
                  f"{'within the bar' if on[0] - base[0] <= base[1] else 'SLOWER than the bar allows'}", flush=True)
    ctx.set_option("l2_float_mfma", 1)
    ctx.set_option("l2_fold_counts", 1)


def pairs_section():
    nk = 4096
    for B in (64, 512):
        f32 = [synth.stereo_pair_f32(nk, 20260400 + b, unmatched_frac=0.3 + 0.02 * (b % 8)) for b in range(16)]
        u8 = [synth.stereo_pair(nk, seed=20260200 + b, unmatched_frac=0.3 + 0.02 * (b % 8)) for b in range(16)]
        K = f32[0]["K"]
        th = 0.8 * 4.0 / (np.sqrt(2.0) * (2 * K[0] + 2 * K[1]))
        k4 = (C.c_double * 4)(*K)
        stk = [torch.from_numpy(np.stack([f32[b % 16][k] for b in range(B)])).to(dev) for k in ("desc1", "desc2", "kp1", "kp2")]
        stk8 = [torch.from_numpy(np.stack([u8[b % 16][k] for b in range(B)])).to(dev) for k in ("desc1", "desc2", "kp1", "kp2")]
        seeds = np.arange(B) + 100
        mt = {"idx": torch.empty((B, nk, 2), dtype=torch.int32, device=dev), "dist": torch.empty((B, nk, 2), dtype=torch.float32, device=dev),
              "matches": torch.empty((B, nk, 4), dtype=torch.int32, device=dev), "count": torch.empty((B,), dtype=torch.int32, device=dev)}
        p1 = torch.zeros((B, nk, 2), dtype=torch.float64, device=dev)
        p2 = torch.zeros((B, nk, 2), dtype=torch.float64, device=dev)
        masks = torch.zeros((B, nk), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream

        def front():
            """batched match chain, count read-back, a gather per pair -> counts"""
            check(ctx.lib.mlpl_knn2_l2sq_f32_dev(ctx.handle, stk[0].data_ptr(), nk, 128, nk * 128, stk[1].data_ptr(), nk, 128, nk * 128, 128, 2, B,
                                                 mt["idx"].data_ptr(), mt["dist"].data_ptr(), st), "knn")
            check(ctx.lib.mlpl_ratio_compact_f32_dev(ctx.handle, mt["idx"].data_ptr(), mt["dist"].data_ptr(), nk, 2, B, 0.75, mt["matches"].data_ptr(),
                                                     mt["count"].data_ptr(), st), "ratio")
            counts = mt["count"].cpu().numpy()
            for b in range(B):
                check(ctx.lib.mlpl_gather_match_points_dev(ctx.handle, mt["matches"][b].data_ptr(), int(counts[b]), stk[2][b].data_ptr(), stk[3][b].data_ptr(), k4, k4,
                                                           p1[b].data_ptr(), p2[b].data_ptr(), st), "gather")
            return counts

        def comp_ransac():
            counts = front()
            batch.ransac_pose_batched(ctx, p1, p2, counts, seeds, th, recover_pose=True, masks_out=masks)

        def comp_usac():
            counts = front()
            mh = mt["matches"].cpu().numpy()
            orders = []
            for b in range(B):
                o = np.zeros(int(counts[b]), np.uint32)
                check(ctx.lib.mlpl_sorted_match_idx(np.ascontiguousarray(mh[b, :counts[b]]).ctypes.data, int(counts[b]), o.ctypes.data), "sort")
                orders.append(o)
            got = pose.usac_essential_batch(p1, p2, counts, th, seeds, sorted_idx=orders, prosac_beta=0.05, sprt_ms=6.0, sprt_tm=2736.0, estimator=2,
                                            masks_out=masks, ctx=ctx)
            pose.recover_pose_batch(p1, p2, counts, np.stack([g["E"].reshape(9) for g in got]), masks, ctx=ctx)

        report(f"{B} pairs of {nk} keypoints, RANSAC:", {"composition of existing entries": comp_ransac,
                                                          "mlpl_pair_pose_batch_f32_dev": lambda: batch.process_pairs_batched(ctx, *stk, K, K, seeds),
                                                          "mlpl_pair_pose_batch_dev (uint8)": lambda: batch.process_pairs_batched(ctx, *stk8, K, K, seeds)},
               pair_calls, unit_pairs=B)
        report(f"{B} pairs of {nk} keypoints, USAC-PROSAC:", {"composition of existing entries": comp_usac,
                                                               "mlpl_pair_pose_batch_usac_f32_dev": lambda: batch.process_pairs_batched_usac(ctx, *stk, K, K, seeds, prosac=True),
                                                               "mlpl_pair_pose_batch_usac_dev (uint8)": lambda: batch.process_pairs_batched_usac(ctx, *stk8, K, K, seeds, prosac=True)},
               pair_calls, unit_pairs=B)


print(f"{mpa.load_library().mlpl_version().decode()}; {torch.cuda.get_device_name(0)}; calls {calls}, pair calls {pair_calls}, runs {runs}", flush=True)
if what in ("match", "all"):
    match_section()
if what in ("pairs", "all"):
    pairs_section()
ctx.close()
