"""mlpl_refine_essential_linear_batch_dev: device-event time per call for 512 problems x 4096 correspondences (50 % inliers) starting from the
RANSAC batch entry's models and masks, for refineMethod 0x21, 0x23, 0x13 and 0x33; then the harness chain RANSAC batch -> refine 0x21 ->
mlpl_recover_pose_batch_dev against the RANSAC batch with recover_pose = 1.  Every refined problem is checked against the single-problem
entry (bit-identical E, mask, counts); exits 1 on a mismatch.  usage: python tools/linear_refine_timing.py [B=512] [n=4096] [reps=10]
With a fourth argument `kneip`: 0x21 as above and, beside it, PR_KNEIP (0x24) through mlpl_refine_essential_linear_rt_batch_dev from no start
rotation and from the rotation of its own first result, wall clock per call split into kneip_sums_kernel, the host solves,
kneip_eval_kernel and the hops (uploads, downloads, synchronisation), again checked against the single entry
(profiles/linear_refine_kneip_timing.txt)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import batch, pose, synth

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
kneip = len(sys.argv) > 4 and sys.argv[4] == "kneip"
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
scenes = [synth.pose_scene(n, 0.5, seed=20261000 + b, noise_px=0.3) for b in range(B)]
th = scenes[0][5]
d1 = torch.from_numpy(np.stack([s[0] for s in scenes])).to(dev)
d2 = torch.from_numpy(np.stack([s[1] for s in scenes])).to(dev)
counts = np.full(B, n, np.int32)
seeds = np.arange(B) + 1
m0 = torch.zeros((B, n), dtype=torch.uint8, device=dev)
rs = batch.ransac_pose_batched(ctx, d1, d2, counts, seeds, th, recover_pose=False, masks_out=m0)
E0 = np.stack([r["E"].reshape(9) for r in rs])
assert all(r["status"] == 0 for r in rs)
h1, h2, hm0 = d1.cpu().numpy(), d2.cpu().numpy(), m0.cpu().numpy()


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        fn(prep=True)
        torch.cuda.synchronize()
        ev[0].record()
        fn(prep=False)
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return np.array(ts)


bad = 0
dm = m0.clone()
for method in ((0x21,) if kneip else (0x21, 0x23, 0x13, 0x33)):
    out = {}

    def run(prep, method=method, out=out):
        if prep:
            dm.copy_(m0)
            return
        out["r"] = pose.refine_essential_linear_batch(d1, d2, counts, E0, dm, th, method, ctx=ctx)

    run(True), run(False)  # warm-up
    ts = timed(run)
    res, masks = out["r"], dm.cpu().numpy()
    for b in range(B):
        g = pose.refine_essential_linear(h1[b], h2[b], E0[b], hm0[b], method, th=th, ctx=ctx)
        same = (res["status"][b] == 0) == g["ok"] and res["E"][b].tobytes() == g["E"].tobytes() and masks[b].tobytes() == g["mask"].tobytes() \
            and res["n_inliers"][b] == g["n_inliers"] and res["steps_done"][b] == g["steps_done"]
        bad += 0 if same else 1
    print(f"refine 0x{method:02x}: {B} problems x {n}: {np.min(ts):.0f} us per call (median {np.median(ts):.0f}, {reps} calls) = "
          f"{np.min(ts) / B:.2f} us per problem; refined {int((res['status'] == 0).sum())}, mean steps {res['steps_done'].mean():.2f}, "
          f"mean inliers {E0.shape[0] and res['n_inliers'].mean():.0f} (RANSAC {hm0.sum(1).mean():.0f})", flush=True)

if kneip:
    pose.kneip_refine_times(ctx, enable=1)
    R_prev = None
    for label in ("no start rotation (12 perturbed starts at step 0)", "start rotation = the first run's result"):
        wall, split = [], []
        for rep in range(reps + 1):  # the first call is the warm-up
            dm.copy_(m0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pose.refine_essential_linear_rt_batch(d1, d2, counts, E0, dm, th, 0x24, R=R_prev, seeds=seeds, ctx=ctx)
            wall.append((time.perf_counter() - t0) * 1e6)
            split.append(pose.kneip_refine_times(ctx))
        wall, split = np.array(wall[1:]), split[1:]
        k = int(np.argmin(wall))
        masks = dm.cpu().numpy()
        for b in range(B):
            g = pose.refine_essential_linear_rt(h1[b], h2[b], E0[b], hm0[b], 0x24, R=None if R_prev is None else R_prev[b], th=th, seed=int(seeds[b]),
                                                ctx=ctx)
            same = (res["status"][b] == 0) == g["ok"] and res["E"][b].tobytes() == g["E"].tobytes() and masks[b].tobytes() == g["mask"].tobytes() \
                and res["n_inliers"][b] == g["n_inliers"] and res["steps_done"][b] == g["steps_done"] and bool(res["rt_valid"][b]) == g["rt_valid"] \
                and (not g["rt_valid"] or (res["R"][b].tobytes() == g["R"].tobytes() and res["t"][b].tobytes() == g["t"].tobytes()))
            bad += 0 if same else 1
        sp = split[k]
        print(f"refine 0x24, {label}: {B} problems x {n}: {np.min(wall):.0f} us per call, wall clock (median {np.median(wall):.0f}, {reps} calls) = "
              f"{np.min(wall) / B:.2f} us per problem; of the fastest call: sums kernel {sp['sums'] * 1e6:.0f} us, host solves {sp['solve'] * 1e6:.0f} us, "
              f"eval kernel {sp['eval'] * 1e6:.0f} us, hops {sp['hops'] * 1e6:.0f} us; refined {int((res['status'] == 0).sum())}, "
              f"with pose {int(res['rt_valid'].sum())}, mean steps {res['steps_done'].mean():.2f}, mean attempts {res['attempts_used'].mean():.2f}, "
              f"mean inliers {res['n_inliers'].mean():.0f} (RANSAC {hm0.sum(1).mean():.0f})", flush=True)
        if R_prev is None:
            R_prev = np.where(res["rt_valid"][:, None, None] != 0, res["R"], np.eye(3)[None])
    pose.kneip_refine_times(ctx, enable=0)
    print(f"mismatches against the single entry: {bad}", flush=True)
    ctx.close()
    sys.exit(1 if bad else 0)


def chain(prep):
    if prep:
        return
    rr = batch.ransac_pose_batched(ctx, d1, d2, counts, seeds, th, recover_pose=False, masks_out=dm)
    E = np.stack([r["E"].reshape(9) for r in rr])
    ref = pose.refine_essential_linear_batch(d1, d2, counts, E, dm, th, 0x21, ctx=ctx)
    pose.recover_pose_batch(d1, d2, counts, ref["E"], dm, ctx=ctx)


def plain(prep):
    if prep:
        return
    batch.ransac_pose_batched(ctx, d1, d2, counts, seeds, th, recover_pose=True, masks_out=dm)


chain(False), plain(False)
tc, tp = timed(chain), timed(plain)
print(f"chain RANSAC batch -> refine 0x21 -> recover_pose_batch: {np.min(tc) / 1e3:.2f} ms (median {np.median(tc) / 1e3:.2f}); "
      f"RANSAC batch with recover_pose = 1: {np.min(tp) / 1e3:.2f} ms (median {np.median(tp) / 1e3:.2f})", flush=True)
print(f"mismatches against the single entry: {bad}", flush=True)
ctx.close()
sys.exit(1 if bad else 0)
