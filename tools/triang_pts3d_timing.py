"""mlpl_triang_pts3d_batch_dev: device-event time per call for 512 problems x 4096 correspondences with masks (the scene's 50 % inliers), with
and without the 3-D points, beside mlpl_recover_pose_batch_dev (the four-way cheirality test on the essential matrix of the same pose) at
the same shape in the same run.  Warm-up first; every call starts from a fresh copy of the masks.  A sample of the problems is checked
against the single entry (bit-identical mask, count and points); exits 1 on a mismatch.  Writes nothing: redirect the output
(profiles/triang_pts3d_timing.txt).  usage: python tools/triang_pts3d_timing.py [B=512] [n=4096] [reps=10]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import pose, synth

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
scenes = [synth.pose_scene(n, 0.5, seed=20261000 + b, noise_px=0.3) for b in range(B)]
d1 = torch.from_numpy(np.stack([s[0] for s in scenes])).to(dev)
d2 = torch.from_numpy(np.stack([s[1] for s in scenes])).to(dev)
m0 = torch.from_numpy(np.stack([s[4].astype(np.uint8) for s in scenes])).to(dev)
R = np.stack([s[2] for s in scenes])
t = np.stack([s[3] for s in scenes])
skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])  # noqa: E731
E = np.stack([skew(s[3]) @ s[2] for s in scenes])
counts = np.full(B, n, np.int32)
dm = m0.clone()
dq = torch.zeros((B, n, 3), dtype=torch.float64, device=dev)


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for rep in range(reps + 1):  # the first call is the warm-up
        dm.copy_(m0)
        torch.cuda.synchronize()
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return np.array(ts[1:]), out


ts_m, good_m = timed(lambda: pose.triang_pts3d_batch(d1, d2, counts, R, t, dm, None, 50.0, ctx=ctx))
masks_m = dm.cpu().numpy()
ts_q, good_q = timed(lambda: pose.triang_pts3d_batch(d1, d2, counts, R, t, dm, dq, 50.0, ctx=ctx))
masks_q, Q = dm.cpu().numpy(), dq.cpu().numpy()
ts_r, rec = timed(lambda: pose.recover_pose_batch(d1, d2, counts, E, dm, 50.0, ctx=ctx))
bad = 0
h1, h2, hm = d1.cpu().numpy(), d2.cpu().numpy(), m0.cpu().numpy()
for b in range(0, B, max(1, B // 16)):
    g, Qs, ms = pose.triangPts3D(R[b], t[b], h1[b], h2[b], hm[b], 50.0, ctx=ctx)
    same = g == good_m[b] == good_q[b] and ms.tobytes() == masks_m[b].tobytes() == masks_q[b].tobytes() and Qs.tobytes() == Q[b].tobytes()
    bad += 0 if same else 1
for name, ts in (("triang_pts3d_batch, masks, no points", ts_m), ("triang_pts3d_batch, masks, points", ts_q), ("recover_pose_batch, masks", ts_r)):
    print(f"{name}: {B} problems x {n}: {np.min(ts):.0f} us per call (median {np.median(ts):.0f}, {reps} calls) = {np.min(ts) / B:.2f} us per problem")
print(f"valid points per problem: triang_pts3d {good_m.mean():.0f}, recover_pose {rec['n_good'].mean():.0f} (flagged {hm.sum(1).mean():.0f})")
print(f"mismatches against the single entry: {bad}", flush=True)
ctx.close()
sys.exit(1 if bad else 0)
