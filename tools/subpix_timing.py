"""mlpl_subpix_matches_dev: device-event time per call (windows of back-to-back calls between one pair of events, each window at least
20 ms or 1000 calls long, after a warm-up), median and range of the windows, for 8192 matches per list at template sides 17 and 37
(keypoint sizes 0 and 31 on synth.subpix_scene textures of 1280 x 720), batch 1 and 64, with max_side set to the side and left at 0 (LDS
provisioned for side 255: one workgroup per compute unit).  The first list of every shape is checked against the single entry (mask, status
and keypoint bits); exits 1 on a mismatch.  Writes profiles/subpix_timing.txt.
usage: python tools/subpix_timing.py [reps=20] [out=profiles/subpix_timing.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import matching, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "subpix_timing.txt")
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
lines, bad = [], 0
N, W, H = 8192, 1280, 720


def say(s):
    print(s, flush=True)
    lines.append(s)


WINDOW_MS = 20.0   # one timed window: as many calls, enqueued back to back between one pair of events, as fill it (1000 at the most)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def timed(fn, reps=reps):
    """microseconds per call of every window, and the calls per window"""
    fn()   # warm-up (sizes the workspace)
    torch.cuda.synchronize()
    calls = int(min(1000, max(1, np.ceil(WINDOW_MS * 1e3 / window(fn, 3)))))
    return np.array([window(fn, calls) for _ in range(reps)]), calls


scenes = [synth.subpix_scene("texture", N, seed=200 + k, width=W, height=H, scramble=0.2) for k in range(4)]   # four image pairs, repeated over the batch
ident = np.zeros(N, matching.DMATCH_DTYPE)
ident["queryIdx"] = ident["trainIdx"] = np.arange(N)
for size, side in ((0.0, 17), (31.0, 37)):
    for B in (1, 64):
        pick = [scenes[b % 4] for b in range(B)]
        d_i1 = torch.from_numpy(np.stack([s["img1"] for s in pick])).to(dev)
        d_i2 = torch.from_numpy(np.stack([s["img2"] for s in pick])).to(dev)
        d_k1 = torch.from_numpy(np.stack([s["kp1"] for s in pick])).to(dev)
        d_k2 = torch.from_numpy(np.stack([s["kp2"] for s in pick])).to(dev)
        d_sz = torch.full((B, N), size, dtype=torch.float32, device=dev)
        d_m = torch.from_numpy(np.stack([ident] * B).view(np.int32).reshape(B, N, 4)).to(dev)
        d_n = torch.full((B,), N, dtype=torch.int32, device=dev)
        g = matching.subpix_matches(pick[0]["img1"], pick[0]["img2"], pick[0]["kp1"], pick[0]["kp2"], np.full(N, size, np.float32),
                                    np.full(N, size, np.float32), ctx=ctx)
        for max_side in (side, 0):
            out = matching.subpix_matches_device(d_m, d_n, d_k1, d_k2, d_i1, d_i2, d_sz, d_sz, max_side=max_side, ctx=ctx)
            t, c = timed(lambda: matching.subpix_matches_device(d_m, d_n, d_k1, d_k2, d_i1, d_i2, d_sz, d_sz, max_side=max_side, ctx=ctx, out=out),
                         reps if B == 1 else max(3, reps // 4))
            same = (out["inlier"][0].cpu().numpy().tobytes() == g["inlier"].astype(np.uint8).tobytes() and int(out["status"][0]) == g["status"]
                    and out["kp2"][0].cpu().numpy().tobytes() == g["kp2"].tobytes())
            bad += 0 if same else 1
            say(f"{B} x {N} matches, side {side}, max_side {max_side}: median {np.median(t):.1f} us per call (min {t.min():.1f}, max {t.max():.1f} over "
                f"{len(t)} windows of {c} calls), {np.median(t) * 1e3 / (B * N):.1f} ns per match; refined {g['n_refined']} of {N} in list 0")
say(f"mismatches against the single entry: {bad}")
ctx.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
