"""mlpl_subpix_separate_dev: device-event time per call (windows of back-to-back calls between one pair of events, each window at least
20 ms or 1000 calls long, after a warm-up), median and range of the windows, for 8192 matches per list at window half-sizes 3 and 10
(keypoint sizes 6 and 0 on synth.corner_scene checkerboards of 640 x 480, every keypoint up to 2 px from a corner), batch 1 and 64.  The
first list of every shape is checked against the single entry (mask, status and the bits of both keypoint arrays); exits 1 on a mismatch.
Writes profiles/subpix_separate_timing.txt, with the recorded figures of profiles/subpix_timing.txt beside its own.
usage: python tools/subpix_separate_timing.py [reps=20] [out=profiles/subpix_separate_timing.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import matching, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "subpix_separate_timing.txt")
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
lines, bad = [], 0
N, W, H = 8192, 640, 480


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


def scene(k):
    """image pair k: two boards at different angles, N keypoints up to 2 px from their corners"""
    rng = np.random.default_rng(300 + k)
    b1 = synth.corner_scene(W, H, angle=0.12 + 0.05 * k, origin=(5.3 + k, 7.7), supersample=4)
    b2 = synth.corner_scene(W, H, angle=-0.47 + 0.05 * k, origin=(11.6, 3.2 + k), supersample=4)
    kp1 = b1["corners"][rng.integers(0, len(b1["corners"]), N)] + rng.uniform(-2, 2, (N, 2))
    kp2 = b2["corners"][rng.integers(0, len(b2["corners"]), N)] + rng.uniform(-2, 2, (N, 2))
    return dict(img1=b1["img"], img2=b2["img"], kp1=kp1.astype(np.float32), kp2=kp2.astype(np.float32))


scenes = [scene(k) for k in range(4)]   # four image pairs, repeated over the batch
ident = np.zeros(N, matching.DMATCH_DTYPE)
ident["queryIdx"] = ident["trainIdx"] = np.arange(N)
for size, w in ((6.0, 3), (0.0, 10)):
    for B in (1, 64):
        pick = [scenes[b % 4] for b in range(B)]
        d_i1 = torch.from_numpy(np.stack([s["img1"] for s in pick])).to(dev)
        d_i2 = torch.from_numpy(np.stack([s["img2"] for s in pick])).to(dev)
        d_k1 = torch.from_numpy(np.stack([s["kp1"] for s in pick])).to(dev)
        d_k2 = torch.from_numpy(np.stack([s["kp2"] for s in pick])).to(dev)
        d_sz = torch.full((B, N), size, dtype=torch.float32, device=dev)
        d_m = torch.from_numpy(np.stack([ident] * B).view(np.int32).reshape(B, N, 4)).to(dev)
        d_n = torch.full((B,), N, dtype=torch.int32, device=dev)
        g = matching.subpix_separate(pick[0]["img1"], pick[0]["img2"], pick[0]["kp1"], pick[0]["kp2"], np.full(N, size, np.float32),
                                     np.full(N, size, np.float32), ctx=ctx)
        assert (g["w1"], g["w2"]) == (w, w)
        out = matching.subpix_separate_device(d_m, d_n, d_k1, d_k2, d_i1, d_i2, d_sz, d_sz, ctx=ctx)
        t, c = timed(lambda: matching.subpix_separate_device(d_m, d_n, d_k1, d_k2, d_i1, d_i2, d_sz, d_sz, ctx=ctx, out=out),
                     reps if B == 1 else max(3, reps // 4))
        same = (out["inlier"][0].cpu().numpy().tobytes() == g["inlier"].astype(np.uint8).tobytes() and int(out["status"][0]) == g["status"]
                and out["kp1"][0].cpu().numpy().tobytes() == g["kp1"].tobytes() and out["kp2"][0].cpu().numpy().tobytes() == g["kp2"].tobytes())
        bad += 0 if same else 1
        passes = float(g["iters"].mean())
        say(f"{B} x {N} matches, w {w}: median {np.median(t):.1f} us per call (min {t.min():.1f}, max {t.max():.1f} over {len(t)} windows of "
            f"{c} calls), {np.median(t) * 1e3 / (B * N):.1f} ns per match, {np.median(t) * 1e3 / (B * N * 2 * passes):.1f} ns per pass "
            f"({passes:.2f} passes per point in list 0); inliers {g['n_refined']} of {N} in list 0")
say(f"mismatches against the single entry: {bad}")
ref = os.path.join(ROOT, "profiles", "subpix_timing.txt")   # the template-matching refinement at the same list sizes, as last recorded
if os.path.exists(ref):
    say("for comparison, mlpl_subpix_matches_dev (profiles/subpix_timing.txt, max_side = the side):")
    for ln in open(ref):
        if "max_side 0" not in ln and " matches, side " in ln:
            say("  " + ln.split(" (min")[0] + "," + ln.split("),")[1].split(";")[0])
ctx.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
