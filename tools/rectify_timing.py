"""Stereo rectification: device-event time (torch.cuda.Event = hipEvent around windows of back-to-back calls, each window at least 20 ms
long, after a warm-up; median and range of the windows) of
  - one 1242 x 375 pair through the fused entry mlpl_rectify_images_dev,
  - 512 such pairs through the fused entry in one launch,
  - the same 512 pairs as mlpl_rectify_maps_dev followed by mlpl_remap_bilinear_dev per image (1024 x 2 launches, one pair of map buffers),
with the bytes each path has to move.  The fused result of pair 0 and of the last pair is compared with the two-step one; exits 1 on a
mismatch.  Writes profiles/rectify_timing.txt.
usage: python tools/rectify_timing.py [reps=9] [pairs=512] [out=profiles/rectify_timing.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import matchinglib_poselib_amd as mpa
import rectify_scenes as S
from matchinglib_poselib_amd import pose

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "rectify_timing.txt")
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
lines, bad = [], 0
WINDOW_MS = 20.0


def say(s):
    print(s, flush=True)
    lines.append(s)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def timed(fn):
    fn()   # warm-up (sizes the workspace, loads the code object)
    torch.cuda.synchronize()
    calls = int(min(1000, max(1, np.ceil(WINDOW_MS * 1e3 / window(fn, 2)))))
    return np.array([window(fn, calls) for _ in range(reps)]), calls


def report(what, t, calls, pairs, bytes_per_pixel):
    px = pairs * 2 * W * H
    med = np.median(t)
    say(f"{what}: median {med:.1f} us per call (min {t.min():.1f}, max {t.max():.1f} over {len(t)} windows of {calls} calls), "
        f"{med * 1e3 / (pairs * 2):.0f} ns per image, {px / med * 1e-3:.1f} Gpixel/s, {px * bytes_per_pixel / med * 1e-6:.2f} TB/s at {bytes_per_pixel} B per pixel")


W, H = S.out_size("kitti")
blocks = np.stack([pose.rectify_param_block(*S.map_args("kitti", side)) for side in (0, 1)])
# every pair gets its own parameters: the principal point of the new camera moves a little from pair to pair
params = np.repeat(blocks[None], B, 0).copy()
params[:, :, 28] += np.linspace(-3, 3, B)[:, None]
base = np.stack([S.image(W, H, 4), S.image(W, H, 5)])
d1 = torch.from_numpy(base[0]).to(dev)[None].repeat(B, 1, 1).contiguous()
d2 = torch.from_numpy(base[1]).to(dev)[None].repeat(B, 1, 1).contiguous()
for b in range(1, B):   # the images differ too
    d1[b] = torch.roll(d1[0], b, 1)
    d2[b] = torch.roll(d2[0], -b, 0)
o1, o2 = torch.empty_like(d1), torch.empty_like(d2)
mx = torch.empty((H, (W + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :W]
my = torch.empty((H, (W + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :W]
t1, t2 = torch.empty_like(d1), torch.empty_like(d2)


def fused(n):
    pose.rectify_images_batch(d1[:n], d2[:n], params[:n], out=(o1[:n], o2[:n]), ctx=ctx)


def two_step(n):
    for b in range(n):
        for side, (d, t) in enumerate(((d1, t1), (d2, t2))):
            p = params[b, side]
            pose.rectify_maps(p[:9], p[9:17], p[17:26], p[26:35], (W, H), ctx=ctx, device_out=(mx, my))
            pose.remap_bilinear(d[b], mx, my, ctx=ctx, device_out=t[b])


say(f"{W} x {H} images, 8-bit; fused: 1 B read (every source pixel once; the four taps of neighbouring pixels share cache lines) + 1 B written "
    f"per pixel; maps then remap: 8 B of maps written, 8 B read back, 1 B read, 1 B written")
t, c = timed(lambda: fused(1))
report("1 pair, fused (mlpl_rectify_images_dev)", t, c, 1, 2)
t, c = timed(lambda: fused(B))
report(f"{B} pairs, fused, one launch", t, c, B, 2)
tf = np.median(t)
t, c = timed(lambda: two_step(B))
report(f"{B} pairs, maps then remap, {4 * B} launches", t, c, B, 18)
say(f"fused / two-step = {tf / np.median(t):.3f}")
torch.cuda.synchronize()
for b in (0, B - 1):
    same = torch.equal(o1[b], t1[b]) and torch.equal(o2[b], t2[b])
    bad += 0 if same else 1
say(f"non-black share of pair 0: {float((o1[0] > 0).float().mean()):.3f}; mismatches between fused and two-step (pairs 0 and {B - 1}): {bad}")
ctx.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
