"""mlpl_refine_multicam_ba_batch_dev: for m in {2, 4, 8, 16} cameras at 4096 points with about 60 % visibility (every point in at least two
cameras, so m = 2 is full visibility), one problem alone and 512 problems in one call.  Per call: the wall time around a synchronise (upload
of the poses, the launch, the read-back of poses and info) and the kernel time from the library's profile counters (mlpl_profile_read,
kernel id 7).  The 512 problems are 8 distinct scenes (tests/ba_multicam_scenes.py: noise 0.3 px, 15 % outliers, the facade's threshold)
repeated 64 times.  The m = 2 data also go through the existing stereo entry (mlpl_refine_stereo_ba_batch_dev, kernel id 6): the ratio of the
two kernel times is the figure a tuning change starts from.  A sample of each batch is checked against the single entry (bit-identical);
exits 1 on a mismatch.  Writes the figures to the file named (default profiles/ba_multicam_timing.txt) and to stdout.
usage: python tools/ba_multicam_timing.py [out] [B=512] [n=4096] [reps=3]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import ba_multicam_scenes as S
import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import pose

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ba_multicam_timing.txt")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
DISTINCT = 8
PROF_STEREO, PROF_MULTICAM = 6, 7
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def kernel_ms(kid):
    ms, launches = C.c_double(0), C.c_int(0)
    assert ctx.lib.mlpl_profile_read(ctx.handle, kid, C.byref(ms), C.byref(launches)) == 0
    return ms.value, launches.value


def timed(kid, call, restore):
    """-> wall us per call, kernel us per call, the last result; the first call is the warm-up"""
    wall, kern, res = [], [], None
    for _ in range(reps + 1):
        restore()
        torch.cuda.synchronize()
        ctx.lib.mlpl_profile_reset(ctx.handle)
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        ms, launches = kernel_ms(kid)
        assert launches == 1
        kern.append(ms * 1e3)
    return np.array(wall[1:]), np.array(kern[1:]), res


ctx.lib.mlpl_profile_enable(ctx.handle, 1)
bad, k_m2 = 0, None
for m in (2, 4, 8, 16):
    scenes = [S.make_scene(m, n, seed=7000 + 16 * m + k, vis=S.vis_frac(0.6)) for k in range(min(DISTINCT, B))]
    pick = [b % len(scenes) for b in range(B)]
    th = scenes[0]["th"]
    dp = torch.from_numpy(np.stack([scenes[k]["p"] for k in pick])).to(dev)
    dv = torch.from_numpy(np.stack([scenes[k]["vis"] for k in pick])).to(dev)
    q0 = torch.from_numpy(np.stack([scenes[k]["Q"] for k in pick])).to(dev)
    R, t = np.stack([scenes[k]["R"] for k in pick]), np.stack([scenes[k]["t"] for k in pick])
    dq = q0.clone()
    per = {}
    for nb in (1, B):
        cams, counts = np.full(nb, m, np.int32), np.full(nb, n, np.int32)
        per[nb] = timed(PROF_MULTICAM, lambda: pose.refine_multicam_ba_batch(dp[:nb], dv[:nb], cams, counts, R[:nb], t[:nb], dq[:nb], th,
                                                                             S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx), lambda: dq.copy_(q0))
    (w1, k1, _), (wB, kB, res) = per[1], per[B]
    Qb = dq.cpu().numpy()
    for b in range(min(len(scenes), B)):
        s = scenes[b]
        one = pose.refine_multicam_ba(s["p"], s["vis"], s["R"], s["t"], s["Q"], th, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
        same = (one["accepted"] == bool(res["accepted"][b]) and one["R"].tobytes() == res["R"][b].tobytes()
                and one["info"].tobytes() == res["info"][b].tobytes() and one["Q"].tobytes() == Qb[b].tobytes())
        bad += 0 if same else 1
    it, att = res["info"][:, 5], res["info"][:, 9]
    vis_frac = float(np.mean([s["vis"].mean() for s in scenes]))
    say(f"refine_multicam_ba_batch, m = {m}, {n} points, visibility {vis_frac:.2f}, reduced system {6 * (m - 1)} x {6 * (m - 1)}:")
    say(f"  1 problem: wall {np.min(w1):.0f} us per call (median {np.median(w1):.0f}), kernel {np.min(k1):.0f} us (median {np.median(k1):.0f}), {reps} calls")
    say(f"  {B} problems: wall {np.min(wB):.0f} us per call (median {np.median(wB):.0f}), kernel {np.min(kB):.0f} us (median {np.median(kB):.0f})"
        f" = {np.min(kB) / B:.1f} us of kernel time per problem")
    say(f"  iterations per problem: mean {it.mean():.1f} (max {it.max():.0f}); damping attempts: mean {att.mean():.1f}; accepted"
        f" {int(res['accepted'].sum())} of {B}; workspace {(27 + 22 * m) * 8} bytes per point = {B * n * (27 + 22 * m) * 8 / 2**20:.0f} MiB")
    if m == 2:
        k_m2 = (np.min(k1), np.min(kB))
        assert all(s["vis"].all() for s in scenes)
        d1, d2 = dp[:, 0].contiguous(), dp[:, 1].contiguous()
        Rs, ts = np.ascontiguousarray(R[:, 1]), np.ascontiguousarray(t[:, 1])
        st = {}
        for nb in (1, B):
            counts = np.full(nb, n, np.int32)
            st[nb] = timed(PROF_STEREO, lambda: pose.refine_stereo_ba_batch(d1[:nb], d2[:nb], counts, Rs[:nb], ts[:nb], dq[:nb], th, None,
                                                                            S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx), lambda: dq.copy_(q0))
        (sw1, sk1, _), (swB, skB, sres) = st[1], st[B]
        counts_equal = int(np.sum((sres["info"][:, 5:10] == res["info"][:, 5:10]).all(axis=1)))
        verdict_equal = int(np.sum(sres["accepted"] == res["accepted"]))  # (the stereo wrapper does not normalise the OLD t before getRTQuality)
        say(f"  the same data through refine_stereo_ba_batch: 1 problem: wall {np.min(sw1):.0f} us, kernel {np.min(sk1):.0f} us; {B} problems: wall"
            f" {np.min(swB):.0f} us, kernel {np.min(skB):.0f} us = {np.min(skB) / B:.1f} us per problem; iteration, stop and evaluation counts equal on {counts_equal} of {B}, verdict on {verdict_equal}")
        say(f"  kernel time, multi-camera entry / stereo entry at m = 2: {k_m2[0] / np.min(sk1):.2f} (1 problem), {k_m2[1] / np.min(skB):.2f} ({B} problems)")
    del dp, dv, q0, dq
    torch.cuda.empty_cache()
say(f"mismatches against the single entry: {bad}")
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
