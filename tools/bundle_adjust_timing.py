"""mlpl_refine_stereo_ba_batch_dev: 512 problems x 4096 points in one call, and one problem alone.  Per call: the wall time around a
synchronise (upload of the poses, the launch, the read-back of poses and info) and the kernel time from the library's profile counters
(mlpl_profile_read, kernel id 6).  Scenes as in tests/ba_scenes.py (noise 0.3 px, 15 % outliers, the facade's threshold).  A sample of the
batch is checked against the single entry (bit-identical); exits 1 on a mismatch.  Beside it the one-core time of tests/ba_oracle.py on
two of the scenes: a numpy RESTATEMENT, not the reference's speed.  Writes nothing: redirect the output
(profiles/bundle_adjust_timing.txt).  usage: python tools/bundle_adjust_timing.py [B=512] [n=4096] [reps=5]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import ba_scenes as S
import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import pose

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
PROF_BA = 6
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
scenes = [S.make_scene(n, seed=5000 + b) for b in range(B)]
d1 = torch.from_numpy(np.stack([s["p1"] for s in scenes])).to(dev)
d2 = torch.from_numpy(np.stack([s["p2"] for s in scenes])).to(dev)
q0 = torch.from_numpy(np.stack([s["Q"] for s in scenes])).to(dev)
R = np.stack([s["R"] for s in scenes])
t = np.stack([s["t"] for s in scenes])
dq = q0.clone()


def kernel_ms():
    ms, launches = C.c_double(0), C.c_int(0)
    assert ctx.lib.mlpl_profile_read(ctx.handle, PROF_BA, C.byref(ms), C.byref(launches)) == 0
    return ms.value, launches.value


def timed(nb):
    """nb problems per call -> wall us per call, kernel us per call, the last result"""
    counts = np.full(nb, n, np.int32)
    wall, kern, res = [], [], None
    for rep in range(reps + 1):  # the first call is the warm-up
        dq.copy_(q0)
        torch.cuda.synchronize()
        ctx.lib.mlpl_profile_reset(ctx.handle)
        t0 = time.perf_counter()
        res = pose.refine_stereo_ba_batch(d1[:nb], d2[:nb], counts, R[:nb], t[:nb], dq[:nb], S.TH, None, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        ms, launches = kernel_ms()
        assert launches == 1
        kern.append(ms * 1e3)
    return np.array(wall[1:]), np.array(kern[1:]), res


ctx.lib.mlpl_profile_enable(ctx.handle, 1)
w1, k1, _ = timed(1)
wB, kB, res = timed(B)
Qb = dq.cpu().numpy()
bad = 0
for b in range(0, B, max(1, B // 8)):
    s = scenes[b]
    one = pose.refine_stereo_ba(s["p1"], s["p2"], s["R"], s["t"], s["Q"], S.TH, None, S.ANGLE_THRESH, S.T_NORM_THRESH, ctx=ctx)
    same = (one["accepted"] == bool(res["accepted"][b]) and one["R"].tobytes() == res["R"][b].tobytes() and one["info"].tobytes() == res["info"][b].tobytes()
            and one["Q"].tobytes() == Qb[b].tobytes())
    bad += 0 if same else 1
it, att = res["info"][:, 5], res["info"][:, 9]
print(f"refine_stereo_ba_batch, 1 problem x {n}: wall {np.min(w1):.0f} us per call (median {np.median(w1):.0f}), kernel {np.min(k1):.0f} us (median {np.median(k1):.0f}), {reps} calls")
print(f"refine_stereo_ba_batch, {B} problems x {n}: wall {np.min(wB):.0f} us per call (median {np.median(wB):.0f}), kernel {np.min(kB):.0f} us (median {np.median(kB):.0f})"
      f" = {np.min(kB) / B:.1f} us of kernel time per problem, {reps} calls")
print(f"iterations per problem: mean {it.mean():.1f} (min {it.min():.0f}, max {it.max():.0f}); damping attempts: mean {att.mean():.1f}, max {att.max():.0f};"
      f" accepted {int(res['accepted'].sum())} of {B}; stop reasons {sorted(set(int(x) for x in res['info'][:, 6]))}")
print(f"workspace: {53 * 8 + 4} bytes per point = {B * n * (53 * 8 + 4) / 2**20:.0f} MiB for the batch")
ora, agree = [], 0
for b in range(min(2, B)):
    s = scenes[b]
    t0 = time.perf_counter()
    o = S.run_oracle(s)
    ora.append(time.perf_counter() - t0)
    agree += S.integers(o)[1:] == tuple(int(x) for x in res["info"][b][5:10])
print(f"tests/ba_oracle.py (a numpy restatement on one core, NOT the reference's speed), one problem x {n}: {np.min(ora) * 1e3:.0f} ms;"
      f" its iteration, stop and evaluation counts equal the device's on {agree} of {len(ora)}")
print(f"mismatches against the single entry: {bad}", flush=True)
ctx.close()
sys.exit(1 if bad else 0)
