"""What the Hamming ring kernel costs besides its tile loop: 64 C2 pairs (8192 queries each) against nt = 8192, 4096 and 2048 train rows, with two
neighbours and with one (k = 1 skips the epilogue's re-scoring of the best row's block).  Kernel time by the library's own events (every 4th
launch), the shader clock by the clock ring (option hamming_stamps = 2); every call asserts the 16x16x128 throughput instance.  The straight line
through the three train sizes gives the time per tile and the intercept -- launch, prologue and epilogue together -- and k = 2 minus k = 1 the
re-scoring alone.
    python tools/hamming_fixed_cost.py [pairs] [steps]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import matchinglib_poselib_amd as mpa  # noqa: E402
from matchinglib_poselib_amd import synth  # noqa: E402
from matchinglib_poselib_amd.matching import match_hamming_device  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 64
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
n = 8192
NTS = (8192, 4096, 2048)
KIND, QT, NWV, PD, INKERNEL = 2, 3, 5, 6, 12
dev = torch.device("cuda", 0)
ctx = mpa.Context(0)
lib = ctx.lib
qs, ts = zip(*[synth.orb_pair(n, n, seed=20260102 + p) for p in range(P)])
dq, dt = torch.from_numpy(np.stack(qs)).to(dev), torch.from_numpy(np.stack(ts)).to(dev)
ctx.set_option("hamming_stamps", 2)


def run(nt, k):
    t = dt[:, :nt]
    for _ in range(50):
        match_hamming_device(dq, t, ratio_test=k == 2, ctx=ctx)
    rec = ctx.last_kernels()
    assert (rec[KIND], rec[QT], rec[NWV], rec[PD], rec[INKERNEL]) == (4, 4, 8, 2, 1), rec
    assert ctx.last_hamming_shape() == 16 and ctx.last_hamming_top2() == 4, (ctx.last_hamming_shape(), ctx.last_hamming_top2())
    torch.cuda.synchronize()
    lib.mlpl_profile_reset(ctx.handle)
    lib.mlpl_profile_enable(ctx.handle, 4)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        match_hamming_device(dq, t, ratio_test=k == 2, ctx=ctx)
    e1.record()
    torch.cuda.synchronize()
    lib.mlpl_profile_enable(ctx.handle, 0)
    ms, cnt = C.c_double(0), C.c_int(0)
    lib.mlpl_profile_read(ctx.handle, 0, C.byref(ms), C.byref(cnt))
    buf = np.zeros((256, 4), np.uint64)
    m = lib.mlpl_debug_hamming_clock(ctx.handle, buf.ctypes.data, min(STEPS, 256))
    r = buf[:m].astype(np.float64)
    ghz = r[:, 0] / np.maximum(r[:, 1], 1) * 0.1
    out = {"nt": nt, "k": k, "step_us": e0.elapsed_time(e1) / STEPS * 1e3, "kernel_us": ms.value / max(cnt.value, 1) * 1e3, "launches_timed": cnt.value,
           "clock_GHz_median": float(np.median(ghz)), "first_workgroup_us_median": float(np.median(r[:, 1]) / 100.0)}
    print(json.dumps(out), flush=True)
    return out


res = {}
for rnd in range(2):
    for k in (2, 1):
        for nt in NTS:
            res[(rnd, k, nt)] = run(nt, k)
for rnd in range(2):
    for k in (2, 1):
        y = np.array([res[(rnd, k, nt)]["kernel_us"] for nt in NTS])
        slope, icpt = np.polyfit(np.array(NTS) / 32.0, y, 1)
        print(json.dumps({"round": rnd, "k": k, "kernel_us_per_tile": float(slope), "kernel_us_intercept": float(icpt),
                          "residual_us_max": float(np.abs(np.polyval([slope, icpt], np.array(NTS) / 32.0) - y).max())}), flush=True)
    print(json.dumps({"round": rnd, "k2_minus_k1_kernel_us": {str(nt): res[(rnd, 2, nt)]["kernel_us"] - res[(rnd, 1, nt)]["kernel_us"] for nt in NTS}}), flush=True)
ctx.close()
