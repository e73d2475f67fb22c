"""mlpl_vfc_filter_matches_dev: device-event time per call for 512 match lists of about 500 and about 3000 matches (clean scenes of
synth.vfc_scene, list lengths spread by +-10 %), after a warm-up call, median and range of the repetitions, for both settings of option
"vfc_store_u" (0 = the kernel recomputes the m x n kernel matrix U in both passes of an iteration, 1 = it keeps U in the workspace); beside
it the wall time of 512 sequential mlpl_vfc_filter calls on the same lists.  Every list of the batch is checked against the single entry
(byte-identical kept lists, counts, status); exits 1 on a mismatch.  Writes profiles/vfc_timing.txt.
usage: python tools/vfc_timing.py [B=512] [reps=10] [out=profiles/vfc_timing.txt]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import matching, synth

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "vfc_timing.txt")
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
lines, bad = [], 0


def say(s):
    print(s, flush=True)
    lines.append(s)


for centre in (500, 3000):
    rng = np.random.default_rng(centre)
    counts = rng.integers(int(centre * 0.9), int(centre * 1.1) + 1, B).astype(np.int32)
    stride = int(counts.max())
    scenes = [synth.vfc_scene("clean", int(n), 1000 + b) for b, n in enumerate(counts)]
    kp1, kp2 = np.zeros((B, stride, 2), np.float32), np.zeros((B, stride, 2), np.float32)
    m = np.zeros((B, stride), matching.DMATCH_DTYPE)
    for b, s in enumerate(scenes):
        kp1[b, :counts[b]], kp2[b, :counts[b]] = s["x1"], s["x2"]
        m["queryIdx"][b, :counts[b]] = m["trainIdx"][b, :counts[b]] = np.arange(counts[b])
    d_m = torch.from_numpy(m.view(np.int32).reshape(B, stride, 4)).to(dev)
    d_n, d_k1, d_k2 = torch.from_numpy(counts).to(dev), torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
    seeds = np.arange(B, dtype=np.uint32) + 1
    ref = None
    for store_u in (0, 1):
        mpa._lib.check(ctx.lib.mlpl_set_option(ctx.handle, b"vfc_store_u", store_u), "mlpl_set_option")
        out = matching.vfc_filter_matches_device(d_m, d_n, d_k1, d_k2, seeds, ctx=ctx)   # warm-up (sizes the workspace)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            matching.vfc_filter_matches_device(d_m, d_n, d_k1, d_k2, seeds, ctx=ctx, out=out)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = np.array(ts)
        got = (out["matches"].cpu().numpy(), out["count"].cpu().numpy(), out["status"].cpu().numpy())
        t0 = time.perf_counter()
        singles = [matching.vfc_filter_points(s["x1"], s["x2"], int(seeds[b]), ctx) for b, s in enumerate(scenes)]
        t_seq = (time.perf_counter() - t0) * 1e3
        for b, g in enumerate(singles):
            exp = m[b, :counts[b]][g["keep"]].view(np.int32).reshape(-1, 4)
            same = got[2][b] == g["rc"] and got[1][b] == len(exp) and got[0][b, :len(exp)].tobytes() == exp.tobytes()
            bad += 0 if same else 1
        if ref is None:
            ref = got
        else:
            bad += 0 if all(a.tobytes() == c.tobytes() for a, c in zip(ref[1:], got[1:])) else 1
        its = np.array([g["iterations"] for g in singles])
        say(f"vfc_store_u={store_u}: {B} lists of {counts.min()}-{counts.max()} matches: batch call median {np.median(ts):.3f} ms (min {ts.min():.3f}, max "
            f"{ts.max():.3f}, {reps} calls) = {np.median(ts) * 1e3 / B:.2f} us per list; {B} sequential mlpl_vfc_filter calls {t_seq:.1f} ms wall "
            f"= {t_seq * 1e3 / B:.1f} us each; iterations mean {its.mean():.1f} (min {its.min()}, max {its.max()}), kept "
            f"{np.mean([g['n_keep'] for g in singles]) / counts.mean():.3f} of the matches, status != 0 in {int((got[2] != 0).sum())}")
mpa._lib.check(ctx.lib.mlpl_set_option(ctx.handle, b"vfc_store_u", 0), "mlpl_set_option")
say(f"mismatches against the single entry or between the two settings: {bad}")
ctx.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
