"""mlpl_gms_filter_matches_dev: device-event time per call (windows of back-to-back calls between one pair of events, each window at least
20 ms or 1000 calls long, after a warm-up), median and range of the windows, for 1 x 2000, 1 x 8192
and 512 x 8192 matches (smooth scenes of synth.gms_scene) without the scale and rotation switches and 1 x 8192 with both; beside each,
mlpl_vfc_filter_matches_dev on the same lists.  The first list of every shape is checked against the single entry (byte-identical kept
list and count); exits 1 on a mismatch.  Writes profiles/gms_timing.txt.
usage: python tools/gms_timing.py [reps=20] [out=profiles/gms_timing.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import matching, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gms_timing.txt")
ctx = mpa.Context(0)
dev = torch.device("cuda:0")
lines, bad = [], 0
SIZE = (1280, 720)


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
    calls = int(min(1000, max(1, np.ceil(WINDOW_MS * 1e3 / window(fn, 10)))))
    return np.array([window(fn, calls) for _ in range(reps)]), calls


for B, n, switches in ((1, 2000, False), (1, 8192, False), (512, 8192, False), (1, 8192, True)):
    scenes = [synth.gms_scene("smooth", n, 100 + b) for b in range(min(B, 8))]   # eight distinct lists, repeated over the batch
    kp1 = np.stack([scenes[b % 8]["kp1"] for b in range(B)])
    kp2 = np.stack([scenes[b % 8]["kp2"] for b in range(B)])
    m = np.stack([scenes[b % 8]["matches"] for b in range(B)])
    d_m = torch.from_numpy(m.view(np.int32).reshape(B, n, 4)).to(dev)
    d_n = torch.full((B,), n, dtype=torch.int32, device=dev)
    d_k1, d_k2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
    out = matching.gms_filter_matches_device(d_m, d_n, d_k1, d_k2, SIZE, SIZE, switches, switches, ctx=ctx)
    t_gms, c_gms = timed(lambda: matching.gms_filter_matches_device(d_m, d_n, d_k1, d_k2, SIZE, SIZE, switches, switches, ctx=ctx, out=out))
    g = matching.gms_filter(kp1[0], SIZE, kp2[0], SIZE, m[0], switches, switches, ctx=ctx)
    exp = m[0][g["keep"]].view(np.int32).reshape(-1, 4)
    same = int(out["count"][0]) == len(exp) and out["matches"][0, :len(exp)].cpu().numpy().tobytes() == exp.tobytes()
    bad += 0 if same else 1
    vout = matching.vfc_filter_matches_device(d_m, d_n, d_k1, d_k2, ctx=ctx)
    t_vfc, c_vfc = timed(lambda: matching.vfc_filter_matches_device(d_m, d_n, d_k1, d_k2, ctx=ctx, out=vout), reps if B == 1 else 3)
    say(f"{B} x {n} matches, scale and rotation {'on' if switches else 'off'}: GMS median {np.median(t_gms):.1f} us (min {t_gms.min():.1f}, max "
        f"{t_gms.max():.1f} over {reps} windows of {c_gms} calls), kept {g['n_keep']} at run ({g['scale']}, {g['rotation']}); VFC on the same lists median "
        f"{np.median(t_vfc):.1f} us (min {t_vfc.min():.1f}, max {t_vfc.max():.1f} over {len(t_vfc)} windows of {c_vfc} calls), kept {int(vout['count'][0])}")
say(f"mismatches against the single entry: {bad}")
ctx.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
