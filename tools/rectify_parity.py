"""mlpl_rectify_parameters against its restatement tests/rectify_oracle.py on the scenes of tests/rectify_scenes.py, and the yardstick of
that comparison: the distance between two evaluation orders of the restatement itself (the three 3 x 3 inverses by cofactors against
Gaussian elimination with partial pivoting).  Host arithmetic only: runs without a device.  Writes profiles/rectify_parity.txt.
usage: python tools/rectify_parity.py [out=profiles/rectify_parity.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import rectify_scenes as S
from matchinglib_poselib_amd import pose

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rectify_parity.txt")
lines = ["largest absolute difference per output: library - restatement (cofactors) | restatement, cofactors - elimination"]
for name in sorted(S.SCENES):
    g = pose.rectification_parameters(*S.call_args(name))
    o, l = S.oracle_parameters(name), S.oracle_parameters(name, "lu")
    cells = [f"{k} {np.abs(g[k] - o[k]).max():.3g} | {np.abs(o[k] - l[k]).max():.3g}" for k in ("Rect1", "Rect2", "Knew", "P1", "P2")]
    lines.append(f"{name}: " + "; ".join(cells))
    lines.append(f"  roi {g['roi']} (restatement {o['roi']}, elimination {l['roi']}); ceil / floor arguments " + ", ".join(f"{a:.4f}" for a in o["roi_args"]) +
                 f"; fc_new {o['info'][0]:.6f}, s0 {o['info'][1]:.6f}, s1 {o['info'][2]:.6f}, s {o['info'][3]:.6f}; reduction steps library "
                 f"{[int(v) for v in g['info'][4:]]}, restatement {[int(v) for v in o['info'][4:]]}")
print("\n".join(lines))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
