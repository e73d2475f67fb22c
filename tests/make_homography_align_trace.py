"""Writes tests/golden/homography_align_trace.npz: the restatement's outputs and info block (variant 0) for the FIXTURE scenes of
tests/homography_pose_scenes.py, and prints the variant distance S of every scene (the constant S_A is the largest, rounded up).
    python tests/make_homography_align_trace.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_align_oracle as hao  # noqa: E402
import homography_pose_scenes as S  # noqa: E402


def main():
    out, worst = {}, (0.0, None)
    for c in S.SCENES + S.GUARD:
        sc = S.scene(c[0])
        a, b = [hao.alignment(sc["p1"], sc["p2"], sc["labels"], sc["P"], sc["H0"], sc["th"], v) for v in (0, 1)]
        d = S.variant_distance(a, b)
        worst = max(worst, (d, c[0]))
        print(f"{c[0]:10s} n = {len(sc['p1']):5d}  S = {d:.3e}  same decisions: {S.same_decisions(a, b)}  stop margin {a['margin_stop']:.3e}  "
              f"q margin {a['margin_q']:.3e}  q = {a['q']}  rounds {a['rounds'].tolist()}")
        if c[0] in S.FIXTURE:
            for key in ("info", "R", "t", "E", "norms", "Hs"):
                out[f"{c[0]}_{key}"] = a[key]
    print(f"largest S = {worst[0]:.3e} (scene {worst[1]}); S_A = {S.S_A:.3e}, TOL_A = {S.TOL_A:.3e}")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "homography_align_trace.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
