"""Writes tests/golden/homography_trace.npz from the sequential restatement (tests/cpp/homography_oracle.cpp) and prints, for every
scene of tests/homography_scenes.py, the distance s between the two variants of the restatement and the closest threshold comparison:
the numbers S_MAX in homography_scenes.py was set from.  Run from the repository root: python tests/make_homography_trace.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_oracle as ho  # noqa: E402
import homography_scenes as hs  # noqa: E402


def single_pair(name):
    p1, p2, H, planted, th = hs.single(name)
    a, b = ho.homography_arrsac(p1, p2, th), ho.homography_arrsac(p1, p2, th, variant=1)
    return p1, p2, th, a, b


def multi_pair(name, kw):
    p1, p2, Hs, label, th = hs.multi(name)
    a, b = ho.mult_homographies(p1, p2, th, **kw), ho.mult_homographies(p1, p2, th, variant=1, **kw)
    return p1, p2, th, a, b


def main():
    s_max = 0.0
    for c in hs.SINGLE:
        p1, p2, th, a, b = single_pair(c[0])
        s = hs.h_dist(a["H"], b["H"])
        s_max = max(s_max, s)
        print(f"{c[0]:12s} ok={a['ok']} inliers={a['n_inliers']} stats={a['stats'].tolist()} s={s:.3e} margin={min(a['margin'], b['margin']):.3e}")
    for name, kw in hs.MULTI_CASES:
        p1, p2, th, a, b = multi_pair(name, kw)
        s = max([hs.h_dist(x, y) for x, y in zip(a["H"], b["H"])], default=0.0)
        s_max = max(s_max, s)
        print(f"{name:6s} {kw} rc={a['rc']} planes={a['n_planes']} num_inl={a['num_inl'].tolist()} th_used/th={(a['th_used'] / th).tolist()} "
              f"s={s:.3e} margin={min(a['margin'], b['margin']):.3e}")
    print(f"S_MAX measured = {s_max:.3e}")
    out = {"cases": np.array(hs.FIXTURE)}
    for i, name in enumerate(hs.FIXTURE):
        p1, p2, th, a, b = single_pair(name)
        out.update({f"c{i}_p1": p1, f"c{i}_p2": p2, f"c{i}_th": np.array([th]), f"c{i}_ok": np.array([a["ok"]]), f"c{i}_stats": a["stats"],
                    f"c{i}_rng": a["rng_state"], f"c{i}_mask": np.packbits(a["mask"]), f"c{i}_H": a["H"]})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "homography_trace.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
