"""Seeded scenes for the homography tests (tests/test_oracle_homography.py on the CPU, tests/test_gpu_homography.py on the device):
one plane plus uniform outliers and Gaussian noise, in pixel units (coordinates up to 1000, th = 1.5) or camera units
(th = 0.8 * 4 / (sqrt(2) * 3200)), inliers first or shuffled (PROSAC reads the order); two and three planes of unequal size.

Tolerances.  Nothing here is measured against the device code.  S_MAX is the largest max|H_a - H_b| / max|H_a| between the two
variants of the restatement (tests/cpp/homography_oracle.cpp: variant 1 walks the Jacobi pairs backwards and adds the LtL / JtJ sums
from the last point to the first) over every scene below, H scaled to H(2,2) = 1; tests/test_oracle_homography.py measures it again
on every run and fails when a scene exceeds the constant.  TOL_H = 64 * S_MAX covers the device's rcp / rsq + Newton arithmetic and
its different reduction tree; the project's bar for ARRSAC models is 1e-7 and TOL_H must stay below it.

A scene is admissible when both variants take the same decisions (statistics, stream positions, mask) and the closest threshold
comparison either of them made keeps margin >= 1000 * TOL_H * X / th (X: the largest absolute coordinate): a model off by TOL_H moves
a mapped point by about TOL_H * X, so three orders of headroom remain.

One more condition, found on the restatement itself: refineHomography (CvLevMarq) accepts a step iff the cost did not rise, and the last
Gauss-Newton steps that still matter (~1e-10 of H) change the cost by less than the rounding of its own sum.  In plain doubles that test
is then a coin flip; a run of rejections raises lambda until the step vanishes, the relative-change test ends the loop and H stays
~1e-10 .. 1e-9 short of the fixed point -- on about one pixel-unit scene in twenty, in either variant or in both alike (so S does not
show it).  The restatement reports the largest relative size of a step its refinement rejected (`doubt`); a scene is admissible only
with doubt <= TOL_H in both variants, i.e. when no rejected step could have moved H by more than the tolerance.  (The library's kernel
evaluates the residuals of that cost with error-free products and sums, so its own accept test is decided by the cost.)

The seeds below were picked on the CPU so that every scene is admissible; the CPU test asserts it for all of them."""
import numpy as np

S_MAX = 3.3e-13    # measured 3.231e-13 (scene n1200_gen; tests/make_homography_trace.py prints every scene's value), rounded up
TOL_H = 64 * S_MAX  # 2.112e-11

TH_PIX = 1.5
TH_CAM = 0.8 * 4 / (np.sqrt(2) * 3200)


def _units(units):
    if units == "pix":
        return 0.0, 1000.0, TH_PIX, 0.3
    return -0.5, 0.5, TH_CAM, TH_CAM / 5


def random_h(rng, units):
    lo, hi, th, _ = _units(units)
    c = 0.5 * (lo + hi)
    ang, sc = rng.uniform(-0.15, 0.15), rng.uniform(0.9, 1.1)
    A = sc * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]) + rng.uniform(-0.03, 0.03, (2, 2))
    t = np.array([c, c]) - A @ np.array([c, c]) + rng.uniform(-0.03, 0.03, 2) * (hi - lo)
    g = rng.uniform(-0.1, 0.1, 2) / (hi - lo)
    H = np.array([[A[0, 0], A[0, 1], t[0]], [A[1, 0], A[1, 1], t[1]], [g[0], g[1], 1.0]])
    return H


def apply_h(H, p):
    q = np.c_[p, np.ones(len(p))] @ H.T
    return q[:, :2] / q[:, 2:3]


def planes_scene(n, counts, seed, units="pix", shuffled=False, noise=1.0):
    """n correspondences: counts[k] noisy inliers of plane k (in this order), the rest uniform outliers.  Returns p1, p2, Hs, label
    (plane index or -1), th.  noise scales the Gaussian sigma (0.3 pixels, th / 5 in camera units)."""
    rng = np.random.default_rng(seed)
    lo, hi, th, sigma = _units(units)
    p1 = rng.uniform(lo, hi, (n, 2))
    p2 = rng.uniform(lo, hi, (n, 2))
    label = np.full(n, -1)
    Hs, at = [], 0
    for k, c in enumerate(counts):
        H = random_h(rng, units)
        p2[at:at + c] = apply_h(H, p1[at:at + c]) + rng.normal(0, sigma * noise, (c, 2))
        label[at:at + c] = k
        Hs.append(H)
        at += c
    if shuffled:
        perm = rng.permutation(n)
        p1, p2, label = p1[perm], p2[perm], label[perm]
    return np.ascontiguousarray(p1), np.ascontiguousarray(p2), Hs, label, th


# single plane: (name, n, inliers, units, shuffled, seed) -- the sizes at which the library's code takes another path
SINGLE = [
    ("n4", 4, 4, "pix", False, 1),                 # direct path
    ("n5", 5, 5, "cam", False, 1),                 # smallest ARRSAC
    ("n99", 99, 60, "pix", True, 1),               # early return
    ("n100", 100, 70, "cam", True, 1),
    ("n101", 101, 60, "pix", True, 4),             # one preemptive point
    ("n119", 119, 70, "cam", True, 21),             # sub-block edge
    ("n120", 120, 72, "pix", True, 1),
    ("n128", 128, 80, "cam", True, 1),             # head words
    ("n129", 129, 80, "pix", True, 2),
    ("n199", 199, 120, "cam", True, 1),            # first re-order
    ("n200", 200, 120, "pix", True, 1),
    ("n1023", 1023, 600, "cam", True, 2),          # flag row
    ("n1024", 1024, 500, "pix", True, 1),
    ("n1025", 1025, 700, "cam", True, 1),
    ("n5000_64", 5000, 64, "pix", False, 1),       # mask and refinement over many workgroups' worth of points
    ("n5000_65", 5000, 65, "cam", False, 1),
    ("n5000_257", 5000, 257, "pix", False, 1),
    ("n5000_half", 5000, 2500, "pix", True, 2),
    ("n1200_gen", 1200, 1164, "pix", True, 208),     # 97 % inliers: the preemptive stage generates hypotheses
    ("n1500_ext", 1500, 1485, "pix", True, 68),      # 99 %: it keeps generating and ends at correspondence 1119, past the 1024-bit rows
]
# the three scenes of tests/golden/homography_trace.npz
FIXTURE = ["n101", "n200", "n1025"]
# multi-plane: (name, n, counts, units, seed)
MULTI = [
    ("two", 600, (260, 140), "pix", 1),
    ("three", 900, (380, 220, 120), "cam", 11),
]
MULTI_NOISE = ("noise", 300, (), "pix", 3)         # no plane at all: -1 without varTh
MULTI_VARTH = ("varth", 300, (150,), "pix", 65, 5.0)   # noisy plane: no hypothesis survives at 1.5 th, the step to 2.25 th finds it


# what the multi-plane tests run: (scene, keyword arguments of mult_homographies)
MULTI_CASES = [
    ("two", dict(min_pts_per_plane=30)),
    ("two", dict(min_pts_per_plane=30, max_planes=1)),                 # maxPlanes = 1
    ("two", dict(min_pts_per_plane=180)),                              # minPtsPerPlane larger than the second plane
    ("two", dict(min_pts_per_plane=4, max_planes=2)),
    ("two", dict(min_pts_per_plane=30, var_th=False)),
    ("three", dict(min_pts_per_plane=30)),
    ("three", dict(min_pts_per_plane=30, max_planes=1)),
    ("three", dict(min_pts_per_plane=260)),
    ("three", dict(min_pts_per_plane=4, max_planes=3)),
    ("varth", dict(min_pts_per_plane=30)),                             # needs the second threshold step (2.25 th)
    ("varth", dict(min_pts_per_plane=30, var_th=False)),               # ... and fails without it: -1
    ("noise", dict(var_th=False)),                                     # pure noise: -1
]


def sample_cases():
    """Fixed index lists for the sample kernel alone: points, then {name: index list}.  The lists are planted inliers of scene n200
    (noisy, so the 12-point polish moves the model); `flat` is a 6-point list whose image-2 x-coordinates are all equal (zero spread: the
    normalisation refuses it)."""
    p1, p2, H, planted, th = single("n200")
    p2 = p2.copy()
    inl, out = np.flatnonzero(planted), np.flatnonzero(~planted)
    p2[out[:6], 0] = 412.25
    # positions in the inlier list.  LMSolver's turns on a non-minimal sample stop on float32 criteria, and near the optimum its
    # "did the step lower the cost" test is decided by rounding: on most lists two correct evaluations differ by ~1e-10 of H.  These
    # lists were picked on the CPU as ones on which 26 evaluations of the restatement (both variants, permuted point order) agree to
    # 2e-14, i.e. on which no such decision is a coin flip.
    pos = {"m4": [12, 60, 74, 75], "m4b": [7, 31, 58, 100], "m5": [5, 20, 41, 50, 67], "m6": [0, 3, 5, 51, 86, 119],
           "m11": [3, 8, 13, 19, 34, 37, 41, 43, 102, 110, 115], "m12": [5, 11, 39, 40, 55, 61, 62, 68, 72, 92, 96, 113]}
    lists = {k: inl[v] for k, v in pos.items()}
    lists["flat"] = out[:6]
    return p1, p2, {k: np.ascontiguousarray(v, np.int32) for k, v in lists.items()}


def single(name):
    for c in SINGLE:
        if c[0] == name:
            _, n, k, units, shuffled, seed = c
            p1, p2, Hs, label, th = planes_scene(n, (k,), seed, units, shuffled)
            return p1, p2, Hs[0], label == 0, th
    raise KeyError(name)


def multi(name):
    for c in MULTI + [MULTI_NOISE]:
        if c[0] == name:
            _, n, counts, units, seed = c
            return planes_scene(n, counts, seed, units, True)
    if name == "varth":
        _, n, counts, units, seed, noise = MULTI_VARTH
        return planes_scene(n, counts, seed, units, True, noise)
    raise KeyError(name)


def failing_scene(n=150):
    """Every x-coordinate of image 2 is the same: the normalisation refuses every sample, Estimate fails after 500 PROSAC turns."""
    rng = np.random.default_rng(5)
    p1 = rng.uniform(0, 1000, (n, 2))
    p2 = np.c_[np.full(n, 321.5), rng.uniform(0, 1000, n)]
    return p1, p2, TH_PIX


def max_coord(p1, p2):
    return float(max(np.abs(p1).max(), np.abs(p2).max()))


def h_dist(a, b):
    a, b = np.asarray(a, np.float64).reshape(3, 3), np.asarray(b, np.float64).reshape(3, 3)
    a, b = a / a[2, 2], b / b[2, 2]
    return float(np.abs(a - b).max() / np.abs(a).max())
