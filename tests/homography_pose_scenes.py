"""Seeded scenes for the homography-alignment tests (tests/test_oracle_homography_align.py on the CPU,
tests/test_gpu_homography_align.py on the device): several planes seen under ONE camera motion, H_k ~ R (I - t n_k^T) -- the convention
of the reference's construct_analytic_homography: a point P1 of the first camera's frame is P2 = R (P1 - t) in the second's, plane k is
n_k . P1 = 1.  Gaussian noise, uniform outliers (label -1), shuffled order.  Units: `cam` (coordinates in [-0.5, 0.5], th = TH_CAM of
tests/homography_scenes.py, sigma = th / 5), `wide` (coordinates in [-0.8, 0.8], th = 0.003) and `pix`: a camera-unit scene mapped to
pixel-like coordinates x' = 500 (x + 1) in [250, 750] with th = 1.5 and H0 mapped alike.  The function takes no camera matrix, so in
`pix` the planes' homographies are no longer R (I - t n^T) of one motion and the result is not a pose of the scene; the scene is there
for the magnitudes (1e2 .. 1e3 in the rows, 1e5 .. 1e6 in the 11 x 11 system the equilibrated LU solves), and device and restatement
must still agree on it.

Tolerances.  Nothing here is measured against the device code.  S_A is the largest of max|R_a - R_b|, max|t_a - t_b| and
max|norms_a - norms_b| between the two variants of the restatement (tests/cpp/homography_align_oracle.cpp: variant 1 adds every sum from
the last point to the first and walks the Jacobi pairs backwards) over every scene below; tests/test_oracle_homography_align.py measures
it again on every run and fails when a scene exceeds the constant.  TOL_A = 64 * S_A covers the device's different reduction tree and
division and square-root sequences (the factor TOL_H carries); the project's bar for R and t is 1e-6 and TOL_A must stay below it.

A scene is admissible when both variants take the same decisions (code, chosen q, rounds of every outer turn, every candidate choice)
and the closest stop-test comparison either of them made (|e1 - e2| against 1e-5 / 1e-6, e1 against tol), as well as the distance of
the two final motion errors the q choice compares, keep a relative margin of at least 1000 * TOL_A.  The seeds below were picked on the
CPU so that every scene is admissible; the CPU test asserts it for all of them."""
import numpy as np

from homography_scenes import TH_CAM, TH_PIX

S_A = 2.4e-11   # measured 2.299e-11 (scene pix_n110; the camera-unit and wide scenes stay below 4.0e-13, the largest of them forty at 3.974e-13;
                # tests/make_homography_align_trace.py prints every scene's value), rounded up
TOL_A = 64 * S_A  # 1.536e-9
S_CAM = 4.0e-13  # the same yardstick over the camera-unit and wide scenes alone (every scene but `pix`): they are held to 64 * S_CAM


def tol_of(units):
    return TOL_A if units == "pix" else 64 * S_CAM


def units_of(name):
    return next(c[3] for c in SCENES + GUARD + FULL + [FULL_ONE, FULL_WEAK] if c[0] == name)
PIX_MAP = np.array([[500.0, 0.0, 500.0], [0.0, 500.0, 500.0], [0.0, 0.0, 1.0]])
MARGIN = 1000 * TOL_A
TH_WIDE = 0.003


def _units(units):
    if units == "wide":
        return 0.8, TH_WIDE, TH_WIDE / 5
    return 0.5, TH_CAM, TH_CAM / 5      # (`pix` is generated in camera units and mapped afterwards)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def plane_normals(rng, P):
    """Unit normals tilted 28 deg .. 38 deg off the optical axis at azimuths 360 / P apart (P <= 3: pairwise angle >= 30 deg); further
    planes get smaller tilts in between."""
    az0 = rng.uniform(0, 2 * np.pi)
    out = []
    for k in range(P):
        tilt = np.deg2rad(rng.uniform(28, 38)) if k < 3 else np.deg2rad(rng.uniform(8, 14))
        az = az0 + 2 * np.pi * (k % 3) / 3 + (0.9 if k >= 3 else 0.0) * (k - 2)
        out.append(np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)]))
    return out


def pose_scene(counts, n_out, seed, units="cam", noise=1.0, shuffled=True, h0_jitter=1e-3):
    """counts[k] correspondences on plane k plus n_out uniform outliers.  Returns a dict: p1, p2, labels (int32, plane or -1), P,
    num_inl, R, t (planted: P2 = R (P1 - t)), normals n_k (n_k . P1 = 1), Hs (planted, H(2,2) = 1), H0 (plane 0's homography with a
    relative jitter, the stand-in for the robust estimate), th."""
    rng = np.random.default_rng(seed)
    half, th, sigma = _units(units)
    P = len(counts)
    R = rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(2.0, 7.0)))
    depth = rng.uniform(4.0, 7.0, P)
    tdir = rng.normal(size=3)
    tdir[2] *= 0.3
    tdir /= np.linalg.norm(tdir)
    t = tdir * rng.uniform(0.12, 0.2) * depth.min()
    normals = [m / (d * m[2]) for m, d in zip(plane_normals(rng, P), depth)]   # depth d on the optical axis
    p1s, p2s, labels, Hs = [], [], [], []
    for k, c in enumerate(counts):
        x = rng.uniform(-half, half, (c, 2))
        ray = np.c_[x, np.ones(c)]
        z = 1.0 / (ray @ normals[k])
        assert (z > 0).all()
        P2 = (ray * z[:, None] - t) @ R.T
        assert (P2[:, 2] > 0).all()
        p1s.append(x)
        p2s.append(P2[:, :2] / P2[:, 2:3] + rng.normal(0, sigma * noise, (c, 2)))
        labels.append(np.full(c, k))
        H = R @ (np.eye(3) - np.outer(t, normals[k]))
        Hs.append(H / H[2, 2])
    if n_out:
        p1s.append(rng.uniform(-half, half, (n_out, 2)))
        p2s.append(rng.uniform(-half, half, (n_out, 2)))
        labels.append(np.full(n_out, -1))
    p1, p2, labels = np.concatenate(p1s), np.concatenate(p2s), np.concatenate(labels)
    if shuffled:
        perm = rng.permutation(len(p1))
        p1, p2, labels = p1[perm], p2[perm], labels[perm]
    H0 = Hs[0] * (1 + h0_jitter * rng.normal(size=(3, 3)))
    H0 = H0 / H0[2, 2]
    if units == "pix":
        to_pix = lambda p: (np.c_[p, np.ones(len(p))] @ PIX_MAP.T)[:, :2]
        p1, p2, th = to_pix(p1), to_pix(p2), TH_PIX
        H0 = PIX_MAP @ H0 @ np.linalg.inv(PIX_MAP)
        H0 = H0 / H0[2, 2]
        Hs = [PIX_MAP @ H @ np.linalg.inv(PIX_MAP) for H in Hs]
    return {"p1": np.ascontiguousarray(p1), "p2": np.ascontiguousarray(p2), "labels": np.ascontiguousarray(labels, np.int32), "P": P,
            "num_inl": np.array(counts, np.int32), "R": R, "t": t, "normals": np.array(normals), "Hs": np.array(Hs), "H0": H0, "th": th}


# (name, counts, outliers, units, noise, seed): the shapes at which the library's kernel takes another path
SCENES = [
    ("p2_n38", (15, 15), 8, "cam", 1.0, 30),                # below one wave per plane, ragged
    ("p2_n63", (40, 23), 0, "cam", 1.0, 30),                # one short of a wave
    ("p2_n65", (48, 17), 0, "wide", 1.0, 35),               # one over a wave
    ("p3_n900", (380, 220, 120), 180, "cam", 1.0, 69),      # crosses the block stride
    ("p5_n75", (15, 15, 15, 15, 15), 0, "cam", 1.0, 57),    # the per-plane tables
    ("p2_n4100", (3000, 1100), 0, "wide", 1.0, 30),         # points no longer fit the cached path
    ("exact", (60, 40), 10, "cam", 0.0, 35),                # noise-free: stops on e1 < tol
    ("slow", (60, 40), 0, "wide", 6.0, 30),                 # noise above the threshold: e1 stays above tol, the |e1 - e2| test ends the rounds
    ("forty", (15, 15, 15, 15, 15), 0, "wide", 8.0, 2006),  # ... and here it does not: all 40 rounds of every turn of q = 0
    ("pix_n110", (60, 40), 10, "pix", 1.0, 105),            # pixel-like magnitudes in the 11 x 11 system
]
FIXTURE = ["p2_n38", "p3_n900", "exact"]
# noise-free scenes with well separated normals and a baseline of at least 10 % of the depth, for the convention guard
GUARD = [("guard2", (80, 60), 0, "cam", 0.0, 30), ("guard3", (80, 60, 50), 0, "wide", 0.0, 69)]


# the whole function (plane search included): (name, counts, outliers, units, noise, seed).  Admissible as above, and as
# tests/homography_scenes.py asks of the plane search (equal statistics and stream positions in both variants, margin, doubt <= TOL_H);
# the closest `err < th^2` of the final mask keeps a relative margin of at least FULL_MARGIN.
FULL = [
    ("full_two", (150, 90), 60, "cam", 1.0, 30),
    ("full_three", (200, 120, 80), 100, "cam", 1.0, 229),
    ("full_wide", (150, 90), 60, "wide", 1.0, 13),
]
FULL_ONE = ("full_one", (150,), 60, "cam", 1.0, 30)          # one plane: -3
FULL_WEAK = ("full_weak", (90, 45), 165, "cam", 1.0, 30)     # planes too weak (strengths sum to less than 0.5): -2 with checkPlaneStrength
FULL_MARGIN = 1e-3


def full_scene(name):
    for c in FULL + [FULL_ONE, FULL_WEAK]:
        if c[0] == name:
            _, counts, n_out, units, noise, seed = c
            return pose_scene(counts, n_out, seed, units, noise)
    raise KeyError(name)


def full_mask(n):
    """The input mask of the mask-path tests: every fifth row dropped."""
    m = np.ones(n, np.uint8)
    m[::5] = 0
    return m


def noise_scene(n=300, seed=3):
    """No plane at all: -1 (without varTh)."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-0.5, 0.5, (n, 2))), np.ascontiguousarray(rng.uniform(-0.5, 0.5, (n, 2))), TH_CAM


def scene(name):
    for c in SCENES + GUARD:
        if c[0] == name:
            _, counts, n_out, units, noise, seed = c
            return pose_scene(counts, n_out, seed, units, noise, h0_jitter=0.0 if noise == 0.0 else 1e-3)
    raise KeyError(name)


def angle_deg_rot(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.rad2deg(np.arccos(np.clip(c, -1, 1))))


def angle_deg_vec(a, b):
    c = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.rad2deg(np.arccos(np.clip(c, -1, 1))))


def variant_distance(a, b):
    return float(max(np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max(), np.abs(a["norms"] - b["norms"]).max()))


def same_decisions(a, b):
    return (a["code"] == b["code"] and a["q"] == b["q"] and (a["rounds"] == b["rounds"]).all() and a["choices"] == b["choices"]
            and a["reason"] == b["reason"])
