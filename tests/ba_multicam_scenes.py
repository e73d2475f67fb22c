"""Seeded scenes for the multi-camera bundle-adjustment tests, and the tolerances the device is held to.

A scene, built like ba_scenes.make_scene: 3-D points 4 .. 20 deep in front of camera 0; m cameras on an arc of radius 10 about the middle of
the cloud, all facing it, neighbours about one unit apart (the arc is capped at 40 degrees, so 16 cameras stand closer); projections with image
noise of 0.3 px at ba_scenes.K; 15 % of every free camera's measurements are gross outliers (a random image point) that STAY visible; the
start is every free camera's true pose turned by `rot_err_deg` and shifted, and the true points scaled by a few per cent.  Camera 0 keeps its
true pose: it is the gauge.  `world` moves the whole scene rigidly, so that camera 0 stands at a general pose."""
import zlib

import numpy as np

import ba_multicam_oracle as BMO
import ba_scenes as BAS

K = BAS.K
ANGLE_THRESH, T_NORM_THRESH = BAS.ANGLE_THRESH, BAS.T_NORM_THRESH
NOISE_PX, OUTLIER_FRAC = BAS.NOISE_PX, BAS.OUTLIER_FRAC
N_PERMUTATIONS = 20


def threshold(m):
    return BMO.convert_threshold_multicam([K] * m)


# ---- visibility patterns: (rng, m, n) -> bool [m, n] ----------------------------------------------------------------------------------------------
def _at_least_two(rng, vis):
    for i in np.flatnonzero(vis.sum(axis=0) < 2):
        vis[rng.permutation(vis.shape[0])[:2], i] = True
    return vis


def vis_all(rng, m, n):
    return np.ones((m, n), bool)


def vis_frac(frac):
    return lambda rng, m, n: _at_least_two(rng, rng.random((m, n)) < frac)


def vis_exactly_two(rng, m, n):
    vis = np.zeros((m, n), bool)
    for i in range(n):
        vis[rng.permutation(m)[:2], i] = True
    return vis


def vis_sparse_cam(rng, m, n):
    """The last camera sees 7 points."""
    vis = np.zeros((m, n), bool)
    vis[:m - 1] = _at_least_two(rng, rng.random((m - 1, n)) < 0.7)
    vis[m - 1, np.sort(rng.permutation(n)[:7])] = True
    return vis


def vis_disjoint_1_3(rng, m, n):
    """Cameras 1 and 3 share no point."""
    vis = rng.random((m, n)) < 0.7
    side = rng.random(n) < 0.5
    vis[1, side] = False
    vis[3, ~side] = False
    others = [j for j in range(m) if j not in (1, 3)]
    for i in np.flatnonzero(vis.sum(axis=0) < 2):
        vis[rng.permutation(others)[:2], i] = True
    return vis


UNSEEN_ROW, CAM0_ONLY_ROW = 17, 40


def vis_unseen(rng, m, n):
    vis = _at_least_two(rng, rng.random((m, n)) < 0.7)
    vis[:, UNSEEN_ROW] = False
    vis[:, CAM0_ONLY_ROW] = False
    vis[0, CAM0_ONLY_ROW] = True
    return vis


# name -> dict(m, n, seed, vis, and what differs from the defaults of make_scene)
SCENES = {
    "m2_full_n65": dict(m=2, n=65, seed=1, vis=vis_all),
    "m3_n15_short": dict(m=3, n=15, seed=2, vis=vis_exactly_two),          # nobs = 60 < nvars = 63: the optimiser refuses
    "m3_n64": dict(m=3, n=64, seed=3, vis=vis_frac(0.7)),
    "m4_n257": dict(m=4, n=257, seed=4, vis=vis_frac(0.6)),
    "m5_sparse_cam": dict(m=5, n=300, seed=5, vis=vis_sparse_cam),
    "m5_disjoint": dict(m=5, n=200, seed=6, vis=vis_disjoint_1_3),
    "m8_n1000": dict(m=8, n=1000, seed=7, vis=vis_frac(0.5)),
    "m16_n128": dict(m=16, n=128, seed=8, vis=vis_frac(0.4)),
    "unseen_point": dict(m=3, n=80, seed=9, vis=vis_unseen),
    "rejected": dict(m=4, n=257, seed=10, vis=vis_frac(0.6), start_off=(2, 30.0)),     # camera 2 starts 30 degrees off
    "cam0_not_identity": dict(m=3, n=100, seed=11, vis=vis_frac(0.7), world=True),
}
REFUSED = ("m3_n15_short", "rejected")         # every input comes back bit for bit

# The device differs from ba_multicam_oracle only in the association of its sums.  Each row: pose (R, t absolute), q (Q absolute), info
# (info[0..1] relative), mu (at exit, relative) = 50 x the largest spread that N_PERMUTATIONS seeded permutations of the point order produce
# in the oracle itself on THAT scene (test_oracle_ba_multicam.py recomputes the spread and asserts 10 x spread <= constant <= 100 x spread);
# the measured spreads stand behind each row in that order.  One row per scene: the reduced camera system's conditioning differs widely between
# two cameras with full visibility and sixteen with sparse visibility.  0 = bit for bit (a refused scene returns its inputs and a zero info).
TOL = {
    "m2_full_n65": (1.4e-15, 2.2e-14, 3.3e-14, 3.5e-10),                      # 2.78e-17, 4.44e-16, 6.67e-16, 6.94e-12
    "m3_n15_short": (0.0, 0.0, 0.0, 0.0),                                     # refused by the optimiser: 0, 0, 0, 0
    "m3_n64": (1.1e-14, 1.1e-14, 8.2e-14, 5.6e-10),                           # 2.22e-16, 2.22e-16, 1.65e-15, 1.13e-11
    "m4_n257": (2.2e-14, 8.9e-14, 5.3e-14, 4.0e-10),                          # 4.44e-16, 1.78e-15, 1.06e-15, 7.97e-12
    "m5_sparse_cam": (2.4e-14, 4.4e-14, 5.0e-14, 3.0e-10),                    # 4.72e-16, 8.88e-16, 9.99e-16, 6.00e-12
    "m5_disjoint": (1.3e-14, 4.4e-14, 4.6e-14, 1.3e-10),                      # 2.52e-16, 8.88e-16, 9.20e-16, 2.55e-12
    "m8_n1000": (1.1e-14, 8.9e-14, 7.2e-14, 3.3e-10),                         # 2.22e-16, 1.78e-15, 1.44e-15, 6.69e-12
    "m16_n128": (1.2e-14, 4.4e-14, 4.0e-14, 2.4e-10),                         # 2.43e-16, 8.88e-16, 8.09e-16, 4.87e-12
    "unseen_point": (2.3e-14, 2.2e-14, 1.5e-13, 1.4e-9),                      # 4.58e-16, 4.44e-16, 3.05e-15, 2.75e-11
    "rejected": (0.0, 0.0, 3.0e-14, 1.9e-11),                                 # -, -, 6.03e-16, 3.85e-13
    "cam0_not_identity": (5.5e-15, 4.4e-14, 2.0e-14, 2.1e-10),                # 1.11e-16, 8.88e-16, 4.08e-16, 4.15e-12
}


def tol(name):
    return dict(zip(("pose", "q", "info", "mu"), TOL[name]))


def make_scene(m, n, seed, vis, rot_err_deg=0.3, noise_px=NOISE_PX, outlier_frac=OUTLIER_FRAC, point_err=0.03, t_err=0.01, start_off=None,
               world=False, th=None):
    rng = np.random.default_rng(20261021 + seed)
    z = rng.uniform(4, 20, n)
    X = np.stack([rng.uniform(-0.35, 0.35, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], axis=1)
    centre = np.array([0.0, 0.0, 10.0])
    step = min(np.rad2deg(0.1), 40.0 / (m - 1))
    R_true, t_true = np.zeros((m, 3, 3)), np.zeros((m, 3))
    for j in range(m):
        Rc = BAS._rot((0, 1, 0), j * step) @ (BAS._rot((1, 0, 0), rng.uniform(-2, 2)) if j else np.eye(3))
        c = centre - Rc @ np.array([0.0, 0.0, 10.0])
        R_true[j] = Rc.T
        t_true[j] = -Rc.T @ c
    if world:          # the same scene seen from a general frame: X' = G X + g
        G, g = BAS._rot((0.3, -0.5, 0.8), 25.0), np.array([0.4, -0.2, 0.7])
        X = X @ G.T + g
        for j in range(m):
            R_true[j] = R_true[j] @ G.T
            t_true[j] = t_true[j] - R_true[j] @ g
    v = vis(rng, m, n)
    sigma = noise_px / K[0, 0]
    p = np.zeros((m, n, 2))
    for j in range(m):
        Xc = X @ R_true[j].T + t_true[j]
        assert Xc[:, 2].min() > 1.0
        p[j] = Xc[:, :2] / Xc[:, 2:3] + rng.normal(0, sigma, (n, 2))
        if j:
            seen = np.flatnonzero(v[j])
            out = seen[rng.permutation(seen.size)[:int(round(outlier_frac * seen.size))]]
            p[j, out] = np.stack([rng.uniform(-0.35, 0.35, out.size), rng.uniform(-0.3, 0.3, out.size)], axis=1)
    R, t = R_true.copy(), t_true.copy()
    for j in range(1, m):
        R[j] = BAS._rot(rng.normal(size=3), rot_err_deg) @ R_true[j]
        t[j] = t_true[j] + rng.normal(0, t_err, 3)
    if start_off is not None:
        R[start_off[0]] = BAS._rot(rng.normal(size=3), start_off[1]) @ R_true[start_off[0]]
    cam0 = -R_true[0].T @ t_true[0]
    Q = cam0 + (X - cam0) * (1.0 + rng.normal(0, point_err, (n, 1)))
    return dict(p=np.ascontiguousarray(p), vis=np.ascontiguousarray(v.astype(np.uint8)), R=R, t=t, Q=np.ascontiguousarray(Q),
                th=threshold(m) if th is None else th, R_true=R_true, t_true=t_true, X=X, m=m, n=n)


_scenes, _results, _spread = {}, {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = make_scene(**SCENES[name])
    return _scenes[name]


def run_oracle(s, perm=None):
    """ba_multicam_oracle on a scene, optionally with the POINTS permuted (the result's Q comes back in the scene's own order)."""
    if perm is None:
        return BMO.ba_multicam_oracle(s["p"], s["vis"], s["R"], s["t"], s["Q"], s["th"], ANGLE_THRESH, T_NORM_THRESH)
    o = BMO.ba_multicam_oracle(s["p"][:, perm], s["vis"][:, perm], s["R"], s["t"], s["Q"][perm], s["th"], ANGLE_THRESH, T_NORM_THRESH)
    Q = np.empty_like(o["Q"])
    Q[perm] = o["Q"]
    o["Q"] = Q
    return o


def oracle_result(name):
    """Computed once per session and shared; callers must not modify it."""
    if name not in _results:
        _results[name] = run_oracle(scene(name))
    return _results[name]


integers = BAS.integers
rel_diff = BAS.rel_diff

# ---- the stereo scenes of ba_scenes.BRANCH_SCENES as two-camera problems: they reach every exit of the optimiser, which SCENES above do not -------
_two_cam, _two_cam_results = {}, {}


def two_camera(name):
    """Scene `name` of ba_scenes.BRANCH_SCENES as this entry's arguments: the rows outside the mask dropped, camera 0 at the identity, every
    point seen by both cameras, the scene's own thresholds."""
    if name not in _two_cam:
        s = BAS.scene(name)
        keep = slice(None) if s["mask"] is None else s["mask"] != 0
        p = np.ascontiguousarray(np.stack([s["p1"][keep], s["p2"][keep]]))
        _two_cam[name] = dict(p=p, vis=np.ones(p.shape[:2], np.uint8), R=np.stack([np.eye(3), s["R"]]), t=np.stack([np.zeros(3), s["t"]]),
                              Q=np.ascontiguousarray(s["Q"][keep]), th=s["th"], angle_thresh=s["angle_thresh"], t_norm_thresh=s["t_norm_thresh"],
                              m=2, n=p.shape[1])
    return _two_cam[name]


def two_camera_oracle_result(name):
    """ba_multicam_oracle on two_camera(name).  Computed once per session and shared; callers must not modify it."""
    if name not in _two_cam_results:
        s = two_camera(name)
        with np.errstate(all="ignore"):        # the stop-6 and stop-7 scenes overflow or divide by zero on purpose
            _two_cam_results[name] = BMO.ba_multicam_oracle(s["p"], s["vis"], s["R"], s["t"], s["Q"], s["th"], s["angle_thresh"], s["t_norm_thresh"])
    return _two_cam_results[name]


def compacted(s):
    """The facade's arguments: ps[j] = camera j's observations in ascending point order, map3D[j] = int8 [n]."""
    vis = s["vis"].astype(bool)
    return [np.ascontiguousarray(s["p"][j][vis[j]]) for j in range(s["m"])], [s["vis"][j].astype(np.int8) for j in range(s["m"])]


def spread(name):
    """-> dict(pose, q, info, mu, stable) of one scene: the largest difference between the oracle on the scene and on N_PERMUTATIONS seeded
    permutations of its points; stable = every permutation gave the scene's own verdict, iteration count, stop reason and counts.  The
    permutations are seeded by the scene's name."""
    if name not in _spread:
        s, o = scene(name), oracle_result(name)
        sp = dict(pose=0.0, q=0.0, info=0.0, mu=0.0, stable=True)
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        for _ in range(N_PERMUTATIONS):
            r = run_oracle(s, rng.permutation(s["n"]))
            if integers(r) != integers(o):
                sp["stable"] = False
                continue
            sp["pose"] = max(sp["pose"], np.abs(r["R"] - o["R"]).max(), np.abs(r["t"] - o["t"]).max())
            sp["q"] = max(sp["q"], np.abs(r["Q"] - o["Q"]).max())
            sp["info"] = max(sp["info"], rel_diff(r["info"][0], o["info"][0]), rel_diff(r["info"][1], o["info"][1]))
            sp["mu"] = max(sp["mu"], rel_diff(r["mu"], o["mu"]))
        _spread[name] = sp
    return _spread[name]
