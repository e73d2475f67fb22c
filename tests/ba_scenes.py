"""Seeded scenes for the bundle-adjustment tests, and the tolerances the device is held to.

A scene: 3-D points 4 .. 20 deep in front of both cameras, projected with image noise of 0.3 px at K = diag(700, 700, 1), principal point
(320, 240); 15 % of the valid rows are gross outliers (a random second-view point) that STAY in the mask; the start is the true pose turned by
`rot_err_deg` and shifted, and the true points scaled by a few per cent.  `rows` > n_valid adds rows outside the mask (garbage measurements and
points that must come back untouched).

Two tables: SCENES, six runs of that one geometry sharing four tolerances, and BRANCH_SCENES, one scene per exit of the optimiser, branch of
the wrapper and edge size, each with its own thresholds, expectations and tolerances."""
import zlib

import numpy as np

import ba_oracle as BAO

K = np.array([[700.0, 0.0, 320.0], [0.0, 700.0, 240.0], [0.0, 0.0, 1.0]])
TH = BAO.convert_threshold(K, K)            # the facade's conversion of the default Huber threshold
ANGLE_THRESH, T_NORM_THRESH = 1.25, 0.05
NOISE_PX, OUTLIER_FRAC = 0.3, 0.15

# name -> (n_valid, rows, seed, rot_err_deg); n_valid walks the kernel's boundaries: fewer points than unknowns allow (7: the optimiser
# refuses), one wave full / one over (64, 65), one over the workgroup (257), several points per lane behind a mask (1000 of 1650)
SCENES = {
    "n7": (7, 7, 11, 0.3),
    "n64": (64, 64, 12, 0.3),
    "n65": (65, 65, 13, 0.3),
    "n257": (257, 257, 14, 0.3),
    "n1000_masked": (1000, 1650, 15, 0.3),
    "rejected": (257, 257, 17, 30.0),       # a start far beyond ANGLE_THRESH: the optimiser turns it by about 1.6 degrees and is refused
}

# The device differs from ba_oracle only in the association of its sums.  These are 10 x the largest spread that 20 seeded permutations of
# the point order produce in ba_oracle itself over the scenes above (test_oracle_bundle_adjust.py recomputes the spread and asserts
# 10 x spread <= constant <= 100 x spread): R, t absolute; Q absolute; info[0..1] relative; mu at exit relative.
TOL_POSE = 2.5e-15     # measured spread 2.2e-16
TOL_Q = 2e-14          # 1.8e-15
TOL_INFO = 1.5e-14     # 1.4e-15
TOL_MU = 1e-10         # 8.6e-12
N_PERMUTATIONS = 20


def _rot(axis, deg):
    axis = np.asarray(axis, float)
    axis = axis / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def make_scene(n_valid, rows=None, seed=0, rot_err_deg=0.3, noise_px=NOISE_PX, outlier_frac=OUTLIER_FRAC, point_err=0.03,
               rot_axis=(0.2, 0.9, 0.1), rot_deg=5.0, t_true=None, t_err=0.01, start_rot_deg=None, t_scale=None, q_rows=None, th=TH):
    """The defaults give the scenes of SCENES byte for byte.  rot_axis, rot_deg: the true rotation; t_true: the true translation as it is (NOT
    normalised while the points are placed: two cameras that face each other need a baseline longer than the points are deep; the scene is
    brought to a unit baseline afterwards); t_err: sigma of the start's translation
    error; start_rot_deg: the start rotation is this angle about rot_axis instead of the truth turned by rot_err_deg; t_scale: the start
    translation is multiplied by it AFTER its normalisation; q_rows: {row: f(p1_row, Q_row) -> the start point of that row}."""
    rows = n_valid if rows is None else rows
    rng = np.random.default_rng(20261019 + seed)
    R_true = _rot(rot_axis, rot_deg)
    custom_baseline = t_true is not None
    if t_true is None:
        t_true = np.array([1.0, 0.05, -0.02])
        t_true = t_true / np.linalg.norm(t_true)
    else:
        t_true = np.array(t_true, float)
    z = rng.uniform(4, 20, rows)
    X = np.stack([rng.uniform(-0.35, 0.35, rows) * z, rng.uniform(-0.3, 0.3, rows) * z, z], axis=1)
    X2 = X @ R_true.T + t_true
    assert X2[:, 2].min() > 1.0
    sigma = noise_px / K[0, 0]
    p1 = X[:, :2] / X[:, 2:3] + rng.normal(0, sigma, (rows, 2))
    p2 = X2[:, :2] / X2[:, 2:3] + rng.normal(0, sigma, (rows, 2))
    if custom_baseline:           # the gauge: the depths above are in units of the points, the pose carries a unit translation
        X, t_true = X / np.linalg.norm(t_true), t_true / np.linalg.norm(t_true)
    mask = np.zeros(rows, np.uint8)
    valid = np.sort(rng.permutation(rows)[:n_valid])
    mask[valid] = np.where(rng.random(n_valid) < 0.5, 1, 255)
    out = valid[rng.permutation(n_valid)[:int(round(outlier_frac * n_valid))]]
    p2[out] = np.stack([rng.uniform(-0.35, 0.35, out.size), rng.uniform(-0.3, 0.3, out.size)], axis=1)
    R = _rot(rng.normal(size=3), rot_err_deg) @ R_true
    if start_rot_deg is not None:
        R = _rot(rot_axis, start_rot_deg)
    t = t_true + rng.normal(0, 0.01, 3) * (t_err / 0.01)
    t = t / np.linalg.norm(t)
    if t_scale is not None:
        t = t * t_scale
    Q = X * (1.0 + rng.normal(0, point_err, (rows, 1)))
    for row, f in (q_rows or {}).items():
        Q[row] = f(p1[row], Q[row])
    return dict(p1=np.ascontiguousarray(p1), p2=np.ascontiguousarray(p2), R=R, t=t, Q=np.ascontiguousarray(Q),
                mask=None if rows == n_valid else mask, th=th, R_true=R_true, t_true=t_true, X=X)


# The family that the optimiser's rarer exits were searched in (seeds 0 .. 1999, on ba_oracle alone): the seed picks n, then one of six
# (rot_err_deg, noise_px, outlier_frac, point_err), then the Huber threshold, in mixed radix, and seeds the scene's random numbers.
FAMILY_N = (12, 16, 30, 64, 100)
FAMILY_SETTINGS = ((0.3, 0.3, 0.15, 0.03), (1.0, 1.0, 0.3, 0.1), (3.0, 3.0, 0.5, 0.3), (0.3, 0.0, 0.0, 0.03), (10.0, 3.0, 0.5, 1.0),
                   (30.0, 0.3, 0.15, 0.5))
FAMILY_TH = (TH, 1.0, 1e-2, 1e-8)


def family_scene(seed):
    rot, noise, outl, perr = FAMILY_SETTINGS[(seed // 5) % 6]
    return make_scene(FAMILY_N[seed % 5], seed=seed, rot_err_deg=rot, noise_px=noise, outlier_frac=outl, point_err=perr,
                      th=FAMILY_TH[(seed // 30) % 4])


_scenes, _results = {}, {}


def scene(name):
    if name not in _scenes:
        if name in SCENES:
            n_valid, rows, seed, rot = SCENES[name]
            _scenes[name] = make_scene(n_valid, rows, seed, rot)
        else:
            row = BRANCH_SCENES[name]
            _scenes[name] = dict(row["build"](), angle_thresh=row.get("angle_thresh", ANGLE_THRESH), t_norm_thresh=row.get("t_norm_thresh", T_NORM_THRESH))
    return _scenes[name]


def run_oracle(s, perm=None):
    """ba_oracle on a scene, optionally with the ROWS permuted (the result's Q comes back in the scene's own order)."""
    at, tt = s.get("angle_thresh", ANGLE_THRESH), s.get("t_norm_thresh", T_NORM_THRESH)       # a scene of BRANCH_SCENES may carry its own
    if perm is None:
        return BAO.ba_oracle(s["p1"], s["p2"], s["R"], s["t"], s["Q"], s["th"], s["mask"], at, tt)
    m = None if s["mask"] is None else s["mask"][perm]
    o = BAO.ba_oracle(s["p1"][perm], s["p2"][perm], s["R"], s["t"], s["Q"][perm], s["th"], m, at, tt)
    Q = np.empty_like(o["Q"])
    Q[perm] = o["Q"]
    o["Q"] = Q
    return o


def oracle_result(name):
    """Computed once per session and shared; callers must not modify it."""
    if name not in _results:
        _results[name] = run_oracle(scene(name))
    return _results[name]


def integers(o):
    return (bool(o["accepted"]), int(o["info"][5]), int(o["info"][6]), int(o["info"][7]), int(o["info"][8]), int(o["info"][9]))


_spread = {}


def permutation_spread():
    """-> dict(pose, q, info, mu, stable): the largest difference between ba_oracle on a scene and on N_PERMUTATIONS seeded permutations of its
    rows, over every scene; stable = every permutation gave the scene's own verdict, iteration count, stop reason and counts."""
    if not _spread:
        sp = dict(pose=0.0, q=0.0, info=0.0, mu=0.0, stable=True)
        for k, name in enumerate(SCENES):
            s, o = scene(name), oracle_result(name)
            rng = np.random.default_rng(1000 + k)
            for _ in range(N_PERMUTATIONS):
                perm = rng.permutation(s["p1"].shape[0])
                r = run_oracle(s, perm)
                if integers(r) != integers(o):
                    sp["stable"] = False
                    continue
                sp["pose"] = max(sp["pose"], np.abs(r["R"] - o["R"]).max(), np.abs(r["t"] - o["t"]).max())
                sp["q"] = max(sp["q"], np.abs(r["Q"] - o["Q"]).max())
                for i in (0, 1):
                    if o["info"][i] != 0:
                        sp["info"] = max(sp["info"], abs(r["info"][i] - o["info"][i]) / abs(o["info"][i]))
                if o["mu"] != 0:
                    sp["mu"] = max(sp["mu"], abs(r["mu"] - o["mu"]) / abs(o["mu"]))
        _spread.update(sp)
    return _spread


# ---- one scene per exit of the optimiser, branch of the wrapper and edge size ------------------------------------------------------------------
def _exact(n, seed, **kw):
    """Noise-free measurements; with rot_err_deg = t_err = point_err = 0 the start is the truth."""
    return make_scene(n, seed=seed, noise_px=0.0, outlier_frac=0.0, th=1.0, **kw)


def _plant(n, seed, row, f):
    return make_scene(n, seed=seed, q_rows={row: f})


def _shrunk(n, seed, scale):
    """The whole scene at another scale: |t| = scale and the points with it."""
    return make_scene(n, seed=seed, t_scale=scale, q_rows={r: (lambda p, q: q * scale) for r in range(n)})


PLANTED_ROW = 30        # of 64: valid points before and after it
FACING = (0.5, 0.2, 30.0)   # the baseline of two cameras that face each other over points 4 .. 20 deep (rotations about x and y)

# name -> build: the scene; kind: "accepted" (R, t, Q, info[0..1], mu to tol), "refused" (R, t, Q byte for byte the inputs; info[0..4], mu to
# tol; entries that are not finite in the oracle must be not finite on the device); expect: what test_oracle_bundle_adjust.py finds in the
# oracle's run (stop, verdict, and the branch the scene is named for); tol: (pose, q, info, mu) from the spread over N_PERMUTATIONS
# permutations of THIS scene by the rule below; the measured spreads stand behind each row in that order; 0 = bit for bit.  Every scene keeps
# all six integers under all permutations, the 150-iteration one included (family seed 170; seed 58, n = 64, is a second one), so none
# is held to fewer than six.  The spread is the largest of 20 draws and moves with the draw (stop5_exact: 1.5e-15 .. 1.5e-13 in R between
# two seeds of the permutations); branch_spread seeds the draw by the scene's name, so the figures below are reproducible row by row.
BRANCH_SCENES = {}


def _add(name, build, kind, expect, tol, **thresholds):
    BRANCH_SCENES[name] = dict(build=build, kind=kind, expect=expect, tol=dict(zip(("pose", "q", "info", "mu"), tol)), **thresholds)


# The rule for tol: 10 x the largest spread of the scene's own study (written with a little headroom: 12 x the figure behind it).  One
# exception, a rule fixed before any device figure was seen: an entry of R or t is at most 1 in size and an entry of Q at most 32 (0.67 in the
# two facing-camera scenes, 0.01 in t_tiny_kept), so ONE rounding of such an entry going the other way costs 1.1e-16 resp. 3.6e-15
# (1.1e-16, 1.7e-18); where 20 permutations happened to contain no such event the spread is that of the small entries alone, and 10 x it
# would demand the large ones bit for bit.  Where 10 x the spread lies below four such roundings the constant is about 90 x the spread
# instead (the test allows 10 x .. 100 x).  A spread of exactly 0 stays 0: those scenes' steps are too small to reach the last bit (mu is
# huge, or the start is the truth), on the device as in the oracle.
# the five normal exits
_add("stop1_at_truth", lambda: _exact(64, 1, rot_err_deg=0.0, t_err=0.0, point_err=0.0), "accepted",
     dict(stop=1, accepted=True, itno=0, t_case="kept_unit"), (0, 0, 0, 0))                      # spread 0, 0, 0, 0: e is exactly 0
_add("stop5_exact", lambda: _exact(120, 5), "accepted", dict(stop=5, accepted=True),
     (1.9e-14, 2.8e-12, 9.6e-15, 1.5e-14))                                                         # 1.55e-15, 2.31e-13, 8.00e-16, 1.23e-15
_add("stop2_rejected8_n12", lambda: family_scene(360), "accepted", dict(stop=2, accepted=True, min_rejected=8),
     (6.2e-16, 0, 2e-15, 4.5e-14))                                                                 # 6.94e-18 (90 x), 0, 1.63e-16, 3.75e-15
_add("stop4_refused_solves", lambda: family_scene(158), "accepted", dict(stop=4, accepted=True, min_refused_solves=1, min_rejected=2),
     (2.6e-12, 5.7e-10, 1e-11, 3e-11), angle_thresh=180.0, t_norm_thresh=10.0)                     # 2.17e-13, 4.71e-11, 8.52e-13, 2.52e-12
_add("stop3_n12", lambda: family_scene(170), "refused",
     dict(stop=3, accepted=False, itno=150, min_refused_solves=1, min_rejected=2, refused_by=("angle", "t_norm")),
     (0, 0, 1.3e-6, 5.7e-7))                                                                       # -, -, 1.06e-7, 4.77e-8
# the two exits that make the wrapper refuse, at the start and in mid-run
_add("stop7_start_z0", lambda: _plant(64, 23, PLANTED_ROW, lambda p, q: np.array([q[0], q[1], 0.0])), "refused",
     dict(stop=7, accepted=False, itno=0), (0, 0, 0, 0))
_add("stop7_start_nan", lambda: _plant(64, 23, PLANTED_ROW, lambda p, q: np.array([q[0], np.nan, q[2]])), "refused",
     dict(stop=7, accepted=False, itno=0), (0, 0, 0, 0))
_add("stop7_midrun_12", lambda: family_scene(155), "refused", dict(stop=7, accepted=False, itno=12),
     (0, 0, 6e-11, 2.7e-11))                                                                       # -, -, 4.99e-12, 2.23e-12
_add("stop7_midrun_32", lambda: family_scene(161), "refused", dict(stop=7, accepted=False, itno=32),
     (0, 0, 3.9e-10, 7.5e-13))                                                                     # -, -, 3.22e-11, 6.29e-14
# one V*_i whose determinant overflows: the first attempts fail at the planted point, and once mu^3 overflows too, at point 0; 30 doublings
_add("stop6_first_bad", lambda: _plant(64, 24, PLANTED_ROW, lambda p, q: np.array([p[0], p[1], 1.0]) * 1e-52), "refused",
     dict(stop=6, accepted=False, itno=1, first_bad=PLANTED_ROW, refused_by=("stop",)), (0, 0, 9.6e-15, 0))     # -, -, 8.02e-16, 0
# the same with V_i's own diagonal overflowing: mu = inf from the start, every attempt fails at point 0, info[4] = inf / inf
_add("stop6_first_bad_inf", lambda: _plant(64, 24, PLANTED_ROW, lambda p, q: np.array([p[0], p[1], 1.0]) * 1e-160), "refused",
     dict(stop=6, accepted=False, itno=1, first_bad=0, refused_by=("stop",)), (0, 0, 9.6e-15, 0))               # -, -, 8.02e-16, 0
# the wrapper: MatToQuat's pivots and the two sign fixes, the three cases of |t|, the rejection rules
_add("pivot0_x175", lambda: make_scene(64, seed=20, rot_axis=(1, 0, 0), rot_deg=175.0, t_true=FACING), "accepted",
     dict(accepted=True, pivot=0, r0_flipped=False), (6.8e-16, 1.3e-15, 5.7e-14, 2.8e-10))         # 5.64e-17, 1.11e-16, 4.79e-15, 2.37e-11
_add("pivot1_y185", lambda: make_scene(64, seed=20, rot_axis=(0, 1, 0), rot_deg=-175.0, t_true=FACING), "accepted",
     dict(accepted=True, pivot=1, r0_flipped=True), (5.7e-16, 2.7e-15, 6.7e-14, 2.2e-10))          # 4.77e-17, 2.22e-16, 5.61e-15, 1.84e-11
_add("pivot2_z175", lambda: make_scene(64, seed=20, rot_axis=(0, 0, 1), rot_deg=175.0), "accepted",
     dict(accepted=True, pivot=2, r0_flipped=False), (1.2e-15, 2.1e-14, 1.1e-14, 1.2e-11))         # 1.39e-17 (90 x), 1.78e-15, 8.99e-16, 9.91e-13
_add("qn_flip_across_180", lambda: _exact(64, 21, rot_axis=(0, 0, 1), rot_deg=180.1, start_rot_deg=179.9), "accepted",
     dict(accepted=True, pivot=2, qn_flipped=True), (2.7e-14, 2.9e-12, 6e-15, 1.4e-14))            # 2.22e-15, 2.42e-13, 4.98e-16, 1.13e-15
_add("t_unit_kept", lambda: _exact(64, 22, t_scale=1.00005, rot_err_deg=0.0, t_err=0.0, point_err=0.0), "accepted",
     dict(accepted=True, t_case="kept_unit", t_out_is_unit=False), (0, 0, 6.5e-15, 7.2e-15))       # 0, 0, 5.45e-16, 6.04e-16
_add("t_times3_normalised", lambda: make_scene(64, seed=22, t_scale=3.0), "accepted", dict(accepted=True, t_case="normalised"),
     (4.6e-16, 0, 8.1e-15, 8.1e-12), t_norm_thresh=10.0)                                           # 5.20e-18 (90 x), 0, 6.71e-16, 6.73e-13
# |t| = 5e-4 and the points with it: R is held bit for bit (mu ends at 9e7, the rotation's last steps do not reach its last bit)
_add("t_tiny_kept", lambda: _shrunk(64, 25, 5e-4), "accepted", dict(accepted=True, t_case="kept_tiny"),
     (1.9e-17, 2.1e-17, 2.7e-14, 6.8e-12))                                                         # 2.17e-19 (90 x), 1.73e-18, 2.25e-15, 5.63e-13
_add("refused_by_t_norm", lambda: make_scene(64, 64, 12, 0.3), "refused", dict(accepted=False, stop=4, refused_by=("t_norm",)),
     (0, 0, 8.9e-13, 8.9e-13), t_norm_thresh=1e-6)                                                 # -, -, 7.41e-14, 7.39e-14
# sizes: the refusal boundary with and without a mask, the lane-ownership boundaries
_add("n11", lambda: make_scene(11, seed=51), "refused", dict(accepted=False, itno=0, stop=0), (0, 0, 0, 0))
_add("n11_of_40", lambda: make_scene(11, 40, seed=51), "refused", dict(accepted=False, itno=0, stop=0), (0, 0, 0, 0))
for _n, _tol in ((12, (3.1e-16, 0, 2.4e-15, 3e-12)),                                               # 3.47e-18 (90 x), 0, 1.99e-16, 2.46e-13
                 (13, (3.7e-15, 8e-14, 4.2e-14, 4.2e-10)),                                         # 4.16e-17 (90 x), 8.88e-16 (90 x), 3.47e-15, 3.45e-11
                 (255, (2.8e-15, 9.9e-15, 9.5e-15, 1.2e-12)),                                      # 3.12e-17 (90 x), 1.11e-16 (90 x), 7.86e-16, 1.01e-13
                 (256, (5.9e-16, 3.9e-14, 1.4e-14, 4.7e-11)),                                      # 4.86e-17, 4.44e-16 (90 x), 1.13e-15, 3.92e-12
                 (512, (1.7e-15, 4.3e-14, 1.5e-14, 3.2e-10)),                                      # 1.39e-16, 3.55e-15, 1.22e-15, 2.67e-11
                 (513, (3.4e-15, 1.9e-14, 1.8e-14, 7e-11))):                                       # 3.82e-17 (90 x), 2.22e-16 (90 x), 1.44e-15, 5.77e-12
    _add("n%d" % _n, (lambda n: lambda: make_scene(n, seed=40 + n))(_n), "accepted", dict(accepted=True), _tol)
_add("n12_of_40", lambda: make_scene(12, 40, seed=52), "accepted", dict(accepted=True),
     (1.4e-15, 3.9e-14, 5.1e-14, 4.5e-10))                                                         # 1.11e-16, 4.44e-16 (90 x), 4.21e-15, 3.76e-11

INFO_COMPARED = {"accepted": (0, 1), "refused": (0, 1, 2, 3, 4)}


def rel_diff(got, want):
    """|got - want| / |want|; 0 when both are not finite or bit-equal, inf when only one is not finite or want is 0 and got is not."""
    if not np.isfinite(want) or not np.isfinite(got):
        return 0.0 if (not np.isfinite(want) and not np.isfinite(got)) else np.inf
    if got == want:
        return 0.0
    return abs(got - want) / abs(want) if want != 0 else np.inf


_branch_spread = {}


def branch_spread(name):
    """-> dict(pose, q, info, mu, stable) of ONE scene of BRANCH_SCENES, as permutation_spread measures them over SCENES; info over
    INFO_COMPARED of the scene's kind.  The permutations are seeded by the scene's name, so a new row leaves the others' figures alone."""
    if name not in _branch_spread:
        s, o, kind = scene(name), oracle_result(name), BRANCH_SCENES[name]["kind"]
        sp = dict(pose=0.0, q=0.0, info=0.0, mu=0.0, stable=True)
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        for _ in range(N_PERMUTATIONS):
            r = run_oracle(s, rng.permutation(s["p1"].shape[0]))
            if integers(r) != integers(o):
                sp["stable"] = False
                continue
            if kind == "accepted":
                sp["pose"] = max(sp["pose"], np.abs(r["R"] - o["R"]).max(), np.abs(r["t"] - o["t"]).max())
                sp["q"] = max(sp["q"], np.abs(r["Q"] - o["Q"]).max())
            sp["info"] = max([sp["info"]] + [rel_diff(r["info"][i], o["info"][i]) for i in INFO_COMPARED[kind]])
            sp["mu"] = max(sp["mu"], rel_diff(r["mu"], o["mu"]))
        _branch_spread[name] = sp
    return _branch_spread[name]
