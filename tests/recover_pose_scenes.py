"""Scenes, masks and cases of the pose-recovery tests (test_oracle_recover_pose.py on the CPU, test_gpu_recover_pose.py on the MI355X).

The generator is synth.pose_scene's with an arbitrary motion: points uniform in x, y in [-2, 2] and z in [4, 12], 0.3 px of noise, 80 %
inliers, uniform outliers in each view's bounding box, points less than 0.5 deep in view 2 dropped (their places go to outliers), and the
exact E = [t]x R / |.|.  The motions are chosen so that every candidate of [R1|t] [R2|t] [R1|-t] [R2|-t] wins somewhere (asserted on the CPU,
test_oracle_recover_pose.py); `forward` is the one motion where all four candidates get points, which the tie cases are built from."""
import numpy as np

import recover_pose_oracle as RPO
from matchinglib_poselib_amd import synth

LADDER = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2049)   # either side of a wave (64), of a wave's 256-point share, of a workgroup's 1024; 2049 = a third workgroup
SHORT = (65, 257)
MOTIONS = {   # axis, degrees, t before normalising
    "side5": ((.2, .9, .1), 5, (1, .05, -.02)),
    "side05": ((.2, .9, .1), 0.5, (1, .05, -.02)),
    "forward": ((.1, .2, .9), 3, (.02, -.03, 1)),
    "backward": ((.1, .2, .9), 3, (.02, .03, -1)),
    "vertical": ((.9, .1, .2), 8, (.05, -1, .1)),
    "roll30": ((0, 0, 1), 30, (-1, .2, .1)),
    "roll90": ((.05, .02, 1), 90, (.6, -.7, .2)),
    "roll170": ((.02, .03, 1), 170, (.5, .5, .3)),
    "yaw20": ((0, 1, 0), 20, (-1, 0, .3)),
    "norot": (None, 0, (1, 0, 0)),
}
SCALES = {"pos": 1.0, "neg": -1.0, "x2.5": 2.5}
# (scale of E, dist, coincident): the full product of scale and distance, and the coincident rows under either sign
VARIANTS = tuple((s, d, False) for d in (50.0, 9.0) for s in SCALES) + (("pos", 50.0, True), ("neg", 9.0, True))
MASKS = ("none", "half", "zero", "ones", "first256")
MARGIN = 1e-9
SENTINEL = 0xA5


def sizes(motion):
    return LADDER if motion in ("forward", "side5") else SHORT


def motion(name):
    """-> R, t (unit)"""
    axis, deg, t = MOTIONS[name]
    R = np.eye(3) if axis is None else synth._rot(axis, deg)
    t = np.asarray(t, np.float64)
    return R, t / np.linalg.norm(t)


def essential(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return E / np.linalg.norm(E)


_scenes, _cands = {}, {}


def scene(name, n, coincident=False):
    """-> p1, p2 (n x 2 float64).  seed = 100 + n; `coincident`: 2 % of the rows get p2 = p1."""
    key = (name, n, coincident)
    if key not in _scenes:
        if coincident:
            p1, p2 = scene(name, n)
            p2 = p2.copy()
            idx = np.random.default_rng(n).permutation(n)[:coincident_rows(n)]
            p2[idx] = p1[idx]
        elif n == 0:
            p1, p2 = np.zeros((0, 2)), np.zeros((0, 2))
        else:
            R, t = motion(name)
            rng = np.random.default_rng(100 + n)
            n_in = int(round(n * 0.8))
            X = np.stack([rng.uniform(-2, 2, n_in), rng.uniform(-2, 2, n_in), rng.uniform(4, 12, n_in)], 1)
            x1 = X[:, :2] / X[:, 2:3]
            X2 = X @ R.T + t
            keep = X2[:, 2] > 0.5
            x2 = X2[:, :2] / X2[:, 2:3]
            s = 0.3 * synth.PIX_TO_CAM
            x1 = x1 + rng.normal(0, s, x1.shape)
            x2 = x2 + rng.normal(0, s, x2.shape)
            x1, x2 = x1[keep], x2[keep]
            no = n - len(x1)
            o1 = rng.uniform(x1.min(0), x1.max(0), (no, 2))
            o2 = rng.uniform(x2.min(0), x2.max(0), (no, 2))
            perm = rng.permutation(n)
            p1, p2 = np.ascontiguousarray(np.concatenate([x1, o1])[perm]), np.ascontiguousarray(np.concatenate([x2, o2])[perm])
        _scenes[key] = (p1, p2)
    return _scenes[key]


def coincident_rows(n):
    return int(round(0.02 * n))


def variants(name, n):
    """The variants of one (motion, size): no coincident rows where there would be none, and none on `norot` (parallel rays, the predicates
    are decided by rounding there: test_oracle_recover_pose.py records the margin)."""
    return tuple(v for v in VARIANTS if not v[2] or (coincident_rows(n) > 0 and name != "norot"))


def E_of(name, scale):
    return SCALES[scale] * essential(*motion(name))


def mask(n, kind):
    rng = np.random.default_rng(n + 7)
    if kind == "none":
        return None
    if kind == "half":
        return (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(2, 256, n).astype(np.uint8)   # any nonzero byte counts
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind == "ones":
        return np.ones(n, np.uint8)        # 0 / 1 as StereoRefine holds it: 1 & 255 stays 1
    m = rng.integers(1, 256, n).astype(np.uint8)   # first256: the wave that owns rows 0 .. 255 has nothing to do
    m[:256] = 0
    return m


def cand(oracle, name, n, scale, coincident=False, translation=False):
    key = (name, n, scale, coincident, translation)
    if key not in _cands:
        p1, p2 = scene(name, n, coincident)
        _cands[key] = RPO.candidates(oracle, E_of(name, scale), p1, p2, translation)
    return _cands[key]


_results = {}


def expected(oracle, name, n, variant, kind):
    """The restatement's result of one case (computed once, shared, not to be changed)."""
    key = (name, n, variant, kind)
    if key not in _results:
        scale, dist, coincident = variant
        _results[key] = RPO.decide(cand(oracle, name, n, scale, coincident), mask(n, kind), dist)
    return _results[key]


def comparable(Q):
    return np.all(np.isfinite(Q), axis=1) & (np.abs(Q).max(axis=1) < 1e6)


# ---- ties: `forward`, n = 257, E, dist 50.  Every point is good under at most one candidate; the incoming mask keeps as many points
# exclusive to one candidate as to the other and nothing else, so their counts are equal and the others zero.
TIE_N = 257
TIES = tuple((a, b) for a in range(4) for b in range(a + 1, 4)) + ("all", "only3")


def tie_expected_pick(tie):
    return {"all": 0, "only3": 3}.get(tie, tie[0] if isinstance(tie, tuple) else None)


def exclusive(masks):
    M = masks != 0
    once = M.sum(0) == 1
    return [np.flatnonzero(M[c] & once) for c in range(4)]


def tie_mask(oracle, tie, name="forward", translation=False):
    """-> the incoming mask (arbitrary nonzero bytes on the kept rows) and k, the tied count."""
    base = RPO.decide(cand(oracle, name, TIE_N, "pos", translation=translation), None, 50.0)
    ex = exclusive(base["masks"])
    who = (0, 1, 2, 3) if tie == "all" else (3,) if tie == "only3" else tie
    k = min(len(ex[c]) for c in who)
    m = np.zeros(TIE_N, np.uint8)
    rng = np.random.default_rng(5)
    for c in who:
        m[ex[c][:k]] = rng.integers(1, 256, k)
    return m, k


# ---- the batch: eight problems of one launch, every pick among them
BATCH_COUNTS = (0, 1, 64, 257, 1024, 1025, 2049, 300)
BATCH_STRIDE = 2049 + 7
BATCH_MOTIONS = (("forward", "pos"), ("side5", "pos"), ("side5", "neg"), ("backward", "pos"), ("forward", "pos"), ("backward", "neg"),
                 ("roll90", "pos"), ("vertical", "neg"))
BATCH_MASKS = ("half", "none", "first256")

# ---- translation only: `norot` (R = I) and its essential matrix [t]x, from which getTfromTransEssential reads -t: E picks [I|-t] (2), -E
# picks [I|t] (0); the tie keeps as many rows exclusive to candidate 0 as to candidate 2 (tie_mask((0, 2), "norot", translation=True))
TRANS_SIZES = (1, 64, 65, 257)
TRANS_PICKS = {"pos": 2, "neg": 0}
