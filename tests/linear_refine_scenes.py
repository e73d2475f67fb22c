"""Scenes of the refineEssentialLinear edge tests (test_oracle_linear_refine.py on the CPU, test_gpu_linear_refine_edges.py on the MI355X).

Every scene is generated from a seed (no files): `cnt` listed rows that are noisy projections of 3-D points under one of
recover_pose_scenes' motions, the other rows projections and uniform outliers, the listed rows placed by a mask pattern, and a starting
model E0 = scale * (the exact E + e0_eps * N(0, 1)).  TABLE names each scene, says what it is there for (`why`) and what the restatement's
trace must show (`claim`, checked by broken_claims).

The choice among five-point solutions: with every listed row on the 3-D plane z = 8 + 0.3 x - 0.2 y both essential matrices of the plane's
homography solve the system and fit the rows alike, so the early exit (tested at every 4th list position) fires nowhere; the ORDER of the
listed rows, which leaves the system as it is up to rounding, then places the exit (order_rows).

Seeds were searched on the CPU (the restatement only) until the trace showed the branch a scene is there for and the scene was decidable:
margin > 1e-9 and linear_refine_oracle.stable(); test_oracle_linear_refine.py asserts both for every scene, none is exempt."""
import numpy as np

import linear_refine_oracle as LRO
import recover_pose_scenes as RPS
from matchinglib_poselib_amd import synth

METHODS = tuple(s | w for s in (0x1, 0x2, 0x3) for w in (0x10, 0x20, 0x30))
FIVE_POINT = tuple(m for m in METHODS if m & 0xF != 0x1)
COUNTS = (6, 7, 8, 9, 63, 64, 65, 127, 128, 129, 257)
MARGIN = 1e-9
SENTINEL = 0xA5
TH = 0.8 * synth.PIX_TO_CAM


def _points(rng, k, planar):
    x, y = rng.uniform(-2, 2, k), rng.uniform(-2, 2, k)
    z = 8 + 0.3 * x - 0.2 * y if planar else rng.uniform(4, 12, k)
    return np.stack([x, y, z], 1)


def _views(rng, X, R, t, noise_px):
    X2 = X @ R.T + t
    assert np.all(X2[:, 2] > 0.5)
    s = noise_px * synth.PIX_TO_CAM
    x1, x2 = X[:, :2] / X[:, 2:3], X2[:, :2] / X2[:, 2:3]
    return x1 + rng.normal(0, s, x1.shape), x2 + rng.normal(0, s, x2.shape)


def listed_rows(n, cnt, kind):
    """The listed rows of a mask kind, ascending."""
    if kind == "spread":          # evenly over the rows
        return np.unique(np.linspace(0, n - 1, cnt).round().astype(int))
    if kind == "first":
        return np.arange(cnt)
    if kind == "last":            # only the last rows (cnt <= 64 of n = 257: the last 64-row block alone)
        return np.arange(n - cnt, n)
    if kind == "ends":            # row 0 and the last cnt - 1
        return np.concatenate([[0], np.arange(n - cnt + 1, n)])
    if kind == "second":          # every second row
        return np.arange(0, 2 * cnt, 2)
    raise ValueError(kind)


def _greedy(eA, eB, head, goal):
    """The rows `head` in an order whose running ratio sum(eB) / sum(eA) follows goal(position) as closely as a greedy choice can."""
    left, out, sA, sB = list(head), [], 0.0, 0.0
    for i in range(len(head)):
        want = np.log(goal(i))
        j = min(left, key=lambda r: abs(np.log((sB + eB[r]) / (sA + eA[r])) - want))
        left.remove(j)
        out.append(j)
        sA, sB = sA + eA[j], sB + eB[j]
    return out


def order_rows(errs, order):
    """A permutation of the listed rows that places the choice's exit.  A = the solution with the smallest total, B = the runner-up, r =
    the running sum of B's errors over that of A's; the test fires where r < 0.66 (B) or r > 1 / 0.66 (A), and the total says A.
      ("exit", k):  r is held at 0.70 up to position k - 4, brought under 0.66 by position k, back over it by k + 4 and then raised as
                    fast as the rows allow: the exit at k takes B, every later decision takes A, so a device that misses the exit, or
                    takes a later hit of the chunk for the first, returns another model.
      ("none", "flip", t):   the last t rows are those that speak most for A, and without them B is ahead: a device that leaves the
                    partial last chunk out of the sums returns B.
      ("none", "local", t):  the last t rows are those that speak most for B: a device that does not carry the sums into the last chunk
                    returns B.
      ("none", "plain"): r is held at the total's ratio."""
    tot = errs.sum(1)
    A, B = np.argsort(tot)[:2]
    eA, eB = errs[A], errs[B]
    cnt = eA.size
    if order[0] == "exit":
        k = order[1]
        return _greedy(eA, eB, range(cnt), lambda i: 0.70 if i < k - 3 else (0.62 if i <= k else (0.72 if i <= k + 4 else 1e3)))
    kind, t = order[1], (order[2] if len(order) > 2 else 0)
    d = np.argsort(eB - eA)
    tail = list(d[::-1][:t]) if kind == "flip" else list(d[:t])
    head = [r for r in range(cnt) if r not in set(tail)]
    hold = (tot[B] - eB[tail].sum()) / (tot[A] - eA[tail].sum())
    return _greedy(eA, eB, head, lambda i: hold) + tail[::-1]


def make(motion="side5", n=300, cnt=100, seed=0, method=0x22, plane=False, order=None, noise_px=0.3, mask="spread", mask_value=1,
         e0_eps=1e-4, scale=1.0, exact=0, rest_in=0.5, rows=None, kw=None, why=""):
    """-> dict(p1, p2, E0, mask, th, method, kw, why).
    plane: the listed rows' 3-D points lie on the plane; exact: that many of the listed rows (the first ones) carry no noise, with noise_px
    on the others; rest_in: the share of projections among the unlisted rows (0: outliers only); rows: the listed rows themselves;
    order: see order_rows (the listed rows are permuted, which leaves the first step's system, and hence its solutions, as they are up to
    rounding)."""
    R, t = RPS.motion(motion)
    rng = np.random.default_rng(seed)
    X = _points(rng, cnt, plane)
    a1, a2 = _views(rng, X, R, t, noise_px)
    if exact:
        b1, b2 = _views(rng, X[:exact], R, t, 0.0)
        a1[:exact], a2[:exact] = b1, b2
    if rows is not None:   # the listed rows given as (x1, y1, x2, y2)
        a1, a2 = np.array(rows)[:, :2], np.array(rows)[:, 2:]
    rest = n - cnt
    n_g = int(rest * rest_in)
    g1, g2 = _views(rng, _points(rng, n_g, False), R, t, noise_px)
    o1 = rng.uniform(a1.min(0), a1.max(0), (rest - n_g, 2))
    o2 = rng.uniform(a2.min(0), a2.max(0), (rest - n_g, 2))
    perm = rng.permutation(rest)
    u1, u2 = np.concatenate([g1, o1])[perm], np.concatenate([g2, o2])[perm]
    at = listed_rows(n, cnt, mask)
    assert at.size == cnt and at[-1] < n
    m = np.zeros(n, np.uint8)
    m[at] = mask_value if mask_value != "mixed" else rng.integers(2, 256, cnt)
    E0 = scale * (RPS.essential(R, t) + e0_eps * rng.normal(size=(3, 3)))
    kw = dict(kw or {})

    def place(a1, a2):
        p1, p2 = np.zeros((n, 2)), np.zeros((n, 2))
        p1[m != 0], p2[m != 0] = a1, a2
        p1[m == 0], p2[m == 0] = u1, u2
        return np.ascontiguousarray(p1), np.ascontiguousarray(p2)

    p1, p2 = place(a1, a2)
    if order is not None:
        o = LRO.refine_essential_linear(p1, p2, E0, m, method, th=TH, **dict(oracle_kw(kw), steps=1))
        errs = o["trace"][0]["errs"]
        if errs is None:
            raise ValueError("the first step has one solution: nothing to order")
        row = order_rows(errs, order)
        p1, p2 = place(a1[row], a2[row])
    return dict(p1=p1, p2=p2, E0=E0, mask=m, th=TH, method=method, kw=kw, why=why)


KW = dict(num_iterative_steps="steps", threshold_multiplier="th_mult", pseudo_huber_threshold_multiplier="ph_mult",
          max_relative_inlier_cnt_loss="max_loss")


def oracle_kw(kw):
    return {KW[k]: v for k, v in kw.items()}


_results = {}


def expected(name):
    """The restatement's result of a scene (computed once, shared, not to be changed)."""
    if name not in _results:
        s = scene(name)
        _results[name] = LRO.refine_essential_linear(s["p1"], s["p2"], s["E0"], s["mask"], s["method"], th=s["th"], **oracle_kw(s["kw"]))
    return _results[name]


def is_stable(name):
    s = scene(name)
    return LRO.stable(s["p1"], s["p2"], s["E0"], s["mask"], s["method"], th=s["th"], **oracle_kw(s["kw"]))


_scenes = {}


def scene(name):
    if name not in _scenes:
        spec = {k: v for k, v in TABLE[name].items() if k != "claim"}
        _scenes[name] = make(seed=SEEDS.get(name, 0), **spec)
    return _scenes[name]


def _argmin_upto(errs, lo, hi):
    return int(np.argmin(errs[:, lo:hi].sum(1)))


def broken_claims(name, o=None):
    """What the restatement's trace does NOT show of what the table says the scene is there for (empty: all shown)."""
    o = o or expected(name)
    claim, bad = TABLE[name].get("claim", {}), []
    t0 = o["trace"][0] if o["trace"] else None

    def need(what, ok):
        if not ok:
            bad.append(what)

    for key, want in claim.items():
        if key == "rc":
            need(f"rc {want}: {o['rc']}", o["rc"] == want)
        elif key == "end":
            need(f"end {want}: {o['end']}", o["end"] == want)
        elif key == "steps_done":
            lo, hi = want if isinstance(want, tuple) else (want, want)
            need(f"steps_done in {lo}..{hi}: {o['steps_done']}", lo <= o["steps_done"] <= hi)
        elif key == "n_sols":
            need(f"{want} solutions in the first step: {t0 and t0['n_sols']}", t0 is not None and t0["n_sols"] == want)
        elif key == "exit":
            need(f"exit at {want}: {t0 and t0['exit']}", t0 is not None and t0["exit"] == want)
            if t0 is None or t0["exit"] != want:
                continue
            errs, cnt, chosen = t0["errs"], t0["n_list"], t0["chosen"]
            if want >= 0:
                # every later decision takes another solution: the next tested position, the later hits, the whole list
                need("the whole list chooses another solution", _argmin_upto(errs, 0, cnt) != chosen)
                need("no later hit with the exit's solution", all(s != chosen for _, s in t0["fires"][1:]))
                chunk = [f for f in t0["fires"] if f[0] // 64 == want // 64]
                if cnt >= 64 and want % 64 != 60:   # 60 is the last tested position of its chunk
                    need("a second hit in the exit's chunk", len(chunk) >= 2)
            else:
                need("no position fires", not t0["fires"])
                tail = claim.get("tail")
                if tail == "flip":     # without the partial last chunk another solution is ahead
                    need("the partial last chunk decides", _argmin_upto(errs, 0, cnt // 64 * 64) != chosen)
                elif tail == "local":  # the last chunk on its own is for another solution
                    need("the last chunk alone chooses another solution", _argmin_upto(errs, (cnt - 1) // 64 * 64, cnt) != chosen)
        elif key == "first_verdict":
            need(f"first verdict {want}: {t0 and t0['verdict']}", t0 is not None and t0["verdict"] == want)
        elif key == "keeps_all":   # every step is accepted with exactly the rows it started from: the >= of the acceptance decides
            need("every step keeps exactly its rows", bool(o["trace"]) and all(t["count"] == t["n_list"] and t["verdict"] == "accepted" for t in o["trace"]))
        elif key == "loses_one":   # a step that loses exactly one row is not accepted
            last = o["trace"][-1] if o["trace"] else None
            need("the last step loses exactly one row", last is not None and last["count"] == last["n_list"] - 1 and last["verdict"] != "accepted")
        elif key == "some_weights_zero":
            s = scene(name)
            f, fp = LRO.bearing(s["p1"]), LRO.bearing(s["p2"])
            at = np.flatnonzero(s["mask"])
            w = LRO.pseudo_huber_weight(s["E0"], f[at], fp[at], s["th"] * s["kw"].get("pseudo_huber_threshold_multiplier", 0.1))
            need("some weights zero, not all", 0 < np.count_nonzero(w == 0) < w.size)
        elif key != "tail":
            raise KeyError(key)
    return bad


# ---- the table.  claim = what the first step's trace (or the result) must show; the seeds below were searched until it does ----
TABLE = {}


def _add(name, why, claim=None, **spec):
    assert name not in TABLE
    TABLE[name] = dict(spec, why=why, claim=claim or {})


# the choice among solutions: every row of the list on the plane, ordered by order_rows.  One step, so that the entry returns what the
# first choice took (over four steps the loop picks up rows off the plane and ends at the same model whichever solution came first)
ONE_STEP = dict(num_iterative_steps=1)
for _k, _cnt, _m in ((4, 100, 0x22), (8, 100, 0x12), (60, 100, 0x32), (64, 150, 0x23), (68, 150, 0x22), (128, 200, 0x12), (136, 257, 0x32)):
    _add(f"exit{_k}", f"the choice exits at list position {_k} with a solution that no later decision takes", dict(exit=_k, rc=0, steps_done=1),
         n=_cnt + 43, cnt=_cnt, method=_m, plane=True, order=("exit", _k), kw=ONE_STEP)
_NONE_WHY = dict(plain="one full chunk, the sums end at its last entry m - 1 = 63 (nothing in this scene tells a wrong choice apart)",
                 flip="the partial last chunk decides, a device that leaves it out returns the other solution",
                 local="the last chunk alone is for the other solution, a device that does not carry the sums returns it")
for _cnt, _m, _o in ((64, 0x22, ("none", "plain")), (65, 0x12, ("none", "flip", 1)), (129, 0x32, ("none", "local", 1)),
                     (200, 0x23, ("none", "flip", 8)), (203, 0x22, ("none", "local", 11))):
    _add(f"none{_cnt}", f"no exit over {_cnt} listed rows: {_NONE_WHY[_o[1]]}", dict(exit=-1, tail=_o[1], rc=0, steps_done=1), n=_cnt + 43, cnt=_cnt, method=_m,
         plane=True, order=_o, kw=ONE_STEP)
_add("sols2", "two real solutions", dict(n_sols=2, rc=0), n=143, cnt=100, method=0x22, plane=True, order=("exit", 8))
# six rows without geometry whose five-point system has ten real solutions: one in some 10^5 random draws has eight, none had ten; these
# came from a random walk that started at a draw with eight, kept to draws with at least eight and, once at ten, went on until every
# one of 30 copies moved by 1e-3 had ten as well.  One step with every loss allowed,
# so that the chosen solution is what the entry returns.
TEN = ((0.415983, -0.404592, 0.064326, -0.01365), (-0.217959, 0.024328, 0.222968, 0.548453), (-0.009421, -0.081539, 0.278474, 0.285585),
       (0.17897, -0.127365, 0.562756, 0.351886), (-0.130409, -0.391849, -0.434682, 0.238792), (0.37196, 0.585033, 0.469934, -0.490765))
for _m in (0x32, 0x23):
    _add(f"sols10_{_m:02x}", "ten real solutions (the most the choice handles)", dict(n_sols=10, rc=0, steps_done=1), n=17, cnt=6, method=_m, rows=TEN,
         kw=dict(num_iterative_steps=1, max_relative_inlier_cnt_loss=1.0))

# counts
_add("cnt5", "five listed rows: refused", dict(rc=LRO.MLPL_E_FAILED, end="too few"), n=18, cnt=5, method=0x21)
for _c in COUNTS:
    for _m in METHODS:
        _claim = dict(rc=0, steps_done=0, end="no fit: rows") if (_m & 0xF == 1 and _c < 8) else {}
        _add(f"cnt{_c}_{_m:02x}", f"{_c} listed rows", _claim, n=_c + _c // 2 + 11, cnt=_c, method=_m)
_add("cnt8_accept", "the 8-point fit on exactly 8 rows, accepted", dict(rc=0, steps_done=(1, 4)), n=23, cnt=8, method=0x21, noise_px=0.05)

# control flow
for _m in (0x21, 0x22):
    _add(f"loss_mid_{_m:02x}", "the loop stops by loss after an accepted step (3 % allowed)", dict(rc=0, end="loss", steps_done=(1, 3)), n=300, cnt=150,
         method=_m, noise_px=0.45, kw=dict(max_relative_inlier_cnt_loss=0.03))
_add("loss_mid_plane", "the same with the default 15 %, rows on the plane", dict(rc=0, end="loss", steps_done=(1, 3)), n=107, cnt=64, method=0x22, plane=True)
for _m in (0x21, 0x22):
    _add(f"loss0_keep_{_m:02x}", "max loss 0 and nothing lost: count == (1 - 0) * count is accepted", dict(rc=0, steps_done=4, keeps_all=True), n=130,
         cnt=90, method=_m, noise_px=0.05, rest_in=0.0, kw=dict(max_relative_inlier_cnt_loss=0.0))
    _add(f"loss0_one_{_m:02x}", "max loss 0 and one row lost: not accepted", dict(loses_one=True), n=130, cnt=90, method=_m, noise_px=0.25, rest_in=0.0,
         kw=dict(max_relative_inlier_cnt_loss=0.0))
for _m in (0x21, 0x22):
    _add(f"reject_{_m:02x}", "the first step loses more than 15 %: refused, nothing written", dict(rc=LRO.MLPL_E_FAILED, end="rejected"), n=200, cnt=120,
         method=_m, noise_px=1.2)
for _m in (0x21, 0x22, 0x13):
    for _s in (1, 2, 7):
        _add(f"steps{_s}_{_m:02x}", f"{_s} steps", dict(rc=0, steps_done=(1, _s)), n=200, cnt=120, method=_m, kw=dict(num_iterative_steps=_s))
    _add(f"thm1_{_m:02x}", "threshold multiplier 1: step size 0", dict(rc=0), n=200, cnt=120, method=_m, noise_px=0.15, kw=dict(threshold_multiplier=1.0))
    _add(f"thm3_{_m:02x}", "threshold multiplier 3", dict(rc=0, steps_done=(1, 4)), n=200, cnt=120, method=_m, kw=dict(threshold_multiplier=3.0))
for _m in (0x21, 0x22, 0x23):
    _add(f"ph001_{_m:02x}", "pseudo-Huber threshold multiplier 0.01", dict(rc=0), n=200, cnt=120, method=_m, kw=dict(pseudo_huber_threshold_multiplier=0.01))
    _add(f"ph1_{_m:02x}", "pseudo-Huber threshold multiplier 1", dict(rc=0, steps_done=(1, 4)), n=200, cnt=120, method=_m,
         kw=dict(pseudo_huber_threshold_multiplier=1.0))
for _m in (0x21, 0x22):
    _add(f"exact_{_m:02x}", "noise-free rows and the exact model: every pseudo-Huber weight is zero", dict(rc=0, steps_done=0, end="no fit: weights"),
         n=160, cnt=100, method=_m, noise_px=0.0, e0_eps=0.0)
    _add(f"half_{_m:02x}", "the same with noise on half of the rows: some weights zero, not all", dict(rc=0, steps_done=(1, 4), some_weights_zero=True),
         n=160, cnt=100, method=_m, exact=50, e0_eps=0.0)

# inputs
for _name, _sc in (("neg", -1.0), ("x2.5", 2.5), ("x1e-3", 1e-3)):
    for _m in (0x11, 0x21, 0x12, 0x22):
        _add(f"scale_{_name}_{_m:02x}", f"E0 times {_sc}", dict(rc=0, steps_done=(1, 4)), n=200, cnt=120, method=_m, scale=_sc)
_add("scale_tiny_11", "E0 times 1e-160: the Torr weights' squares overflow, their norm is infinite, no fit", dict(rc=0, steps_done=0, end="no fit: weights"),
     n=200, cnt=120, method=0x11, scale=1e-160)
for _mo in ("forward", "roll30", "roll90"):
    for _m in (0x21, 0x22, 0x33):
        _add(f"{_mo}_{_m:02x}", f"motion {_mo}", dict(rc=0, steps_done=(1, 4)), motion=_mo, n=200, cnt=120, method=_m)
for _m in (0x21, 0x22):
    _add(f"mask_last_{_m:02x}", "listed rows only in the last 64-row block of 257", dict(rc=0), n=257, cnt=40, method=_m, mask="last")
    _add(f"mask_ends_{_m:02x}", "rows 0 and n - 6 .. n - 1", dict(rc=0), n=257, cnt=7, method=_m, mask="ends")
    _add(f"mask_second_{_m:02x}", "every second row", dict(rc=0, steps_done=(1, 4)), n=257, cnt=128, method=_m, mask="second")
    _add(f"mask_two_{_m:02x}", "mask bytes 2", dict(rc=0, steps_done=(1, 4)), n=200, cnt=120, method=_m, mask_value=2)
    _add(f"mask_255_{_m:02x}", "mask bytes 255", dict(rc=0, steps_done=(1, 4)), n=200, cnt=120, method=_m, mask_value=255)
    _add(f"mask_mixed_{_m:02x}", "mask bytes 2 .. 255", dict(rc=0, steps_done=(1, 4)), n=200, cnt=120, method=_m, mask_value="mixed")

NAMES = tuple(TABLE)

SEEDS = {   # 0 where a name is absent
    "exit4": 1, "exit8": 1, "exit60": 1, "exit68": 2, "exit128": 116, "exit136": 20, "none64": 1, "none129": 1, "none200": 1, "sols2": 2, "loss_mid_21":
    3, "loss_mid_22": 8, "loss_mid_plane": 5, "loss0_one_21": 11, "loss0_one_22": 11, "forward_22": 3, "forward_33": 1, "reject_21": 1,
}
