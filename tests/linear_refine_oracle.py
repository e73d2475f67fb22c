"""float64 NumPy restatement of poselib::refineEssentialLinear (P/source/pose_linear_refinement.cpp:85-635) -- the checker of
mlpl_refine_essential_linear.  TEST INFRASTRUCTURE ONLY.

The reference needs OpenCV, which this project does not have, so the loop is restated here step by step:
  findRefinementWeights :314-345   Torr (weightingEssential.cpp:210-227) / pseudo-Huber (:165-207, threshold th * ph_mult) weights
  refineModel :347-602             PR_8PT: eightpt_weight / OpenGV eightpt (rows scaled by w / ||w||, the smallest eigenvector, then
                                   U diag(s0, s1, 0) V^T with Eigen's JacobiSVD: oracle_eigen_svd3); PR_NISTER / PR_STEWENIUS: the
                                   five-point system on all listed rows (oracle_run5point_rows), of several solutions the smallest
                                   Sampson-error sum over the list with the early exit at every 4th list position
  evaluateModelE :608-635          getSampsonL2Error on bearing vectors (pose_helper.cpp:3011-3020) < the step's threshold
The bearing vectors follow the device's dg_bearing (x / sqrt(x^2 + (y^2 + 1))); every expression keeps the device's operation order, so
the two agree to rounding and a mask bit can only differ for a point whose error sits on a threshold (`margin` reports the closest one).
"""
import ctypes as C

import numpy as np

import oracle_lib

MLPL_OK, MLPL_E_BAD_INPUT, MLPL_E_UNSUPPORTED, MLPL_E_FAILED = 0, -1, -2, -3
PR_8PT, PR_NISTER, PR_STEWENIUS, PR_KNEIP = 0x1, 0x2, 0x3, 0x4
PR_TORR_WEIGHTS, PR_PSEUDOHUBER_WEIGHTS, PR_NO_WEIGHTS = 0x10, 0x20, 0x30

_lib_cache = None


def _lib():
    global _lib_cache
    if _lib_cache is None:
        lib = oracle_lib.load().lib
        lib.oracle_run5point_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.oracle_run5point_rows.restype = C.c_int
        lib.oracle_eigen_svd3.argtypes = [C.c_void_p] * 4
        lib.oracle_eigen_svd3.restype = None
        _lib_cache = lib
    return _lib_cache


def bearing(p):
    x, y = p[:, 0], p[:, 1]
    nrm = np.sqrt(x * x + (y * y + 1.0))
    return np.stack([x / nrm, y / nrm, 1.0 / nrm], axis=1)


def rows(f1, f2):
    """row i, entry 3 a + b = f2[a] f1[b] (the reference's f2 (x) f1)."""
    return (f2[:, :, None] * f1[:, None, :]).reshape(-1, 9)


def torr_weight(E, f, fp):
    e = E.reshape(9)
    rxc = e[0] * fp[:, 0] + e[3] * fp[:, 1] + e[6] * fp[:, 2]
    ryc = e[1] * fp[:, 0] + e[4] * fp[:, 1] + e[7] * fp[:, 2]
    rx = e[0] * f[:, 0] + e[1] * f[:, 1] + e[2] * f[:, 2]
    ry = e[3] * f[:, 0] + e[4] * f[:, 1] + e[5] * f[:, 2]
    return 1 / np.sqrt(rxc * rxc + ryc * ryc + rx * rx + ry * ry)


def pseudo_huber_weight(E, f, fp, th):
    e = E.reshape(9)
    xpE = [fp[:, 0] * e[c] + fp[:, 1] * e[3 + c] + fp[:, 2] * e[6 + c] for c in range(3)]
    num = xpE[0] * f[:, 0] + xpE[1] * f[:, 1] + xpE[2] * f[:, 2]
    e0 = e[0] * f[:, 0] + e[1] * f[:, 1] + e[2] * f[:, 2]
    e1 = e[3] * f[:, 0] + e[4] * f[:, 1] + e[5] * f[:, 2]
    denom1 = 1 / (np.sqrt(e0 * e0 + e1 * e1 + xpE[0] * xpE[0] + xpE[1] * xpE[1]) + 1e-8)
    d_abs = np.abs(num * denom1) + 1e-12
    q = d_abs / th
    return denom1 * (np.sqrt(2 * (th * th) * (np.sqrt(1 + q * q) - 1)) / d_abs)


def sampson_l2(E, f, fp):
    e = E.reshape(9)
    x2E = [fp[:, 0] * e[c] + fp[:, 1] * e[3 + c] + fp[:, 2] * e[6 + c] for c in range(3)]
    r = x2E[0] * f[:, 0] + x2E[1] * f[:, 1] + x2E[2] * f[:, 2]
    rx = e[0] * f[:, 0] + e[1] * f[:, 1] + e[2] * f[:, 2]
    ry = e[3] * f[:, 0] + e[4] * f[:, 1] + e[5] * f[:, 2]
    return r * r / (x2E[0] * x2E[0] + x2E[1] * x2E[1] + rx * rx + ry * ry)


def sampson_pick(E, f, fp):
    """PoseTools::getSampsonError (PoseFunctions.cpp:146) on the bearing vectors divided by their third component."""
    m = E.reshape(9)
    x1, y1, x2, y2 = f[:, 0] / f[:, 2], f[:, 1] / f[:, 2], fp[:, 0] / fp[:, 2], fp[:, 1] / fp[:, 2]
    rxc = m[0] * x2 + m[3] * y2 + m[6]
    ryc = m[1] * x2 + m[4] * y2 + m[7]
    rwc = m[2] * x2 + m[5] * y2 + m[8]
    r = x1 * rxc + y1 * ryc + rwc
    rx = m[0] * x1 + m[1] * y1 + m[2]
    ry = m[3] * x1 + m[4] * y1 + m[5]
    return r * r / (rxc * rxc + ryc * ryc + rx * rx + ry * ry)


def run5point_rows(Q):
    """All real solutions of the five-point system of the rows Q (n x 9), Frobenius-normalised 3 x 3 matrices."""
    Q = np.ascontiguousarray(Q, np.float64)
    out = np.zeros((10, 9))
    nm = _lib().oracle_run5point_rows(Q.ctypes.data, Q.shape[0], out.ctypes.data)
    return [out[k].reshape(3, 3).copy() for k in range(nm)]


def eigen_svd3(M):
    M = np.ascontiguousarray(M, np.float64)
    sv, U, V = np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3))
    _lib().oracle_eigen_svd3(M.ctypes.data, sv.ctypes.data, U.ctypes.data, V.ctypes.data)
    return sv, U, V


def fit_8pt(Q):
    """solveUsingEigenVectors (weightingEssential.cpp:302-330) + the rank-2 step of eightpt_weight (:276-298)."""
    # The 9th right singular vector.  The thin SVD of 8 rows ends at the 8th, so they get the full one (their exact null vector; the
    # reference takes matrixV().col(8) of the full SVD there, :311-317); from 9 rows on the thin SVD's last row is that vector, and the
    # full one would build a rows x rows U (seconds and gigabytes on the lists of thousands of rows that the other tests pass).
    _, _, Vt = np.linalg.svd(Q, full_matrices=Q.shape[0] < 9)
    F = Vt[-1].reshape(3, 3)
    sv, U, V = eigen_svd3(F)
    return U @ np.diag([sv[0], sv[1], 0.0]) @ V.T


def pick_trace(sols, f, fp):
    """refineModel's choice (pose_linear_refinement.cpp:437-470): sums in list order, early exit at list positions i > 3, i % 4 == 0.
    -> (index of the chosen solution, exit position or -1, fires, errs): fires = every position at which the test holds when the sums are
    continued over the whole list (the exit is fires[0]), each with the solution that is smallest there: what a device that missed the
    exit would choose; errs[solution][list position] = the summed errors."""
    errs = np.stack([sampson_pick(E, f, fp) for E in sols])  # [solutions][list position]
    sums = np.zeros(len(sols))
    chosen, at, fires = None, -1, []
    for i in range(errs.shape[1]):
        sums = sums + errs[:, i]
        if i > 3 and i % 4 == 0:
            s2 = np.sort(sums)
            if s2[0] < 0.66 * s2[1]:
                fires.append((i, int(np.argmin(sums))))
                if chosen is None:
                    chosen, at = int(np.argmin(sums)), i
    if chosen is None:
        chosen = int(np.argmin(sums))
    return chosen, at, tuple(fires), errs


def pick(sols, f, fp):
    return sols[pick_trace(sols, f, fp)[0]]


def _canonical(sols):
    """The solver's solutions in an order of their own (by the first entry once the entry of largest magnitude is made 1): the solver's
    order follows its basis of the null space, which rounding alone decides where that space is degenerate (6 rows).  The choice does not
    depend on the order (ties aside); the trace's `chosen` does."""
    def key(S):
        v = S.reshape(9)
        return v[0] / v[np.argmax(np.abs(v))]
    return sorted(sols, key=key)


def _nudge(rng, A, rel):
    """A moved by rel * |A| in a random direction (row by row for a matrix of rows); rng None: A itself."""
    if rng is None:
        return A
    d = rng.normal(size=A.shape)
    if A.ndim == 2 and A.shape[1] == 9:
        return A + rel * np.linalg.norm(A, axis=1, keepdims=True) * d / np.linalg.norm(d, axis=1, keepdims=True)
    return A + rel * np.linalg.norm(A) * d / np.linalg.norm(d)


def refine_essential_linear(p1, p2, E, mask, method, th=0.008, steps=4, th_mult=2.0, ph_mult=0.1, max_loss=0.15, _rng=None,
                            _rel=(1e-8, 1e-12)):
    """-> dict(rc, E, mask, n_inliers, steps_done, margin, trace, end): rc as mlpl_refine_essential_linear; margin = the smallest relative
    distance of an evaluated error from its step's threshold (inf when nothing was evaluated).
    trace = one record per step that was begun, a dict of
      n_list   the list length
      wn       the weight norm (None without weights)
      n_sols   the number of real solutions (1 for the 8-point fit, None when no fit was run)
      exit     the list position of the choice's early exit, -1 for none, None with one solution / the 8-point fit
      fires    every (position, smallest solution) at which the exit test holds with the sums continued over the list
      errs     the choice's error matrix [solution][list position]
      chosen   the index of the chosen solution among the solver's, in _canonical's order
      count    the points under the step's threshold
      verdict  "accepted" / "rejected" (lost too many at step 0) / "stopped" (lost too many later) / None (no fit)
      end      None while the loop goes on; on the last record why it ended.
    end (also res["end"]): "steps" (exhausted), "loss", "rejected", "no fit: solver", "no fit: rows" (8-point on fewer than 8),
    "no fit: weights" (all zero or not finite), "no fit: not finite", "no fit: no solution"; "too few" when fewer than 6 rows are listed,
    "method" for a refused method.
    _rng, _rel (stable() only): every candidate model is moved by a relative _rel[0], the rows handed to the five-point solver by _rel[1]."""
    p1 = np.ascontiguousarray(p1, np.float64)
    p2 = np.ascontiguousarray(p2, np.float64)
    E = np.array(E, np.float64).reshape(3, 3)
    mask = np.array(mask, np.uint8).reshape(-1)
    solver, wbits = method & 0xF, method & 0xF0
    trace = []
    res = dict(rc=MLPL_E_FAILED, E=E.copy(), mask=mask.copy(), n_inliers=0, steps_done=0, margin=np.inf, trace=trace, end="method")
    if solver == PR_KNEIP:
        res["rc"] = MLPL_E_UNSUPPORTED
        return res
    if solver == PR_8PT and wbits not in (PR_TORR_WEIGHTS, PR_PSEUDOHUBER_WEIGHTS, PR_NO_WEIGHTS):
        res["rc"] = MLPL_E_BAD_INPUT
        return res
    cur = np.flatnonzero(mask != 0)
    if cur.size < 6:
        res["end"] = "too few"
        return res
    f, fp = bearing(p1), bearing(p2)
    fit = 1 if solver == PR_8PT else (2 if solver in (PR_NISTER, PR_STEWENIUS) else 0)
    wmode = 0 if fit == 0 else {PR_TORR_WEIGHTS: 1, PR_PSEUDOHUBER_WEIGHTS: 2}.get(wbits, 0)
    th2 = th * th
    step_size = (th_mult * th2 - th2) / steps if steps else 0.0
    margin, done, end = np.inf, 0, "steps"
    for j in range(steps):
        rec = dict(n_list=int(cur.size), wn=None, n_sols=None, exit=None, fires=(), errs=None, chosen=None, count=None, verdict=None, end=None)
        trace.append(rec)
        if fit == 0 or (fit == 1 and cur.size < 8):
            end = "no fit: solver" if fit == 0 else "no fit: rows"
            break
        Q = rows(f[cur], fp[cur])
        if wmode:
            w = torr_weight(E, f[cur], fp[cur]) if wmode == 1 else pseudo_huber_weight(E, f[cur], fp[cur], th * ph_mult)
            with np.errstate(over="ignore"):   # squares past DBL_MAX: an infinite norm, refused below
                wn = np.sqrt(np.sum(w * w))
            rec["wn"] = float(wn)
            if not (0 < wn < np.inf):  # every weight zero (a model exact to rounding under pseudo-Huber): the reference divides 0 by 0
                end = "no fit: weights"
                break
            Q = Q * (w / wn)[:, None]
        if fit == 1:
            En = fit_8pt(Q)
            if not np.all(np.isfinite(En)):
                end = "no fit: not finite"
                break
            En = _nudge(_rng, En, _rel[0])
            rec.update(n_sols=1, chosen=0)
        else:
            sols = [_nudge(_rng, S, _rel[0]) for S in _canonical(run5point_rows(_nudge(_rng, Q, _rel[1])))]
            rec["n_sols"] = len(sols)
            if not sols:
                end = "no fit: no solution"
                break
            if len(sols) == 1:
                rec["chosen"] = 0
            else:
                rec["chosen"], rec["exit"], rec["fires"], rec["errs"] = pick_trace(sols, f[cur], fp[cur])
            En = sols[rec["chosen"]]
        thr = (th_mult * th2) - (j + 1) * step_size
        err = sampson_l2(En, f, fp)
        margin = min(margin, float(np.min(np.abs(err - thr)) / thr))
        nxt = np.flatnonzero(err < thr)
        rec["count"] = int(nxt.size)
        if float(nxt.size) >= (1.0 - max_loss) * float(cur.size):
            E, cur, done = En, nxt, done + 1
            rec["verdict"] = "accepted"
        elif j == 0:
            rec["verdict"], rec["end"] = "rejected", "rejected"
            res.update(margin=margin, end="rejected")
            return res
        else:
            rec["verdict"], end = "stopped", "loss"
            break
    if trace:
        trace[-1]["end"] = end
    m = np.zeros_like(mask)
    m[cur] = 1
    res.update(rc=MLPL_OK, E=E.copy(), mask=m, n_inliers=int(cur.size), steps_done=done, margin=margin, end=end)
    return res


def _decisions(r):
    return (r["rc"], r["steps_done"], r["end"], r["mask"].tobytes(),
            tuple((t["n_list"], t["n_sols"], t["exit"], t["chosen"], t["count"], t["verdict"], t["end"]) for t in r["trace"]))


def _same_model(A, B, tol):
    a, b = A.reshape(9) / np.linalg.norm(A), B.reshape(9) / np.linalg.norm(B)
    return min(np.abs(a - b).max(), np.abs(a + b).max()) <= tol


def stable(p1, p2, E, mask, method, reruns=5, seed=0, **kw):
    """Whether the case can be decided against the device.
    1. `reruns` runs in which every candidate model is moved by a relative 1e-8 (the bar E is held to) and the five-point solver's rows by
       1e-12, each in a random direction, must all reach the decisions of the plain run: the list length, the number of solutions, the
       exit position, the chosen index, the count and the verdict of every step, why the loop ended, and the mask.  This stands in for a
       numeric margin on the choice among solutions.
    2. The restatement must reproduce its own model: with the solver's rows moved by 1e-15 (rounding, nothing else) the returned E stays
       within 1e-9, a tenth of the bar.  The five-point solver is OpenCV's (Durand-Kerner on the degree-10 polynomial, the null vector per
       root), and on some systems -- rows on one plane more often than others -- a root comes out 1e-7 .. 1e-5 off whatever the rounding
       (DESIGN section 0 counts 0.36 % of minimal models); a model compared at 1e-8 has to come from a reference that holds 1e-9."""
    plain = refine_essential_linear(p1, p2, E, mask, method, **kw)
    want = _decisions(plain)
    rng = np.random.default_rng(seed)
    if not all(_decisions(refine_essential_linear(p1, p2, E, mask, method, _rng=rng, **kw)) == want for _ in range(reruns)):
        return False
    for _ in range(reruns):
        r = refine_essential_linear(p1, p2, E, mask, method, _rng=rng, _rel=(0.0, 1e-15), **kw)
        if _decisions(r) != want or not _same_model(r["E"], plain["E"], 1e-9):
            return False
    return True
