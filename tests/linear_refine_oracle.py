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
    _, _, Vt = np.linalg.svd(Q, full_matrices=False)
    F = Vt[-1].reshape(3, 3)
    sv, U, V = eigen_svd3(F)
    return U @ np.diag([sv[0], sv[1], 0.0]) @ V.T


def pick(sols, f, fp):
    """refineModel's choice (pose_linear_refinement.cpp:437-470): sums in list order, early exit at list positions i > 3, i % 4 == 0."""
    errs = np.stack([sampson_pick(E, f, fp) for E in sols])  # [solutions][list position]
    sums = np.zeros(len(sols))
    for i in range(errs.shape[1]):
        sums = sums + errs[:, i]
        if i > 3 and i % 4 == 0:
            s2 = np.sort(sums)
            if s2[0] < 0.66 * s2[1]:
                break
    return sols[int(np.argmin(sums))]


def refine_essential_linear(p1, p2, E, mask, method, th=0.008, steps=4, th_mult=2.0, ph_mult=0.1, max_loss=0.15):
    """-> dict(rc, E, mask, n_inliers, steps_done, margin): rc as mlpl_refine_essential_linear; margin = the smallest relative distance of
    an evaluated error from its step's threshold (inf when nothing was evaluated)."""
    p1 = np.ascontiguousarray(p1, np.float64)
    p2 = np.ascontiguousarray(p2, np.float64)
    E = np.array(E, np.float64).reshape(3, 3)
    mask = np.array(mask, np.uint8).reshape(-1)
    solver, wbits = method & 0xF, method & 0xF0
    res = dict(rc=MLPL_E_FAILED, E=E.copy(), mask=mask.copy(), n_inliers=0, steps_done=0, margin=np.inf)
    if solver == PR_KNEIP:
        res["rc"] = MLPL_E_UNSUPPORTED
        return res
    if solver == PR_8PT and wbits not in (PR_TORR_WEIGHTS, PR_PSEUDOHUBER_WEIGHTS, PR_NO_WEIGHTS):
        res["rc"] = MLPL_E_BAD_INPUT
        return res
    cur = np.flatnonzero(mask != 0)
    if cur.size < 6:
        return res
    f, fp = bearing(p1), bearing(p2)
    fit = 1 if solver == PR_8PT else (2 if solver in (PR_NISTER, PR_STEWENIUS) else 0)
    wmode = 0 if fit == 0 else {PR_TORR_WEIGHTS: 1, PR_PSEUDOHUBER_WEIGHTS: 2}.get(wbits, 0)
    th2 = th * th
    step_size = (th_mult * th2 - th2) / steps if steps else 0.0
    margin, done = np.inf, 0
    for j in range(steps):
        if fit == 0 or (fit == 1 and cur.size < 8):
            break
        Q = rows(f[cur], fp[cur])
        if wmode:
            w = torr_weight(E, f[cur], fp[cur]) if wmode == 1 else pseudo_huber_weight(E, f[cur], fp[cur], th * ph_mult)
            wn = np.sqrt(np.sum(w * w))
            if not (0 < wn < np.inf):  # every weight zero (a model exact to rounding under pseudo-Huber): the reference divides 0 by 0
                break
            Q = Q * (w / wn)[:, None]
        if fit == 1:
            En = fit_8pt(Q)
            if not np.all(np.isfinite(En)):
                break
        else:
            sols = run5point_rows(Q)
            if not sols:
                break
            En = sols[0] if len(sols) == 1 else pick(sols, f[cur], fp[cur])
        thr = (th_mult * th2) - (j + 1) * step_size
        err = sampson_l2(En, f, fp)
        margin = min(margin, float(np.min(np.abs(err - thr)) / thr))
        nxt = np.flatnonzero(err < thr)
        if float(nxt.size) >= (1.0 - max_loss) * float(cur.size):
            E, cur, done = En, nxt, done + 1
        elif j == 0:
            res["margin"] = margin
            return res
        else:
            break
    m = np.zeros_like(mask)
    m[cur] = 1
    res.update(rc=MLPL_OK, E=E.copy(), mask=m, n_inliers=int(cur.size), steps_done=done, margin=margin)
    return res
