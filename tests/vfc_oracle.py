"""numpy restatement of the reference's VFC match filter (M/source/vfcMatches.cpp:63-100 filterWithVFC, M/source/vfc.cpp: the default
SparseVFC path -- VFC::VFC() sets _method = SPARSE_VFC and nothing changes it), in two arithmetics:

mode="float32_serial"  the reference operation by operation: float32 storage, strictly serial float32 sums (np.add.accumulate), pow(x, 2)
                       evaluated in double and stored as float, expf / logf as float32 functions, cv::solve(DECOMP_LU) as the float LU
                       with partial pivoting whose pivots below 10 * FLT_EPSILON declare the matrix singular (C = 0).
mode="float64"         what the device computes: the same float32 normalisation and control points, everything from the kernels K and U
                       on in float64 with the reference's float constants widened ((double)0.1f ...), the LU with the 100 * DBL_EPSILON
                       rule.  order="forward" | "reverse" sums over the matches front to back or back to front, so that the oracle can
                       state its own spread.

The reference's vfc.cpp needs OpenCV, which is not available to this project's build, so it cannot be compiled as an oracle binary; the
LU (modules/core/src/matrix_decomp.cpp LUImpl: first largest pivot, d = -1 / pivot, row updates left to right, back substitution that
multiplies by the stored reciprocal) and its singular thresholds are restated from memory of OpenCV 3 / 4 and flagged as such.
rand(): glibc's TYPE_3 generator, restated below; the control points use the first 48 values of srand(seed).
"""
from __future__ import annotations

import numpy as np

F = np.float32
THETA_F = F(0.75)
N_CTRL = 16
MAX_ITER = 50


def glibc_rand(seed: int, count: int) -> np.ndarray:
    """The first `count` values of srand(seed); rand() of glibc (TYPE_3 additive feedback)."""
    s = int(seed) & 0xFFFFFFFF
    if s == 0:
        s = 1
    s = s - (1 << 32) if s >= (1 << 31) else s
    r = [0] * (344 + count)
    r[0] = s
    for i in range(1, 31):
        hi, lo = int(r[i - 1] / 127773), int(np.fmod(r[i - 1], 127773))   # C division: truncation
        w = 16807 * lo - 2836 * hi
        if w < 0:
            w += 2147483647
        r[i] = w
    for i in range(31):
        r[i] &= 0xFFFFFFFF
    for i in range(31, 34):
        r[i] = r[i - 31]
    for i in range(34, 344 + count):
        r[i] = (r[i - 31] + r[i - 3]) & 0xFFFFFFFF
    return np.array([v >> 1 for v in r[344:]], np.int64)


def _ssum32(a: np.ndarray, axis: int = -1):
    """strictly serial float32 sum along `axis`, starting from 0"""
    a = np.asarray(a, F)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), F)
    return np.take(np.add.accumulate(a, axis=axis, dtype=F), -1, axis=axis)


def _ssum64(a: np.ndarray, axis: int = -1, reverse: bool = False):
    a = np.asarray(a, np.float64)
    if reverse:
        a = np.flip(a, axis=axis)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), np.float64)
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def normalize(x1: np.ndarray, x2: np.ndarray):
    """VFC::normalize (vfc.cpp:560-621) -> (X, Y) float32 [n, 2], or None when a scale is below 0.1."""
    l, r = np.array(x1, F).reshape(-1, 2), np.array(x2, F).reshape(-1, 2)
    n = l.shape[0]
    l = l - (_ssum32(l, 0) / F(n)).astype(F)
    r = r - (_ssum32(r, 0) / F(n)).astype(F)
    # s1 += pow(x, 2); s1 += pow(y, 2): a serial double sum of exact squares, x and y interleaved
    s1 = np.sqrt(_ssum64(l.astype(np.float64).reshape(-1) ** 2) / n)
    s2 = np.sqrt(_ssum64(r.astype(np.float64).reshape(-1) ** 2) / n)
    if F(s1) < 0.1 or F(s2) < 0.1:
        return None
    l = (l / F(s1)).astype(F)
    r = (r / F(s2)).astype(F)
    return l, (r - l).astype(F)


def select_subset(X: np.ndarray, raw: np.ndarray) -> np.ndarray:
    """VFC::selectSubset (vfc.cpp:130-150) -> indices of the control points."""
    n = X.shape[0]
    want = min(N_CTRL, n)
    chosen = []
    it = 0
    while len(chosen) < want and it < want * 3:
        idx = int(raw[it] % n)
        dist = np.inf
        for c in chosen:
            tmp = F(np.abs(F(X[c, 0] - X[idx, 0])) + np.abs(F(X[c, 1] - X[idx, 1])))
            dist = min(float(tmp), dist)
        if dist > 1e-3:
            chosen.append(idx)
        it += 1
    return np.array(chosen, np.int64)


def lu_solve(A: np.ndarray, B: np.ndarray, dtype):
    """cv::solve(A, B, C, DECOMP_LU) for a square A -> (C, singular).  From memory of OpenCV's LUImpl, see the module docstring."""
    dt = np.dtype(dtype).type
    eps = dt(np.finfo(dtype).eps * (10 if dtype == np.float32 else 100))
    A, B = np.array(A, dtype), np.array(B, dtype)
    m = A.shape[0]
    for i in range(m):
        k = i + int(np.argmax(np.abs(A[i:, i])))    # the first of equal maxima, as the reference's strict '>'
        if np.abs(A[k, i]) < eps:
            return np.zeros_like(B), True
        if k != i:
            A[[i, k]] = A[[k, i]]
            B[[i, k]] = B[[k, i]]
        d = dt(-1) / A[i, i]
        if i + 1 < m:
            alpha = (A[i + 1:, i] * d).astype(dtype)
            A[i + 1:, i + 1:] += (alpha[:, None] * A[i, i + 1:][None, :]).astype(dtype)
            B[i + 1:] += (alpha[:, None] * B[i][None, :]).astype(dtype)
        A[i, i] = -d
    for i in range(m - 1, -1, -1):
        s = B[i].copy()
        for k in range(i + 1, m):
            s -= (A[i, k] * B[k]).astype(dtype)
        B[i] = (s * A[i, i]).astype(dtype)
    return B, False


def _sq(a, b):
    """pow(a.x - b.x, 2) + pow(a.y - b.y, 2): float differences, squares and their sum in double"""
    d = (a - b).astype(F).astype(np.float64)
    return d[..., 0] ** 2 + d[..., 1] ** 2


def _result(n, keep, P, iters, m, refused=False, singular=0, sigma2=None):
    keep = np.asarray(keep, bool)
    kept = int(keep.sum())
    rc = -2 if kept / n < 0.1 else 0
    margin = float(np.min(np.abs(np.asarray(P, np.float64) - float(THETA_F)))) if iters > 0 else np.inf
    return dict(rc=rc, keep=keep, n_keep=kept, P=np.asarray(P, np.float64), iterations=iters, m=m, refused=refused, singular=singular,
                margin=margin, sigma2=sigma2)


def _em_float32(X, Y, ctrl):
    n, m = X.shape[0], ctrl.shape[0]
    beta, lam, a, gamma, ecr, minP, two_pi = F(0.1), F(3.0), F(10.0), F(0.9), F(1e-5), F(1e-5), F(6.283185)
    Xc = X[ctrl]
    K = np.exp((F(_sq(Xc[:, None, :], Xc[None, :, :])) * -beta).astype(F)).astype(F)     # expf
    np.fill_diagonal(K, F(1))
    U = np.exp((-beta * F(_sq(Xc[:, None, :], X[None, :, :]))).astype(F)).astype(F)
    V = np.zeros((n, 2), F)
    C = np.zeros((m, 2), F)
    P = np.ones(n, F)

    def sigma_square():
        t = F(_sq(Y, V))
        return F(_ssum32(P * t) / F(_ssum32(P) * F(2)))

    sigma2 = sigma_square()
    E, tecr, it, singular = F(1), F(1), 0, 0
    keep = np.ones(n, bool)
    while it < MAX_ITER and tecr > ecr and float(sigma2) > 1e-8:
        E_old = E
        # getP
        temp2 = F(F(F(two_pi * sigma2) * F(F(1) - gamma)) / F(gamma * a))     # powf(x, 1.0f) = x
        t = F(_sq(Y, V))
        temp1 = np.exp((-t / F(F(2) * sigma2)).astype(F)).astype(F)
        p = (temp1 / (temp1 + temp2).astype(F)).astype(F)
        P = np.maximum(minP, p)
        sumP = _ssum32(p)
        E = F(_ssum32((p * t).astype(F)) / F(F(2) * sigma2))
        E = F(E + F(F(F(sumP * F(np.log(sigma2))) * F(2)) / F(2)))
        # calculateTraceCKC
        KC = _ssum32((K[:, :, None] * C[None, :, :]).astype(F), 1)
        trace = F(0)
        for i in range(m):
            trace = F(trace + F(F(C[i, 0] * KC[i, 0]) + F(C[i, 1] * KC[i, 1])))
        E = F(E + F(F(lam / F(2)) * trace))
        with np.errstate(all="ignore"):
            tecr = np.abs(F(F(E - E_old) / E))
        # calculateC_SparseVFC
        PU = (P[None, :] * U).astype(F)
        A = _ssum32((PU[:, None, :] * U[None, :, :]).astype(F), 2)
        A = (A + (F(lam * sigma2) * K).astype(F)).astype(F)
        A = np.triu(A) + np.triu(A, 1).T
        B = _ssum32((PU[:, :, None] * Y[None, :, :]).astype(F), 1)
        C, sing = lu_solve(A, B, np.float32)
        singular += int(sing)
        # calculateV, calculateSigmaSquare, calculateGamma
        V = _ssum32((U.T[:, :, None] * C[None, :, :]).astype(F), 1)
        sigma2 = sigma_square()
        keep = P > THETA_F
        gamma = F(max(min(F(F(keep.sum()) / F(n)), F(0.95)), F(0.05)))
        it += 1
    return keep, P, it, singular, float(sigma2)


def _em_float64(X, Y, ctrl, reverse, iterations=None):
    n, m = X.shape[0], ctrl.shape[0]
    D = np.float64
    beta, lam, a, gamma, ecr, minP, two_pi = D(F(0.1)), 3.0, 10.0, D(F(0.9)), D(F(1e-5)), D(F(1e-5)), D(F(6.283185))
    X, Y = X.astype(D), Y.astype(D)
    Xc = X[ctrl]

    def sq(a_, b_):
        d = a_ - b_
        return d[..., 0] ** 2 + d[..., 1] ** 2

    K = np.exp(-beta * sq(Xc[:, None, :], Xc[None, :, :]))
    np.fill_diagonal(K, 1.0)
    U = np.exp(-beta * sq(Xc[:, None, :], X[None, :, :]))
    V = np.zeros((n, 2))
    C = np.zeros((m, 2))
    P = np.ones(n)

    def sigma_square():
        return _ssum64(P * sq(Y, V), reverse=reverse) / (_ssum64(P, reverse=reverse) * 2.0)

    sigma2 = sigma_square()
    E, tecr, it, singular = 1.0, 1.0, 0, 0
    keep = np.ones(n, bool)
    while (it < iterations and sigma2 > 1e-8) if iterations is not None else (it < MAX_ITER and tecr > ecr and sigma2 > 1e-8):
        E_old = E
        temp2 = two_pi * sigma2 * (1.0 - gamma) / (gamma * a)
        t = sq(Y, V)
        temp1 = np.exp(-t / (2.0 * sigma2))
        p = temp1 / (temp1 + temp2)
        P = np.maximum(minP, p)
        sumP = _ssum64(p, reverse=reverse)
        E = _ssum64(p * t, reverse=reverse) / (2.0 * sigma2) + sumP * np.log(sigma2)
        KC = _ssum64(K[:, :, None] * C[None, :, :], 1, reverse)
        E += lam / 2.0 * _ssum64((C * KC).sum(1), reverse=reverse)
        with np.errstate(all="ignore"):
            tecr = abs((E - E_old) / E)
        PU = P[None, :] * U
        A = _ssum64(PU[:, None, :] * U[None, :, :], 2, reverse) + lam * sigma2 * K
        A = np.triu(A) + np.triu(A, 1).T
        B = _ssum64(PU[:, :, None] * Y[None, :, :], 1, reverse)
        C, sing = lu_solve(A, B, np.float64)
        singular += int(sing)
        V = _ssum64(U.T[:, :, None] * C[None, :, :], 1, reverse)
        sigma2 = sigma_square()
        keep = P > D(THETA_F)
        gamma = max(min(keep.sum() / n, D(F(0.95))), D(F(0.05)))
        it += 1
    return keep, P, it, singular, float(sigma2)


def vfc(x1, x2, seed: int = 1, mode: str = "float64", order: str = "forward", iterations=None) -> dict:
    """filterWithVFC on the matched points x1[i] -> x2[i] (float32 [n, 2]).  Returns dict(rc, keep, n_keep, P, iterations, m, refused,
    singular, margin = min |P - 0.75| (inf when no iteration ran), sigma2); rc = 0, -1 (n < 5: keep is empty) or -2 (kept / n < 0.1).
    iterations (float64 only): run exactly that many EM iterations instead of the reference's energy stopping rule -- the rule is not a
    reproducible quantity (module docstring of test_oracle_vfc.py), so two evaluations are compared best at equal counts."""
    assert mode in ("float32_serial", "float64") and order in ("forward", "reverse")
    x1, x2 = np.array(x1, F).reshape(-1, 2), np.array(x2, F).reshape(-1, 2)
    n = x1.shape[0]
    if n < 5 or x2.shape[0] != n:
        return dict(rc=-1, keep=np.zeros(n, bool), n_keep=0, P=np.ones(n), iterations=0, m=0, refused=False, singular=0, margin=np.inf,
                    sigma2=None)
    nz = normalize(x1, x2)
    if nz is None:
        return _result(n, np.ones(n, bool), np.ones(n), 0, 0, refused=True)
    X, Y = nz
    ctrl = select_subset(X, glibc_rand(seed, 3 * N_CTRL))
    if mode == "float32_serial":
        keep, P, it, singular, s2 = _em_float32(X, Y, ctrl)
    else:
        keep, P, it, singular, s2 = _em_float64(X, Y, ctrl, order == "reverse", iterations)
    return _result(n, keep, P, it, len(ctrl), singular=singular, sigma2=s2)


def getmatches_rule(rc: int, n_keep: int, n: int) -> bool:
    """matchers.cpp:726-731: getMatches replaces finalMatches by the filtered list iff this holds."""
    return rc == 0 and (n_keep > 8 or n < 24)


def filter_matches(kp1, kp2, matches, seed: int = 1, rule: bool = False, mode: str = "float64"):
    """filterWithVFC on a DMatch list (structured array with queryIdx / trainIdx) -> (rc, filtered list); rule = getMatches' replacement
    rule; rc = -1 passes the list through (the device entries' convention)."""
    kp1, kp2 = np.asarray(kp1, F).reshape(-1, 2), np.asarray(kp2, F).reshape(-1, 2)
    r = vfc(kp1[matches["queryIdx"]], kp2[matches["trainIdx"]], seed, mode)
    if r["rc"] == -1 or (rule and not getmatches_rule(r["rc"], r["n_keep"], len(matches))):
        return r["rc"], matches.copy()
    return r["rc"], matches[r["keep"]].copy()
