"""CPU restatement of poselib::getPoseTriangPts = recoverPose (five-point.cpp:150-338) over the oracle's decomposition and triangulation
(oracle_decompose_essential, oracle_triangulate_point) -- the checker of mlpl_recover_pose, its device, translation and batch forms with
every intermediate result in the open.  TEST INFRASTRUCTURE ONLY; it is pinned by the C oracle (oracle_recover_pose*, test_oracle_recover_pose.py),
not the other way round.

P0 = [I|0]; the candidates are [R1|t] [R2|t] [R1|-t] [R2|-t] of decomposeEssentialMat.  Per candidate and correspondence X = the unit DLT null
vector, m = X.z * X.w > 0 && (P X).z * X.w > 0 && X.z / X.w < dist (w = 0 gives inf / NaN and a false comparison), the mask byte is
(m ? 255 : 0) & the incoming byte (None = 255), so an incoming 1 stays 1; a candidate's count is the number of its nonzero bytes and
Q = X.xyz / X.w by division.  The if-chain of five-point.cpp:299-336 then picks one candidate:

    good1 >= all                 -> 0
    good2 && good2 >= all        -> 1
    good3 >= all                 -> 2
    else                         -> good4 ? 3 : -1   (R = I, t = 0, Q and the mask zeroed)

With non-negative counts the `good2 &&` and the -1 tail cannot decide anything (all counts zero is caught by the first branch, and the else
is reached only when good4 is the strict maximum); they are restated for the record.

The translation-only form (t_only: recoverPose with R1 = I) tests [I|t] and [I|-t] alone: the counts of candidates 1 and 3 are zero.

`margin` is the smallest distance of a compared quantity from its threshold over all correspondences and all tested candidates:
|X.z * X.w|, |(P X).z * X.w| (X has unit norm, so the products are already relative) and |z - dist| / dist where the quotient z is finite."""
import ctypes as C

import numpy as np


def t_from_translation_essential(E):
    """getTfromTransEssential (pose_helper.cpp:422-433) as oracle_recover_pose_translation has it: t = (E12, E20, E01), normalised unless its
    length is within 1e-3 of one."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    tv = np.array([E[1, 2], E[2, 0], E[0, 1]])
    nrm = np.sqrt(tv[0] * tv[0] + tv[1] * tv[1] + tv[2] * tv[2])
    if abs(nrm - 1.0) > 1e-3:
        tv = tv / nrm
    return tv


def candidates(oracle, E, p1, p2, translation=False):
    """The part that depends on neither the mask nor the distance -> dict(R [4, 3, 3], t [4, 3], P [4, 3, 4], X [4, n, 4], tested [4] bool)."""
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 2)
    n = p1.shape[0]
    if translation:
        tv = t_from_translation_essential(E)
        R1 = R2 = np.eye(3)
    else:
        R1, R2, tv = oracle.decompose_essential(np.asarray(E, np.float64).reshape(3, 3))
    Rs = np.stack([R1, R2, R1, R2])
    ts = np.stack([tv, tv, -tv, -tv])
    tested = np.array([True, not translation, True, not translation])
    P0 = np.ascontiguousarray(np.hstack([np.eye(3), np.zeros((3, 1))]))
    P = np.ascontiguousarray(np.concatenate([Rs, ts[:, :, None]], axis=2))
    X = np.zeros((4, max(n, 1), 4))
    tri = oracle.lib.oracle_triangulate_point
    a0, a1, a2 = P0.ctypes.data, p1.ctypes.data, p2.ctypes.data
    for c in range(4):
        if not tested[c]:
            continue
        ac, ax = P[c].ctypes.data, X[c].ctypes.data
        for i in range(n):
            tri(C.c_void_p(a0), C.c_void_p(ac), C.c_void_p(a1 + 16 * i), C.c_void_p(a2 + 16 * i), C.c_void_p(ax + 32 * i))
    return dict(R=Rs, t=ts, P=P, X=X[:, :n], tested=tested, n=n)


def decide(cand, mask=None, dist=50.0):
    """-> dict(pick, n_good, R, t, Q [n, 3], mask (uint8 [n]: the updated incoming mask, or the 0 / 255 result when none was passed),
    counts [4], masks [4, n], Qs [4, n, 3], margin)."""
    n, P, X = cand["n"], cand["P"], cand["X"]
    m_in = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    masks, Qs, margin = np.zeros((4, n), np.uint8), np.zeros((4, n, 3)), np.inf
    for c in range(4):
        if not cand["tested"][c]:
            continue
        x, y, z, w = X[c, :, 0], X[c, :, 1], X[c, :, 2], X[c, :, 3]
        front1 = z * w
        front2 = (P[c, 2, 0] * x + P[c, 2, 1] * y + P[c, 2, 2] * z + P[c, 2, 3] * w) * w
        with np.errstate(all="ignore"):
            Qs[c] = np.stack([x / w, y / w, z / w], axis=1)
            ok = (front1 > 0) & (front2 > 0) & (Qs[c, :, 2] < dist)
        masks[c] = np.where(ok, 255, 0).astype(np.uint8)
        if m_in is not None:
            masks[c] &= m_in
        if n:
            fin = np.isfinite(Qs[c, :, 2])
            margin = min(margin, np.abs(front1).min(), np.abs(front2).min())
            if fin.any():
                margin = min(margin, (np.abs(Qs[c, fin, 2] - dist) / dist).min())
    counts = [int(np.count_nonzero(masks[c])) for c in range(4)]
    good1, good2, good3, good4 = counts
    if good1 >= good2 and good1 >= good3 and good1 >= good4:
        pick, ret = 0, good1
    elif good2 and good2 >= good1 and good2 >= good3 and good2 >= good4:
        pick, ret = 1, good2
    elif good3 >= good1 and good3 >= good2 and good3 >= good4:
        pick, ret = 2, good3
    else:
        pick, ret = (3 if good4 else -1), good4
    if pick >= 0:
        R, t, Q, m = cand["R"][pick].copy(), cand["t"][pick].copy(), Qs[pick].copy(), masks[pick].copy()
    else:
        R, t, Q, m = np.eye(3), np.zeros(3), np.zeros((n, 3)), np.zeros(n, np.uint8)
    return dict(pick=pick, n_good=ret, R=R, t=t, Q=Q, mask=m, counts=counts, masks=masks, Qs=Qs, margin=float(margin))


def recover_pose(oracle, E, p1, p2, mask=None, dist=50.0):
    return decide(candidates(oracle, E, p1, p2), mask, dist)


def recover_pose_translation(oracle, Et, p1, p2, mask=None, dist=50.0):
    return decide(candidates(oracle, Et, p1, p2, translation=True), mask, dist)
