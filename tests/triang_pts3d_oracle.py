"""CPU restatement of poselib::triangPts3D (P/source/pose_estim.cpp:964-1044) over the oracle's triangulation (oracle_triangulate_point,
the cv::triangulatePoints restatement oracle_recover_pose runs) -- the checker of mlpl_triang_pts3d*.  TEST INFRASTRUCTURE ONLY.

P0 = [I|0], P1 = [R|t]; per correspondence X = the unit DLT null vector; m = ((P1 X).z * X.w > 0), AND-ed bytewise with the incoming mask
(None = all points); Q = X.xyz / X.w by division (w = 0 gives inf / NaN, every comparison then false); m &= (Q.z < dist) & (Q.z > 0).
Mask bytes are in & (m ? 255 : 0), so an incoming 1 stays 1; the return value counts the nonzero bytes.  Q is written for every point.
`margin` is the smallest distance of a compared quantity from its threshold over the points whose quotient is finite: |z - dist| / dist,
|z| / dist and |qz * w| (X has unit norm, so the product is already relative)."""
import ctypes as C

import numpy as np


def triang_pts3d(oracle, R, t, p1, p2, mask=None, dist=50.0):
    """-> dict(n_good, Q [n, 3], mask (uint8 [n]: the updated incoming mask, or the 0 / 255 result when none was passed), margin)."""
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 2)
    n = p1.shape[0]
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    P0 = np.ascontiguousarray(np.hstack([np.eye(3), np.zeros((3, 1))]))
    P1 = np.ascontiguousarray(np.hstack([R, t[:, None]]))
    m_in = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    Q = np.zeros((n, 3))
    out = np.zeros(n, np.uint8)
    X = np.zeros(4)
    margin = np.inf
    tri = oracle.lib.oracle_triangulate_point
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for i in range(n):
        tri(ptr(P0), ptr(P1), ptr(p1[i]), ptr(p2[i]), ptr(X))
        qz = P1[2, 0] * X[0] + P1[2, 1] * X[1] + P1[2, 2] * X[2] + P1[2, 3] * X[3]
        ok = qz * X[3] > 0
        with np.errstate(all="ignore"):
            q = np.array([X[0] / X[3], X[1] / X[3], X[2] / X[3]])
        ok = bool(ok and q[2] < dist and q[2] > 0)
        Q[i] = q
        if np.all(np.isfinite(q)):
            margin = min(margin, abs(q[2] - dist) / dist, abs(q[2]) / dist, abs(qz * X[3]))
        mv = 255 if ok else 0
        if m_in is not None:
            mv &= int(m_in[i])
        out[i] = mv
    return dict(n_good=int(np.count_nonzero(out)), Q=Q, mask=out, margin=float(margin))
