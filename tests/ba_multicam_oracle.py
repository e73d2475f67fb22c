"""float64 numpy restatement of poselib::refineMultCamBA, pointsInImgCoords == false, optimMotionOnly == false (P/source/pose_estim.cpp:1384-1735):
motion and structure bundle adjustment of m cameras over one shared structure with the FIRST CAMERA FIXED AT THE POSE GIVEN, through
SBAdriver::perform_sba (P/source/BA_driver.cpp:1878-2260; nconstframes = 1, a visibility map per camera) and sba_motstr_levmar_x
(sba-1.6/sba_levmar.c:449-1400, mcon = 1) with the pseudo-Huber cost of BA_driver.cpp:2612-2648.

This is ba_oracle.py generalised; its quaternion, projection, cost and Jacobian helpers are imported, not copied, and what that file's header
says about the reference's arithmetic and about what is NOT the reference's (the Jacobian written from the quaternion algebra, the cofactor
inverse of V*_i, the unblocked upper Cholesky with sequential dot products) holds here unchanged.  What is new:

  * the parameter vector [3 local rotation + 3 translation] x m, then the points; EVERY camera's initial quaternion is normalised and
    sign-fixed, camera 0 included, and camera 0 projects through quat_mult_fast(local_quat(0), r0_0) and its own t;
  * the measurements are ordered point-major, cameras ascending within a point (perform_sba's mask2Dpts loop, BA_driver.cpp:2121-2157); the
    norm of the residual (nrmL2xmy) walks that order;
  * sums, as sba_levmar.c:841-1260 has them: U_j, ea_j over the points camera j sees, ascending, j >= 1 only; V_i, eb_i over the cameras that
    see point i, ascending, camera 0 included; W_ij for j >= 1 only; Y_ij = W_ij (V*_i)^-1; S_jk = delta_jk U*_j - sum_i Y_ij W_ik^T over the
    points seen by both, ascending; e_j = ea_j - sum_i Y_ij eb_i; db_i = (V*_i)^-1 (eb_i - sum_j W_ij^T da_j), the inner products summed per
    camera and the cameras added in ascending order;
  * mu starts from the largest of diag(U_j, j >= 1) and diag(V_i); the damping quirk of ba_oracle.py (every earlier rejected mu stays on U's
    diagonal, V_i's diagonal holds the previous attempt's inverse's) is the same code path in the reference and is kept;
  * ||p||^2, ||dp||^2 and dL over the full vector in its order: camera 0's three translation entries are part of ||p||^2, its six entries of
    dp and of J^T e are zero;
  * the optimiser refuses when nobs < nvars with nvars = 6 m + 3 n, the fixed camera counted (sba_levmar.c:611-616); info stays zero;
  * the reduced camera system has size 6 (m - 1);
  * the wrapper (pose_estim.cpp:1400-1735): th = th_px / mean_j((K_j(1,1) + K_j(2,2)) / 2); failure when the optimiser refuses or stops for
    a reason > 5; per camera getRTQuality between the old and the new quaternion and between the old and the new translation, BOTH
    normalised when their norm is not near zero and differs from 1 by more than 1e-4; rejection when any camera exceeds angle_thresh degrees
    or t_norm_thresh; on rejection every t is restored and R, Q stay; on success Q is replaced whole, every R_j (camera 0 included) is
    quatToMatrix of its quaternion and every t_j is what the optimiser left, NOT normalised.

A point that no camera sees has V_i = 0, eb_i = 0: V*_i = mu I inverts, db_i = 0 and the point keeps its coordinates.
"""
import numpy as np

import ba_oracle as BAO
from ba_oracle import (DBL_MIN, EPSILON_SQ, MAXITER, ONE_THIRD, OPTS, ROBUST_THRESH, jacobian, jte_inf_norm, local_quat, mat_to_quat,
                       project, pull_to_measurement, quat_mult_fast, quat_to_matrix, rt_quality, seqsum)

MAX_CAMS = 16       # MLPL_BA_MAX_CAMS: the device's cap, not the oracle's


def chol_solve(S, b):
    """ba_oracle._chol_solve6 at any size: upper Cholesky U^T U = S (upper triangle read) with sequential dot products, U^T y = b, U x = y."""
    d = S.shape[0]
    U = np.zeros((d, d))
    for j in range(d):
        ajj = S[j, j]
        for i in range(j):
            ajj = ajj - U[i, j] * U[i, j]
        if not (ajj > 0.0) or not np.isfinite(ajj):
            return False, None
        ajj = np.sqrt(ajj)
        U[j, j] = ajj
        r = 1.0 / ajj
        if j + 1 < d:
            s = S[j, j + 1:].copy()
            for i in range(j):
                s = s - U[i, j] * U[i, j + 1:]
            U[j, j + 1:] = s * r
    y = np.zeros(d)
    for j in range(d):
        s = b[j]
        for i in range(j):
            s = s - U[i, j] * y[i]
        y[j] = s / U[j, j]
    x = np.zeros(d)
    for j in range(d - 1, -1, -1):
        s = y[j]
        for i in range(j + 1, d):
            s = s - U[j, i] * x[i]
        x[j] = s / U[j, j]
    return True, x


def sba_motstr_multicam(x, vis, r0, t, M, th, itmax=MAXITER, opts=OPTS):
    """sba_motstr_levmar_x for m frames with the first fixed.  x [m, n, 2] (read where vis), vis [m, n] bool, r0 [m, 4], t [m, 3], M [n, 3]
    -> dict(ok, v [m, 3], t [m, 3], M, info[10], mu, trace, attempts, almost_singular) as ba_oracle.sba_motstr returns them."""
    m, n = vis.shape
    info = np.zeros(10)
    out = dict(ok=False, v=np.zeros((m, 3)), t=np.array(t, np.float64), M=np.array(M, np.float64), info=info, mu=0.0, trace=[], attempts=[],
               almost_singular=False)
    nvis = int(vis.sum())
    nobs, nvars = 2 * nvis, 6 * m + 3 * n
    if nobs < nvars:
        return out
    tau, eps1, eps2 = abs(opts[0]), abs(opts[1]), abs(opts[2])
    eps2_sq, eps3_sq, eps4_sq = opts[2] * opts[2], opts[3] * opts[3], opts[4] * opts[4]
    order = BAO._norm_order(nobs)
    pts = [np.flatnonzero(vis[j]) for j in range(m)]                       # the points camera j sees, ascending
    rank = (np.cumsum(vis.T.reshape(-1)) - 1).reshape(n, m).T              # the measurement's place in the point-major order
    meas = [rank[j][pts[j]] for j in range(m)]
    xs = [np.asarray(x[j], np.float64)[pts[j]] for j in range(m)]
    pos = []                                                               # point -> its place in camera j's list
    for j in range(m):
        p = np.full(n, -1, np.int64)
        p[pts[j]] = np.arange(pts[j].size)
        pos.append(p)
    dim = 6 * (m - 1)

    def residual(v, tt, MM):
        e = np.zeros((nvis, 2))
        for j in range(m):
            h = pull_to_measurement(project(quat_mult_fast(local_quat(v[j]), r0[j]), tt[j], MM[pts[j]]), xs[j], th)
            e[meas[j]] = xs[j] - h
        return e, BAO._sq_norm(e.reshape(-1), order)

    v, t, M = np.zeros((m, 3)), np.array(t, np.float64).reshape(m, 3), np.array(M, np.float64)
    with np.errstate(all="ignore"):
        e, p_eL2 = residual(v, t, M)
    init_p_eL2 = p_eL2
    nfev, njev, nlss, nu, stop = 1, 0, 0, 2, 0
    mu = eab_inf = 0.0
    dp_L2 = np.finfo(np.float64).max
    if not np.isfinite(p_eL2):
        stop = 7
    diagU, diagV = np.zeros((m, 6)), np.zeros((n, 3))
    have_diag = False
    itno = 0
    while itno < itmax and not stop:
        A, B = [], []
        for j in range(m):
            Aj, Bj = jacobian(r0[j], v[j], t[j], M[pts[j]])
            A.append(Aj)
            B.append(Bj)
        njev += 1
        U, ea = np.zeros((m, 6, 6)), np.zeros((m, 6))
        for j in range(1, m):
            ej = e[meas[j]]
            for ii in range(6):
                for jj in range(ii, 6):
                    U[j, ii, jj] = seqsum(A[j][:, 0, ii] * A[j][:, 0, jj] + A[j][:, 1, ii] * A[j][:, 1, jj])
                    U[j, jj, ii] = U[j, ii, jj]
                ea[j, ii] = seqsum(A[j][:, 0, ii] * ej[:, 0] + A[j][:, 1, ii] * ej[:, 1])
        Vu, Vd, eb = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        for j in range(m):                                                 # per point: the cameras in ascending order
            ej, Bj, at = e[meas[j]], B[j], pts[j]
            for ii in range(3):
                for jj in range(ii, 3):
                    val = Bj[:, 0, ii] * Bj[:, 0, jj] + Bj[:, 1, ii] * Bj[:, 1, jj]
                    if ii == jj:
                        Vd[at, ii] = Vd[at, ii] + val
                    else:
                        Vu[at, ii + jj - 1] = Vu[at, ii + jj - 1] + val
                eb[at, ii] = eb[at, ii] + (Bj[:, 0, ii] * ej[:, 0] + Bj[:, 1, ii] * ej[:, 1])
        W = [None] * m
        for j in range(1, m):
            Wj = np.zeros((pts[j].size, 6, 3))
            for ii in range(6):
                for jj in range(3):
                    Wj[:, ii, jj] = A[j][:, 0, ii] * B[j][:, 0, jj] + A[j][:, 1, ii] * B[j][:, 1, jj]
            W[j] = Wj
        eab_inf = jte_inf_norm(ea.reshape(-1), eb)
        pvec = np.concatenate([np.concatenate([v, t], axis=1).reshape(-1), M.reshape(-1)])
        p_L2 = float(seqsum(pvec * pvec))
        diagU, diagV, have_diag = np.array([np.diag(U[j]) for j in range(m)]), Vd.copy(), True
        if eab_inf <= eps1:
            dp_L2 = 0.0
            stop = 1
            break
        if itno == 0:
            tmp = DBL_MIN
            for val in list(diagU[1:].reshape(-1)) + list(diagV.reshape(-1)):
                if val > tmp:
                    tmp = val
            mu = tau * tmp
        while True:
            mu_used = mu
            for j in range(1, m):
                for i in range(6):
                    U[j, i, i] += mu
            trial = Vd + mu
            ok, inv = BAO._invert_sym3(trial, Vu)
            if not ok.all():
                f = int(np.argmin(ok))
                Vd[:f] = inv[:f][:, [0, 3, 5]]
                Vd[f] = trial[f]
                out["trace"].append((mu_used, p_eL2, False))
                out["attempts"].append((itno, f, False, False))
            else:
                Vd = inv[:, [0, 3, 5]].copy()
                im = inv[:, np.array(BAO._SYM)]                            # [n, 3, 3]
                S, E = np.zeros((dim, dim)), np.zeros(dim)
                Y = [None] * m
                for j in range(1, m):
                    imj = im[pts[j]]
                    Yj = np.zeros((pts[j].size, 6, 3))
                    for ii in range(6):
                        for jj in range(3):
                            Yj[:, ii, jj] = W[j][:, ii, 0] * imj[:, 0, jj] + W[j][:, ii, 1] * imj[:, 1, jj] + W[j][:, ii, 2] * imj[:, 2, jj]
                    Y[j] = Yj
                for j in range(1, m):
                    for k in range(j, m):
                        both = pts[j][pos[k][pts[j]] >= 0]                 # seen by j and k, ascending
                        Yb, Wb = Y[j][pos[j][both]], W[k][pos[k][both]]
                        ywt = seqsum(Yb[:, :, None, 0] * Wb[:, None, :, 0] + Yb[:, :, None, 1] * Wb[:, None, :, 1]
                                     + Yb[:, :, None, 2] * Wb[:, None, :, 2]) if both.size else np.zeros((6, 6))
                        blk = (U[j] - ywt) if j == k else -ywt
                        S[6 * (j - 1):6 * j, 6 * (k - 1):6 * k] = blk
                    ebj = eb[pts[j]]
                    ye = seqsum(Y[j][:, :, 0] * ebj[:, None, 0] + Y[j][:, :, 1] * ebj[:, None, 1] + Y[j][:, :, 2] * ebj[:, None, 2])
                    E[6 * (j - 1):6 * j] = ea[j] - ye
                solved, da_free = chol_solve(S, E)
                nlss += 1
                accepted = False
                if solved:
                    da = np.concatenate([np.zeros((1, 6)), da_free.reshape(m - 1, 6)])
                    wtda = np.zeros((n, 3))
                    for j in range(1, m):
                        for ii in range(3):
                            s = W[j][:, 0, ii] * da[j, 0]
                            for jj in range(1, 6):
                                s = s + W[j][:, jj, ii] * da[j, jj]
                            wtda[pts[j], ii] = wtda[pts[j], ii] + s
                    r = eb - wtda
                    db = np.zeros((n, 3))
                    for ii in range(3):
                        db[:, ii] = im[:, ii, 0] * r[:, 0] + im[:, ii, 1] * r[:, 1] + im[:, ii, 2] * r[:, 2]
                    dp = np.concatenate([da.reshape(-1), db.reshape(-1)])
                    eab = np.concatenate([ea.reshape(-1), eb.reshape(-1)])
                    dp_L2 = float(seqsum(dp * dp))
                    v_new, t_new, M_new = v + da[:, :3], t + da[:, 3:], M + db
                    if dp_L2 <= eps2_sq * p_L2:
                        stop = 2
                        out["attempts"].append((itno, -1, False, False))
                        break
                    if dp_L2 >= (p_L2 + eps2) / EPSILON_SQ:
                        out["almost_singular"] = True
                        return out
                    with np.errstate(all="ignore"):
                        e_new, pdp_eL2 = residual(v_new, t_new, M_new)
                    nfev += 1
                    if not np.isfinite(pdp_eL2):
                        stop = 7
                        out["attempts"].append((itno, -1, False, False))
                        break
                    dL = float(seqsum(dp * (mu * dp + eab)))
                    dF = p_eL2 - pdp_eL2
                    if dL > 0.0 and dF > 0.0:
                        tmp = 2.0 * dF / dL - 1.0
                        tmp = 1.0 - tmp * tmp * tmp
                        mu = mu * (tmp if tmp >= ONE_THIRD else ONE_THIRD)
                        nu = 2
                        if pdp_eL2 - 2.0 * np.sqrt(p_eL2 * pdp_eL2) < (eps4_sq - 1.0) * p_eL2:
                            stop = 4
                        v, t, M, e, p_eL2 = v_new, t_new, M_new, e_new, pdp_eL2
                        accepted = True
                    out["trace"].append((mu_used, pdp_eL2, accepted))
                    out["attempts"].append((itno, -1, False, accepted))
                else:
                    out["trace"].append((mu_used, p_eL2, False))
                    out["attempts"].append((itno, -1, True, False))
                if accepted:
                    break
            mu *= nu
            nu2 = nu * 2
            if nu2 >= 2 ** 31:
                stop = 6
                break
            nu = nu2
        if p_eL2 <= eps3_sq:
            stop = 5
        itno += 1
    if itno >= itmax:
        stop = 3
    info[0], info[1], info[2], info[3] = init_p_eL2, p_eL2, eab_inf, dp_L2
    if have_diag:
        tmp = DBL_MIN
        for val in list(diagU[1:].reshape(-1)) + list(diagV.reshape(-1)):
            if tmp < val:
                tmp = val
        info[4] = mu / tmp
    info[5], info[6], info[7], info[8], info[9] = itno, stop, nfev, njev, nlss
    out.update(ok=(stop != 7), v=v, t=t, M=M, mu=mu)
    return out


# ---- the wrapper --------------------------------------------------------------------------------------------------------------------------------
def convert_threshold_multicam(Ks, huber_thresh=-1.0):
    """pose_estim.cpp:1510-1514, :1566-1571 -- (1,1) and (2,2), as the reference indexes: (fy + 1) / 2 per camera."""
    th = huber_thresh if huber_thresh >= 0 else ROBUST_THRESH
    f_mean = 0.0
    for K in Ks:
        K = np.asarray(K, np.float64)
        f_mean += (K[1, 1] + K[2, 2]) / 2.0
    f_mean /= float(len(Ks))
    return th / f_mean


def _unit_or_kept(t):
    t_norm = np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    if not (-1e-3 < t_norm < 1e-3) and abs(t_norm - 1.0) > 1e-4:           # nearZero of pose_helper.h:82-87
        return t / t_norm
    return t


def ba_multicam_oracle(p, vis, R, t, Q, th, angle_thresh=1.25, t_norm_thresh=0.05):
    """mlpl_refine_multicam_ba: p [m, n, 2] in camera coordinates (read where vis), vis [m, n], R [m, 3, 3], t [m, 3], Q [n, 3], th in CAMERA
    units.  -> dict(accepted, R, t, Q, quat [m, 4] (the refined quaternions), t_opt (t as the optimiser left it, accepted or not), info, mu,
    trace, attempts, refused_by); on rejection or failure R, t, Q equal the inputs."""
    p = np.asarray(p, np.float64)
    vis = np.asarray(vis).astype(bool)
    m, n = vis.shape
    R0, t0, Q0 = np.array(R, np.float64).reshape(m, 3, 3), np.array(t, np.float64).reshape(m, 3), np.array(Q, np.float64).reshape(n, 3)
    res = dict(accepted=False, R=R0.copy(), t=t0.copy(), Q=Q0.copy(), quat=None, t_opt=t0.copy(), info=np.zeros(10), mu=0.0, trace=[],
               attempts=[], refused_by=())
    if n == 0 or m < 2:
        return res
    quat_old = np.array([mat_to_quat(R0[j]) for j in range(m)])
    r0 = np.zeros((m, 4))
    for j in range(m):
        q = quat_old[j]
        mag = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
        mag = (1.0 if q[0] >= 0.0 else -1.0) / mag
        r0[j] = q * mag
    o = sba_motstr_multicam(p.reshape(m, n, 2), vis, r0, t0, Q0, th)
    res.update(info=o["info"], mu=o["mu"], trace=o["trace"], attempts=o["attempts"])
    if not o["ok"]:
        return res
    quat_new = np.zeros((m, 4))
    for j in range(m):
        q = quat_mult_fast(local_quat(o["v"][j]), r0[j])
        quat_new[j] = q * -1.0 if q[0] < 0.0 else q
    res.update(quat=quat_new, t_opt=o["t"].copy())
    hits = []
    if o["info"][6] > 5:
        hits.append("stop")
    else:
        for j in range(m):
            r_diff, t_diff = rt_quality(quat_old[j], quat_new[j], _unit_or_kept(t0[j]), _unit_or_kept(o["t"][j]))
            r_diff = r_diff / np.pi * 180.0
            if abs(r_diff) > angle_thresh or t_diff > t_norm_thresh:
                hits.append(("angle" if abs(r_diff) > angle_thresh else "t_norm", j))
                break
    res["refused_by"] = tuple(hits)
    if hits:
        return res
    res.update(accepted=True, R=np.array([quat_to_matrix(quat_new[j]) for j in range(m)]), t=o["t"].copy(), Q=o["M"].copy())
    return res


def refine_mult_cam_ba(ps, map3D, Rs, ts, Q, Ks, angle_thresh=1.25, t_norm_thresh=0.05, huber_thresh=-1.0):
    """poselib::refineMultCamBA(ps, map3D, Rs, ts, Q, Ks, false, noArray(), ...): ps[j] holds camera j's observations in ascending point order
    for the non-zero entries of map3D[j].  Fewer than 15 points: refused (None)."""
    n = np.asarray(Q).reshape(-1, 3).shape[0]
    if n < 15:
        return None
    m = len(ps)
    vis = np.array([np.asarray(mp).reshape(-1) != 0 for mp in map3D])
    p = np.zeros((m, n, 2))
    for j in range(m):
        p[j, vis[j]] = np.asarray(ps[j], np.float64).reshape(-1, 2)
    return ba_multicam_oracle(p, vis, Rs, ts, Q, convert_threshold_multicam(Ks, huber_thresh), angle_thresh, t_norm_thresh)
