"""float64 numpy restatement of poselib::refineStereoBA, pointsInImgCoords == false (P/source/pose_estim.cpp:1083-1206, :1294-1348): motion and
structure bundle adjustment of one stereo pair with the first camera fixed, through SBAdriver::perform_sba (P/source/BA_driver.cpp:1878-2260)
and sba_motstr_levmar_x (sba-1.6/sba_levmar.c:449-1400) with the pseudo-Huber cost of BA_driver.cpp:2612-2648.

What is restated as the reference has it
  * the parameter vector [3 local rotation + 3 translation] per frame, then the points; the initial quaternion normalised and sign-fixed, local
    rotations starting at 0; the composition local * initial by the nine-product quaternion multiplication of BA_driver.cpp:153-185;
  * the projection q (0, M) q* + t divided by its z through ONE reciprocal (imgproj.c:181-217), with that file's association;
  * the robust cost: the PREDICTED projection is pulled towards the measurement inside the function evaluation only
    (est = (1 - w) meas + w est, w = sqrt(2 b^2 (sqrt(1 + ((|d| + 1e-12) / b)^2) - 1)) / (|d| + 1e-12)); the Jacobian stays the plain one;
  * the optimiser: U, V, W, ea, eb; ||J^T e||_inf and ||p||^2; mu = tau * max diag on the first iteration; the damping loop, which adds mu onto
    what earlier REJECTED attempts left behind (the diagonal restore at sba_levmar.c:1341-1355 is compiled out): U's diagonal keeps every
    earlier mu, and V_i's diagonal holds the diagonal of the previous attempt's (V*_i)^-1, because the inverse is stored in V_i's lower
    triangle, diagonal included; Y = W V*^-1, S = U* - sum Y W^T, the right-hand side ea - sum Y eb, Cholesky, db_i; stopping tests 1-7 in
    their order; the "almost singular" error return; gain ratio, mu / nu update; the stop = 4 test; the stop = 5 test behind the damping loop
    (it overrides 2 and 7); stop = 3; info[0..9];
  * every sum over points runs sequentially in ascending point order, ||e||^2 in the order of nrmL2xmy (four accumulators over blocks of eight
    walked downwards, the tail upwards into the first), ||p||^2, ||dp||^2 and dL over the parameter vector in its order;
  * the wrapper: mask compaction, MatToQuat, the normalisation of t, getRTQuality, the rejection rule, the scatter back, quatToMatrix.

What is NOT the reference's text or arithmetic (no SBA build stands behind this file; test_oracle_bundle_adjust.py pins it instead)
  * the Jacobian is the analytic derivative of the projection above written from the quaternion algebra (d/dv_k of q M q* = 2 vec(dq_k M q*),
    d/dM = the matrix of the quadratic form, NOT normalised), not the computer-algebra output of imgproj.c:1134; equal up to rounding;
  * (V*_i)^-1 is the cofactor inverse, singular when the determinant is 0 or not finite, where the reference runs LAPACK's pivoted LDL^T;
  * the 6 x 6 system is an unblocked upper Cholesky with sequential dot products and two triangular solves by division.
  * a failed run (fewer measurements than unknowns, i.e. fewer than 12 points; the almost-singular return) leaves info[] all zero here; the
    reference leaves it unwritten.

Beside its results a run reports which way it went, for the tests that must know that a scene reaches the branch it is named for: `attempts`
(per damping attempt the first V*_i that did not invert, a refused Cholesky, the verdict) and `branch` (MatToQuat's pivot, the two sign fixes,
the case of |t|, the rules that refused).  None of it feeds back into the arithmetic.
"""
import numpy as np

ROBUST_THRESH = 0.005
OPTS = (1e-3, 1e-12, 1e-12, 1e-12, 1e-5)
MAXITER = 150
EPSILON_SQ = 1e-12 * 1e-12
ONE_THIRD = 0.3333333334
DBL_MIN = np.finfo(np.float64).tiny


def seqsum(x):
    """Sum along axis 0 strictly left to right (np.sum is pairwise)."""
    x = np.asarray(x, np.float64)
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:])
    return np.add.accumulate(x, axis=0)[-1]


# ---- quaternions ----------------------------------------------------------------------------------------------------------------------------
def quat_mult_fast(a, b):
    t1 = (a[0] + a[1]) * (b[0] + b[1])
    t2 = (a[3] - a[2]) * (b[2] - b[3])
    t3 = (a[1] - a[0]) * (b[2] + b[3])
    t4 = (a[2] + a[3]) * (b[1] - b[0])
    t5 = (a[1] + a[3]) * (b[1] + b[2])
    t6 = (a[1] - a[3]) * (b[1] - b[2])
    t7 = (a[0] + a[2]) * (b[0] - b[3])
    t8 = (a[0] - a[2]) * (b[0] + b[3])
    t9 = 0.5 * (t5 - t6 + t7 + t8)
    return np.array([t2 + t9 - t5, t1 - t9 - t6, -t3 + t9 - t8, -t4 + t9 - t7])


def qmul(a, b):
    """Plain Hamilton product; the components may be arrays."""
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])


def local_quat(v):
    return np.array([np.sqrt(1.0 - v[0] * v[0] - v[1] * v[1] - v[2] * v[2]), v[0], v[1], v[2]])


def mat_to_quat(R):
    R = np.asarray(R, np.float64).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr > 0.0:
        root = np.sqrt(tr + 1.0)
        q[0] = 0.5 * root
        root = 0.5 / root
        q[1] = (R[2, 1] - R[1, 2]) * root
        q[2] = (R[0, 2] - R[2, 0]) * root
        q[3] = (R[1, 0] - R[0, 1]) * root
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        root = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i + 1] = 0.5 * root
        root = 0.5 / root
        q[0] = (R[k, j] - R[j, k]) * root
        q[j + 1] = (R[j, i] + R[i, j]) * root
        q[k + 1] = (R[k, i] + R[i, k]) * root
    return q


def mat_to_quat_pivot(R):
    """Which branch mat_to_quat takes: -1 for tr > 0, else the index i of the largest diagonal entry as that function picks it."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0.0:
        return -1
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return i


def quat_to_matrix(q):
    sw, sx, sy, sz = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    invs = 1 / (sx + sy + sz + sw)
    R = np.zeros((3, 3))
    R[0, 0] = (sx - sy - sz + sw) * invs
    R[1, 1] = (-sx + sy - sz + sw) * invs
    R[2, 2] = (-sx - sy + sz + sw) * invs
    a, b = q[1] * q[2], q[3] * q[0]
    R[1, 0] = 2.0 * (a + b) * invs
    R[0, 1] = 2.0 * (a - b) * invs
    a, b = q[1] * q[3], q[2] * q[0]
    R[2, 0] = 2.0 * (a - b) * invs
    R[0, 2] = 2.0 * (a + b) * invs
    a, b = q[2] * q[3], q[1] * q[0]
    R[2, 1] = 2.0 * (a + b) * invs
    R[1, 2] = 2.0 * (a - b) * invs
    return R


def _rot_conj_pt(q, p):
    """quatMult3DPt(quatConj(q), p) of pose_helper.cpp."""
    c = (q[0], -q[1], -q[2], -q[3])
    s1 = c[2] * p[2] - c[3] * p[1] + c[0] * p[0]
    s2 = c[3] * p[0] - c[1] * p[2] + c[0] * p[1]
    s3 = c[1] * p[1] - c[2] * p[0] + c[0] * p[2]
    s0 = -(c[1] * p[0] + c[2] * p[1] + c[3] * p[2])
    return np.array([((s3 * c[2] - s2 * c[3]) - s0 * c[1]) + c[0] * s1,
                     ((s1 * c[3] - s3 * c[1]) - s0 * c[2]) + c[0] * s2,
                     ((s2 * c[1] - s1 * c[2]) - s0 * c[3]) + c[0] * s3])


def rt_quality(q_a, q_b, t_a, t_b):
    """getRTQuality(q_a, q_b, t_a, t_b) -> (rotation difference in rad, norm of the translation difference)."""
    d = np.array([q_a[1] * q_b[1] + q_a[2] * q_b[2] + q_a[3] * q_b[3] + q_a[0] * q_b[0],
                  ((q_a[3] * q_b[2] - q_a[2] * q_b[3]) - q_a[0] * q_b[1]) + q_b[0] * q_a[1],
                  ((q_a[1] * q_b[3] - q_a[3] * q_b[1]) - q_a[0] * q_b[2]) + q_b[0] * q_a[2],
                  ((q_a[2] * q_b[1] - q_a[1] * q_b[2]) - q_a[0] * q_b[3]) + q_b[0] * q_a[3]])
    length = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]
    check = length - 1
    if check > 0.0000001 or check < -0.0000001:
        d = d * (1.0 / np.sqrt(length))
    c = min(abs(d[0]), 1.0)
    ang = 2 * np.arccos(c)
    if ang > np.pi:
        ang -= 2 * np.pi
    td = _rot_conj_pt(q_a, t_a) - _rot_conj_pt(q_b, t_b)
    return ang, np.sqrt(td[0] * td[0] + td[1] * td[1] + td[2] * td[2])


# ---- projection, cost, Jacobian -----------------------------------------------------------------------------------------------------------------
def camera_point(q, t, M):
    """q (0, M) q* + t for M [n, 3] -> X, Y, Z, in the association of imgproj.c:181-217."""
    m0, m1, m2 = M[:, 0], M[:, 1], M[:, 2]
    a0 = -m0 * q[1] - q[2] * m1 - q[3] * m2
    a1 = q[0] * m0 + q[2] * m2 - q[3] * m1
    a2 = m1 * q[0] + q[3] * m0 - m2 * q[1]
    a3 = q[0] * m2 + m1 * q[1] - q[2] * m0
    X = -q[1] * a0 + q[0] * a1 - a2 * q[3] + q[2] * a3 + t[0]
    Y = -q[2] * a0 + q[0] * a2 - a3 * q[1] + q[3] * a1 + t[1]
    Z = -a0 * q[3] + q[0] * a3 - q[2] * a1 + q[1] * a2 + t[2]
    return X, Y, Z


def project(q, t, M):
    """The UN-weighted projection [n, 2]."""
    X, Y, Z = camera_point(q, t, M)
    iz = 1 / Z
    return np.stack([X * iz, Y * iz], axis=1)


def huber_weight(d, th):
    d_abs = np.abs(d) + 1e-12
    r = d_abs / th
    return np.sqrt(2 * (th * th) * (np.sqrt(1 + r * r) - 1)) / d_abs


def pull_to_measurement(est, meas, th):
    """convertCostToPseudoHuber."""
    d0, d1 = meas[:, 0] - est[:, 0], meas[:, 1] - est[:, 1]
    w = huber_weight(np.sqrt(d0 * d0 + d1 * d1), th)
    return np.stack([(1 - w) * meas[:, 0] + w * est[:, 0], (1 - w) * meas[:, 1] + w * est[:, 1]], axis=1)


def jacobian(r0, v, t, M):
    """Analytic Jacobian of project(local_quat(v) * r0, t, M): A [n, 2, 6] (3 local rotation, 3 translation), B [n, 2, 3] (the point)."""
    n = M.shape[0]
    lq = local_quat(v)
    q = quat_mult_fast(lq, r0)
    X, Y, Z = camera_point(q, t, M)
    iz = 1 / Z
    g0 = -((X * iz) * iz)
    g1 = -((Y * iz) * iz)
    q0, q1, q2, q3 = q
    N = [[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2.0 * (q1 * q2 - q0 * q3), 2.0 * (q1 * q3 + q0 * q2)],
         [2.0 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2.0 * (q2 * q3 - q0 * q1)],
         [2.0 * (q1 * q3 - q0 * q2), 2.0 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]]
    B = np.zeros((n, 2, 3))
    for c in range(3):
        B[:, 0, c] = iz * N[0][c] + g0 * N[2][c]
        B[:, 1, c] = iz * N[1][c] + g1 * N[2][c]
    A = np.zeros((n, 2, 6))
    zero = np.zeros(n)
    b = qmul((zero, M[:, 0], M[:, 1], M[:, 2]), (q0, -q1, -q2, -q3))      # (0, M) q*
    for k in range(3):
        dl = [-(v[k] / lq[0]), 0.0, 0.0, 0.0]
        dl[k + 1] = 1.0
        dq = qmul(dl, r0)
        D = qmul(dq, b)
        dx, dy, dz = 2.0 * D[1], 2.0 * D[2], 2.0 * D[3]
        A[:, 0, k] = iz * dx + g0 * dz
        A[:, 1, k] = iz * dy + g1 * dz
    A[:, 0, 3], A[:, 0, 5] = iz, g0
    A[:, 1, 4], A[:, 1, 5] = iz, g1
    return A, B


# ---- the optimiser ------------------------------------------------------------------------------------------------------------------------------
def _norm_order(nobs):
    """The four accumulators of nrmL2xmy as index lists into e (flat, length nobs)."""
    blockn = (nobs >> 3) << 3
    acc = [[], [], [], []]
    i = blockn - 1
    while i > 0:
        for k in range(8):
            acc[k & 3].append(i - k)
        i -= 8
    acc[0].extend(range(blockn, nobs))
    return [np.array(a, np.int64) for a in acc]


def _sq_norm(e_flat, order):
    sq = e_flat * e_flat
    s = [seqsum(sq[o]) if o.size else 0.0 for o in order]
    return float(s[0] + s[1] + s[2] + s[3])


def _invert_sym3(d, u):
    """d [n, 3] diagonal, u [n, 3] = (01, 02, 12) -> ok [n], inverse (00, 01, 02, 11, 12, 22) [n, 6] by cofactors."""
    a, dd, f = d[:, 0], d[:, 1], d[:, 2]
    b, c, e = u[:, 0], u[:, 1], u[:, 2]
    c00 = dd * f - e * e
    c01 = c * e - b * f
    c02 = b * e - c * dd
    det = a * c00 + b * c01 + c * c02
    ok = np.isfinite(det) & (det != 0)
    with np.errstate(all="ignore"):
        idet = 1 / det
        inv = np.stack([c00 * idet, c01 * idet, c02 * idet, (a * f - c * c) * idet, (b * c - a * e) * idet, (a * dd - b * b) * idet], axis=1)
    return ok, inv


_SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))     # (row, col) -> slot of the packed symmetric 3 x 3


def _chol_solve6(S, b):
    """Upper Cholesky U^T U = S (upper triangle of S read), then U^T y = b, U x = y.  -> (solved, x)"""
    U = np.zeros((6, 6))
    for j in range(6):
        ajj = S[j, j]
        for i in range(j):
            ajj = ajj - U[i, j] * U[i, j]
        if not (ajj > 0.0) or not np.isfinite(ajj):
            return False, None
        ajj = np.sqrt(ajj)
        U[j, j] = ajj
        r = 1.0 / ajj
        for k in range(j + 1, 6):
            s = S[j, k]
            for i in range(j):
                s = s - U[i, j] * U[i, k]
            U[j, k] = s * r
    y = np.zeros(6)
    for j in range(6):
        s = b[j]
        for i in range(j):
            s = s - U[i, j] * y[i]
        y[j] = s / U[j, j]
    x = np.zeros(6)
    for j in range(5, -1, -1):
        s = y[j]
        for i in range(j + 1, 6):
            s = s - U[j, i] * x[i]
        x[j] = s / U[j, j]
    return True, x


def jte_inf_norm(ea, eb):
    """sba_levmar.c:943-944 walks eab with `if(eab_inf < tmp) eab_inf = tmp` from 0: a NaN entry never wins the comparison and is passed over
    (np.max would hand it on); for entries without a NaN this is the plain maximum of the magnitudes."""
    return float(np.fmax.reduce(np.concatenate([[0.0], np.abs(ea), np.abs(eb).reshape(-1)])))


def sba_motstr(x1, x2, r0, t, M, th, itmax=MAXITER, opts=OPTS):
    """sba_motstr_levmar_x for two frames with the first fixed -> dict(ok, v, t, M, info[10], mu, trace, attempts).  ok False = SBA_ERROR.
    attempts: one (itno, first_bad, chol_refused, accepted) per damping attempt; first_bad = the first point whose V*_i did not invert, or -1;
    almost_singular: the run left through the error return behind the stop = 2 test."""
    n = M.shape[0]
    info = np.zeros(10)
    out = dict(ok=False, v=np.zeros(3), t=np.array(t, np.float64), M=np.array(M, np.float64), info=info, mu=0.0, trace=[], attempts=[],
               almost_singular=False)
    nobs, nvars = 4 * n, 12 + 3 * n
    if nobs < nvars:
        return out
    tau, eps1, eps2 = abs(opts[0]), abs(opts[1]), abs(opts[2])
    eps2_sq, eps3_sq, eps4_sq = opts[2] * opts[2], opts[3] * opts[3], opts[4] * opts[4]
    order = _norm_order(nobs)
    q_id = quat_mult_fast(local_quat(np.zeros(3)), np.array([1.0, 0, 0, 0]))
    t_id = np.zeros(3)

    def residual(v, tt, MM):
        h0 = pull_to_measurement(project(q_id, t_id, MM), x1, th)
        h1 = pull_to_measurement(project(quat_mult_fast(local_quat(v), r0), tt, MM), x2, th)
        with np.errstate(all="ignore"):
            e = np.concatenate([x1 - h0, x2 - h1], axis=1)        # [n, 4]: frame 0, frame 1
        return e, _sq_norm(e.reshape(-1), order)

    v, t, M = np.zeros(3), np.array(t, np.float64).reshape(3), np.array(M, np.float64)
    with np.errstate(all="ignore"):
        e, p_eL2 = residual(v, t, M)
    init_p_eL2 = p_eL2
    nfev, njev, nlss, nu, stop = 1, 0, 0, 2, 0
    mu = eab_inf = 0.0
    dp_L2 = np.finfo(np.float64).max
    if not np.isfinite(p_eL2):
        stop = 7
    diagU, diagV = np.zeros(6), np.zeros((n, 3))
    have_diag = False
    itno = 0
    while itno < itmax and not stop:
        _, B0 = jacobian(np.array([1.0, 0, 0, 0]), np.zeros(3), t_id, M)
        A, B1 = jacobian(r0, v, t, M)
        njev += 1
        U = np.zeros((6, 6))
        for ii in range(6):
            for jj in range(ii, 6):
                U[ii, jj] = seqsum(A[:, 0, ii] * A[:, 0, jj] + A[:, 1, ii] * A[:, 1, jj])
                U[jj, ii] = U[ii, jj]
        ea = np.array([seqsum(A[:, 0, ii] * e[:, 2] + A[:, 1, ii] * e[:, 3]) for ii in range(6)])
        Vu, Vd, eb = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        for ii in range(3):
            for jj in range(ii, 3):
                val = (B0[:, 0, ii] * B0[:, 0, jj] + B0[:, 1, ii] * B0[:, 1, jj]) + (B1[:, 0, ii] * B1[:, 0, jj] + B1[:, 1, ii] * B1[:, 1, jj])
                if ii == jj:
                    Vd[:, ii] = val
                else:
                    Vu[:, ii + jj - 1] = val
            eb[:, ii] = (B0[:, 0, ii] * e[:, 0] + B0[:, 1, ii] * e[:, 1]) + (B1[:, 0, ii] * e[:, 2] + B1[:, 1, ii] * e[:, 3])
        W = np.zeros((n, 6, 3))
        for ii in range(6):
            for jj in range(3):
                W[:, ii, jj] = A[:, 0, ii] * B1[:, 0, jj] + A[:, 1, ii] * B1[:, 1, jj]
        eab_inf = jte_inf_norm(ea, eb)
        pvec = np.concatenate([np.zeros(6), v, t, M.reshape(-1)])
        p_L2 = float(seqsum(pvec * pvec))
        diagU, diagV, have_diag = np.diag(U).copy(), Vd.copy(), True
        if eab_inf <= eps1:
            dp_L2 = 0.0
            stop = 1
            break
        if itno == 0:
            tmp = DBL_MIN
            for val in list(diagU) + list(diagV.reshape(-1)):
                if val > tmp:
                    tmp = val
            mu = tau * tmp
        while True:
            mu_used = mu
            for i in range(6):
                U[i, i] += mu
            trial = Vd + mu
            ok, inv = _invert_sym3(trial, Vu)
            if not ok.all():
                # the reference walks the points in order and leaves at the first failure: earlier points hold their inverse's diagonal,
                # the failing one its augmented diagonal, later ones are untouched
                f = int(np.argmin(ok))
                Vd[:f] = inv[:f][:, [0, 3, 5]]
                Vd[f] = trial[f]
                out["trace"].append((mu_used, p_eL2, False))
                out["attempts"].append((itno, f, False, False))
            else:
                Vd = inv[:, [0, 3, 5]].copy()
                Y = np.zeros((n, 6, 3))
                for ii in range(6):
                    for jj in range(3):
                        Y[:, ii, jj] = W[:, ii, 0] * inv[:, _SYM[0][jj]] + W[:, ii, 1] * inv[:, _SYM[1][jj]] + W[:, ii, 2] * inv[:, _SYM[2][jj]]
                S = np.zeros((6, 6))
                for ii in range(6):
                    for jj in range(ii, 6):
                        S[ii, jj] = U[ii, jj] - seqsum(Y[:, ii, 0] * W[:, jj, 0] + Y[:, ii, 1] * W[:, jj, 1] + Y[:, ii, 2] * W[:, jj, 2])
                E = np.array([ea[ii] - seqsum(Y[:, ii, 0] * eb[:, 0] + Y[:, ii, 1] * eb[:, 1] + Y[:, ii, 2] * eb[:, 2]) for ii in range(6)])
                solved, da = _chol_solve6(S, E)
                nlss += 1
                accepted = False
                if solved:
                    r = np.zeros((n, 3))
                    for ii in range(3):
                        wt = W[:, 0, ii] * da[0]
                        for jj in range(1, 6):
                            wt = wt + W[:, jj, ii] * da[jj]
                        r[:, ii] = eb[:, ii] - wt
                    db = np.zeros((n, 3))
                    for ii in range(3):
                        db[:, ii] = inv[:, _SYM[ii][0]] * r[:, 0] + inv[:, _SYM[ii][1]] * r[:, 1] + inv[:, _SYM[ii][2]] * r[:, 2]
                    dp = np.concatenate([np.zeros(6), da, db.reshape(-1)])
                    eab = np.concatenate([np.zeros(6), ea, eb.reshape(-1)])
                    dp_L2 = float(seqsum(dp * dp))
                    v_new, t_new, M_new = v + da[:3], t + da[3:], M + db
                    if dp_L2 <= eps2_sq * p_L2:
                        stop = 2
                        out["attempts"].append((itno, -1, False, False))
                        break
                    if dp_L2 >= (p_L2 + eps2) / EPSILON_SQ:
                        out["almost_singular"] = True
                        return out                      # "almost singular": SBA_ERROR, info unwritten
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
            if nu2 >= 2 ** 31:                      # the int wraps around
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
        for val in list(diagU) + list(diagV.reshape(-1)):
            if tmp < val:
                tmp = val
        info[4] = mu / tmp
    info[5], info[6], info[7], info[8], info[9] = itno, stop, nfev, njev, nlss
    out.update(ok=(stop != 7), v=v, t=t, M=M, mu=mu)
    return out


# ---- the wrapper --------------------------------------------------------------------------------------------------------------------------------
def convert_threshold(K1, K2, huber_thresh=-1.0):
    """pose_estim.cpp:1132-1136, :1195 -- (1,1) and (2,2), as the reference indexes."""
    th = huber_thresh if huber_thresh >= 0 else ROBUST_THRESH
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    return 4.0 * th / (np.sqrt(2.0) * (K1[1, 1] + K1[2, 2] + K2[1, 1] + K2[2, 2]))


def ba_oracle(p1, p2, R, t, Q, th, mask=None, angle_thresh=1.25, t_norm_thresh=0.05):
    """mlpl_refine_stereo_ba: th in CAMERA units.  -> dict(accepted, R, t, Q, info, mu, trace, attempts, branch); on rejection or failure R, t, Q
    equal the inputs.  branch: which way the wrapper went -- pivot (mat_to_quat_pivot), r0_flipped, and once the optimiser has ended normally
    qn_flipped, t_case ("kept_unit": |t| within 1e-4 of 1, "kept_tiny": |t| < 1e-3, "normalised") and refused_by (a tuple out of "angle",
    "t_norm", "stop", empty when accepted)."""
    p1, p2 = np.asarray(p1, np.float64).reshape(-1, 2), np.asarray(p2, np.float64).reshape(-1, 2)
    R0, t0 = np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64).reshape(3)
    Q0 = np.array(Q, np.float64).reshape(-1, 3)
    res = dict(accepted=False, R=R0.copy(), t=t0.copy(), Q=Q0.copy(), info=np.zeros(10), mu=0.0, trace=[], attempts=[], branch={})
    n = p1.shape[0]
    idx = np.arange(n) if mask is None else np.flatnonzero(np.asarray(mask).reshape(-1))
    if n == 0 or idx.size == 0:
        return res
    quat_old = mat_to_quat(R0)
    mag = np.sqrt(quat_old[0] * quat_old[0] + quat_old[1] * quat_old[1] + quat_old[2] * quat_old[2] + quat_old[3] * quat_old[3])
    mag = (1.0 if quat_old[0] >= 0.0 else -1.0) / mag
    r0 = quat_old * mag
    o = sba_motstr(p1[idx], p2[idx], r0, t0, Q0[idx], th)
    branch = dict(pivot=mat_to_quat_pivot(R0), r0_flipped=bool(quat_old[0] < 0.0), almost_singular=o["almost_singular"])
    res.update(info=o["info"], mu=o["mu"], trace=o["trace"], attempts=o["attempts"], branch=branch)
    if not o["ok"]:
        return res
    quat_new = quat_mult_fast(local_quat(o["v"]), r0)
    branch["qn_flipped"] = bool(quat_new[0] < 0.0)
    if quat_new[0] < 0.0:
        quat_new = quat_new * -1.0
    t_new = o["t"].copy()
    t_norm = np.sqrt(t_new[0] * t_new[0] + t_new[1] * t_new[1] + t_new[2] * t_new[2])
    if not (-1e-3 < t_norm < 1e-3) and abs(t_norm - 1.0) > 1e-4:      # nearZero of pose_helper.h:82-87
        t_new = t_new / t_norm
        branch["t_case"] = "normalised"
    else:
        branch["t_case"] = "kept_tiny" if -1e-3 < t_norm < 1e-3 else "kept_unit"
    r_diff, t_diff = rt_quality(quat_old, quat_new, t0, t_new)
    r_diff = r_diff / np.pi * 180.0
    branch["refused_by"] = tuple(k for k, hit in (("angle", abs(r_diff) > angle_thresh), ("t_norm", t_diff > t_norm_thresh),
                                                  ("stop", o["info"][6] > 5)) if hit)
    if abs(r_diff) > angle_thresh or t_diff > t_norm_thresh or o["info"][6] > 5:
        return res
    Qn = Q0.copy()
    Qn[idx] = o["M"]
    res.update(accepted=True, R=quat_to_matrix(quat_new), t=t_new, Q=Qn)
    return res


def refine_stereo_ba(p1, p2, R, t, Q, K1, K2, mask=None, angle_thresh=1.25, t_norm_thresh=0.05, huber_thresh=-1.0):
    """poselib::refineStereoBA(p1, p2, R, t, Q, K1, K2, false, mask, ...)."""
    return ba_oracle(p1, p2, R, t, Q, convert_threshold(K1, K2, huber_thresh), mask, angle_thresh, t_norm_thresh)
