// ba_common.h -- what the bundle-adjustment kernels share (bundle_adjust.hip: the stereo pair; bundle_adjust_multicam.hip: m cameras): the
// quaternion algebra and projection of BA_driver.cpp / imgproj.c, the pseudo-Huber residual, the Jacobian blocks of one point in one frame,
// the fixed-order workgroup reductions, the Levenberg-Marquardt core (the slots of the per-point state both kernels use, the damped inverse
// of V*_i with the reference's quirk, the repair after a V*_i that cannot be inverted, the point update, the optimiser's state with every
// stop and the mu / nu rules), the wrapper's helpers of pose_helper.cpp and the host entries' batch checks.  tests/ba_oracle.py is the float64
// restatement all of it follows operation by operation.  The core is device code without a barrier: what the kernels keep is how they gather
// the Jacobian sums, build and solve S, and commit an accepted step.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "mlpl_internal.h"

namespace mlpl {
namespace {

constexpr int kBaThreads = 256;
constexpr int kBaMaxIter = 150;  // MAXITER2 (BA_driver.cpp:57)

struct Quat {
    double w, x, y, z;
};

__device__ __host__ inline Quat quat_mult_fast(const Quat &a, const Quat &b) {  // BA_driver.cpp:153-185, its association
    const double t1 = (a.w + a.x) * (b.w + b.x);
    const double t2 = (a.z - a.y) * (b.y - b.z);
    const double t3 = (a.x - a.w) * (b.y + b.z);
    const double t4 = (a.y + a.z) * (b.x - b.w);
    const double t5 = (a.x + a.z) * (b.x + b.y);
    const double t6 = (a.x - a.z) * (b.x - b.y);
    const double t7 = (a.w + a.y) * (b.w - b.z);
    const double t8 = (a.w - a.y) * (b.w + b.z);
    const double t9 = 0.5 * (t5 - t6 + t7 + t8);
    return Quat{t2 + t9 - t5, t1 - t9 - t6, -t3 + t9 - t8, -t4 + t9 - t7};
}

__device__ inline Quat qmul(const Quat &a, const Quat &b) {
    return Quat{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}

__device__ inline Quat local_quat(const double v[3]) { return Quat{sqrt(1.0 - v[0] * v[0] - v[1] * v[1] - v[2] * v[2]), v[0], v[1], v[2]}; }

__device__ inline void camera_point(const Quat &q, const double t[3], const double M[3], double &X, double &Y, double &Z) {
    const double a0 = -M[0] * q.x - q.y * M[1] - q.z * M[2];
    const double a1 = q.w * M[0] + q.y * M[2] - q.z * M[1];
    const double a2 = M[1] * q.w + q.z * M[0] - M[2] * q.x;
    const double a3 = q.w * M[2] + M[1] * q.x - q.y * M[0];
    X = -q.x * a0 + q.w * a1 - a2 * q.z + q.y * a3 + t[0];
    Y = -q.y * a0 + q.w * a2 - a3 * q.x + q.z * a1 + t[1];
    Z = -a0 * q.z + q.w * a3 - q.y * a1 + q.x * a2 + t[2];
}

// x - (the projection pulled towards the measurement x): the residual of one frame
__device__ inline void residual2(const Quat &q, const double t[3], const double M[3], const double x[2], double th, double e[2]) {
    double X, Y, Z;
    camera_point(q, t, M, X, Y, Z);
    const double iz = 1 / Z;
    const double est0 = X * iz, est1 = Y * iz;
    const double d0 = x[0] - est0, d1 = x[1] - est1;
    const double d_abs = fabs(sqrt(d0 * d0 + d1 * d1)) + 1e-12;
    const double r = d_abs / th;
    const double w = sqrt(2 * (th * th) * (sqrt(1 + r * r) - 1)) / d_abs;
    e[0] = x[0] - ((1 - w) * x[0] + w * est0);
    e[1] = x[1] - ((1 - w) * x[1] + w * est1);
}

// the camera of a frame, as the Jacobian needs it
struct CamJ {
    Quat q;
    double t[3];
    double N[3][3];
    Quat dq[3];
};

__device__ inline void cam_setup(const Quat &r0, const double v[3], const double t[3], bool with_rotation, CamJ &c) {
    const Quat lq = local_quat(v);
    c.q = quat_mult_fast(lq, r0);
    const double q0 = c.q.w, q1 = c.q.x, q2 = c.q.y, q3 = c.q.z;
    for (int k = 0; k < 3; ++k) c.t[k] = t[k];
    c.N[0][0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, c.N[0][1] = 2.0 * (q1 * q2 - q0 * q3), c.N[0][2] = 2.0 * (q1 * q3 + q0 * q2);
    c.N[1][0] = 2.0 * (q1 * q2 + q0 * q3), c.N[1][1] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, c.N[1][2] = 2.0 * (q2 * q3 - q0 * q1);
    c.N[2][0] = 2.0 * (q1 * q3 - q0 * q2), c.N[2][1] = 2.0 * (q2 * q3 + q0 * q1), c.N[2][2] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
    if (with_rotation)
        for (int k = 0; k < 3; ++k) {
            Quat dl{-(v[k] / lq.w), k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
            c.dq[k] = qmul(dl, r0);
        }
}

// A [2][6] (only with_rotation) and B [2][3] of one point in one frame
template <bool kWithA>
__device__ inline void jac_blocks(const CamJ &c, const double M[3], double A[2][6], double B[2][3]) {
    double X, Y, Z;
    camera_point(c.q, c.t, M, X, Y, Z);
    const double iz = 1 / Z;
    const double g0 = -((X * iz) * iz), g1 = -((Y * iz) * iz);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        B[0][k] = iz * c.N[0][k] + g0 * c.N[2][k];
        B[1][k] = iz * c.N[1][k] + g1 * c.N[2][k];
    }
    if (kWithA) {
        const Quat b = qmul(Quat{0.0, M[0], M[1], M[2]}, Quat{c.q.w, -c.q.x, -c.q.y, -c.q.z});
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const Quat D = qmul(c.dq[k], b);
            const double dx = 2.0 * D.x, dy = 2.0 * D.y, dz = 2.0 * D.z;
            A[0][k] = iz * dx + g0 * dz;
            A[1][k] = iz * dy + g1 * dz;
        }
        A[0][3] = iz, A[0][4] = 0.0, A[0][5] = g0;
        A[1][3] = 0.0, A[1][4] = iz, A[1][5] = g1;
    }
}

// Sums of N values over the workgroup in a fixed order; every lane gets the totals.  red: 4 x N doubles of LDS.
template <int N>
__device__ inline void block_sum(double (&v)[N], double *red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
        if (lane == 0) red[wv * N + k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (red[k] + red[N + k]) + (red[2 * N + k] + red[3 * N + k]);
    __syncthreads();
}

__device__ inline double block_max(double x, double *red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, 64));
    if (lane == 0) red[wv] = x;
    __syncthreads();
    x = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return x;
}

__device__ inline int block_min_int(int x, int *red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off, 64));
    if (lane == 0) red[wv] = x;
    __syncthreads();
    x = min(min(red[0], red[1]), min(red[2], red[3]));
    __syncthreads();
    return x;
}

// ---- the per-point state: kernel-independent slots first, the kernel's own (residuals, W) from kPCam on ---------------------------------------------
constexpr int kPM = 0;     // 2 x 3: the point, current / trial
constexpr int kPVu = 6;    // 3: V_i (0,1) (0,2) (1,2)
constexpr int kPVd = 9;    // 3: V_i's working diagonal
constexpr int kPEb = 12;   // 3
constexpr int kPInv = 15;  // 2 x 6: (V*_i)^-1 as (00, 01, 02, 11, 12, 22)
constexpr int kPCam = 27;

// one problem's workspace, structure-of-arrays over the problem's stride: pw(slot, k) is point k's entry
struct PointWs {
    double *ws;
    size_t stride;
    __device__ double &operator()(int slot, int k) const { return ws[(size_t)slot * stride + k]; }
};

__device__ inline int inv_diag(int c) { return c == 0 ? 0 : c == 1 ? 3 : 5; }  // where (V*_i)^-1 keeps its diagonal

// (V_i + mu I)^-1 of point k by cofactors, written beside the inverse it may read; false where the determinant is zero or not finite.
// sba_levmar.c:1341-1355 (restoring V_i's diagonal after a rejected attempt) is compiled out in the reference, and V_i's lower triangle is
// where it keeps the inverse: after a rejected attempt mu is added onto the DIAGONAL OF THAT ATTEMPT'S INVERSE (vd_from_inv), not onto V_i's.
__device__ inline bool damped_inverse(const PointWs &pw, int k, bool vd_from_inv, int cur_inv, double mu, double inv[6]) {
    double d[3];
    for (int c = 0; c < 3; ++c) d[c] = (vd_from_inv ? pw(kPInv + cur_inv * 6 + inv_diag(c), k) : pw(kPVd + c, k)) + mu;
    const double vb = pw(kPVu + 0, k), vc = pw(kPVu + 1, k), ve = pw(kPVu + 2, k);
    const double c00 = d[1] * d[2] - ve * ve, c01 = vc * ve - vb * d[2], c02 = vb * ve - vc * d[1];
    const double det = d[0] * c00 + vb * c01 + vc * c02;
    if (!(isfinite(det) && det != 0)) return false;
    const double idet = 1 / det;
    inv[0] = c00 * idet, inv[1] = c01 * idet, inv[2] = c02 * idet;
    inv[3] = (d[0] * d[2] - vc * vc) * idet, inv[4] = (vb * vc - d[0] * ve) * idet, inv[5] = (d[0] * d[1] - vb * vb) * idet;
    for (int c = 0; c < 6; ++c) pw(kPInv + (cur_inv ^ 1) * 6 + c, k) = inv[c];
    return true;
}

// The reference walks the points in order and leaves at the first V*_i it cannot invert: earlier points hold their new inverse's diagonal,
// the failing one its augmented diagonal, later ones are untouched.  Afterwards the working diagonal lives in kPVd again.
__device__ inline void repair_first_bad(const PointWs &pw, int n, int first_bad, bool vd_from_inv, int cur_inv, double mu) {
    for (int k = threadIdx.x; k < n; k += kBaThreads)
        for (int c = 0; c < 3; ++c) {
            const double old = vd_from_inv ? pw(kPInv + cur_inv * 6 + inv_diag(c), k) : pw(kPVd + c, k);
            pw(kPVd + c, k) = k < first_bad ? pw(kPInv + (cur_inv ^ 1) * 6 + inv_diag(c), k) : k == first_bad ? old + mu : old;
        }
}

// the accepted attempt's inverse of point k; a caller issues it before it forms r, so that the loads wait behind that work
__device__ inline void load_inverse(const PointWs &pw, int k, int cur_inv, double inv[6]) {
    for (int c = 0; c < 6; ++c) inv[c] = pw(kPInv + cur_inv * 6 + c, k);
}

// db_i = (V*_i)^-1 r with r = eb_i - sum_j W_ij^T da_j from the caller; the trial point Mn beside the current one; ||db||^2 onto s3[0], this
// point's share of dL onto s3[2]
__device__ inline void point_update(const PointWs &pw, int k, int cur_m, const double inv[6], const double r[3], const double ebv[3], double mu,
                                    double Mn[3], double s3[3]) {
    const double im[3][3] = {{inv[0], inv[1], inv[2]}, {inv[1], inv[3], inv[4]}, {inv[2], inv[4], inv[5]}};
#pragma unroll
    for (int ii = 0; ii < 3; ++ii) {
        const double db = im[ii][0] * r[0] + im[ii][1] * r[1] + im[ii][2] * r[2];
        Mn[ii] = pw(kPM + cur_m * 3 + ii, k) + db;
        pw(kPM + (cur_m ^ 1) * 3 + ii, k) = Mn[ii];
        s3[0] += db * db;
        s3[2] += db * (mu * db + ebv[ii]);
    }
}

// ---- the optimiser's state and decisions (sba_levmar.c:449-1400); every value is workgroup-uniform, each lane holds its own copy -------------------
enum LmVerdict { kLmAccepted, kLmRejected, kLmLeave };

struct LmState {
    double mu = 0.0, p_eL2 = 0.0, init_p_eL2 = 0.0, eab_inf = 0.0, dp_L2 = DBL_MAX, max_diag = 0.0;
    int nu = 2, stop = 0, itno = 0, nfev = 1, njev = 0, nlss = 0;
    bool have_diag = false, failed = false;

    __device__ void start(double cost) {
        p_eL2 = init_p_eL2 = cost;
        if (!isfinite(p_eL2)) stop = 7;
    }
    // after the gradient sums: false = stop 1; the first mu
    __device__ bool after_gradient(double mx_e, double mx_d) {
        const double tau = 1e-3, eps1 = 1e-12;
        eab_inf = mx_e;
        max_diag = mx_d, have_diag = true;
        if (eab_inf <= eps1) {
            dp_L2 = 0.0;
            stop = 1;
            return false;
        }
        if (itno == 0) mu = tau * max_diag;
        return true;
    }
    // a trial step: the cameras' part of ||dp||^2 and dL, s3 = ||db||^2, ||e(p + dp)||^2, dL over the points, p_L2 = ||p||^2.  On
    // kLmAccepted the caller commits the trial; on kLmLeave it leaves the damping loop (stop or failed says why)
    __device__ LmVerdict verdict(double cam_dp_L2, double cam_dL, const double s3[3], double p_L2) {
        const double eps2 = 1e-12, eps2_sq = 1e-12 * 1e-12, eps4_sq = 1E-05 * 1E-05;
        dp_L2 = cam_dp_L2 + s3[0];
        const double dL = cam_dL + s3[2];
        const double pdp_eL2 = s3[1];
        if (dp_L2 <= eps2_sq * p_L2) {
            stop = 2;
            return kLmLeave;
        }
        if (dp_L2 >= (p_L2 + eps2) / (1E-12 * 1E-12)) {  // "almost singular": the optimiser fails, info stays unwritten
            failed = true;
            return kLmLeave;
        }
        ++nfev;
        if (!isfinite(pdp_eL2)) {
            stop = 7;
            return kLmLeave;
        }
        const double dF = p_eL2 - pdp_eL2;
        if (!(dL > 0.0 && dF > 0.0)) return kLmRejected;
        double tmp = 2.0 * dF / dL - 1.0;
        tmp = 1.0 - tmp * tmp * tmp;
        mu = mu * ((tmp >= 0.3333333334) ? tmp : 0.3333333334);
        nu = 2;
        if (pdp_eL2 - 2.0 * sqrt(p_eL2 * pdp_eL2) < (eps4_sq - 1.0) * p_eL2) stop = 4;
        p_eL2 = pdp_eL2;
        return kLmAccepted;
    }
    // a rejected or refused attempt: false = stop 6
    __device__ bool reject() {
        mu *= nu;
        if (nu >= (1 << 30)) {  // 2 nu no longer fits an int
            stop = 6;
            return false;
        }
        nu *= 2;
        return true;
    }
    // the end of an outer step: false = the optimiser failed
    __device__ bool end_step() {
        const double eps3_sq = 1e-12 * 1e-12;
        if (failed) return false;
        if (p_eL2 <= eps3_sq) stop = 5;
        return true;
    }
    // info as sba writes it; -> sba_ok.  A failed run leaves info unwritten and mu at 0.
    __device__ bool finish(double info[10]) {
        if (failed) {
            mu = 0.0;
            return false;
        }
        if (itno >= kBaMaxIter) stop = 3;
        info[0] = init_p_eL2, info[1] = p_eL2, info[2] = eab_inf, info[3] = dp_L2;
        if (have_diag) info[4] = mu / max_diag;
        info[5] = itno, info[6] = stop, info[7] = nfev, info[8] = njev, info[9] = nlss;
        return stop != 7;
    }
};

// ---- the wrapper's quaternion helpers (P/source/pose_helper.cpp) ---------------------------------------------------------------------------------
__device__ inline Quat mat_to_quat(const double R[9]) {
    const double tr = R[0] + R[4] + R[8];
    double q[4];
    if (tr > 0.0) {
        double root = sqrt(tr + 1.0);
        q[0] = 0.5 * root;
        root = 0.5 / root;
        q[1] = (R[7] - R[5]) * root;
        q[2] = (R[2] - R[6]) * root;
        q[3] = (R[3] - R[1]) * root;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double root = sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
        q[i + 1] = 0.5 * root;
        root = 0.5 / root;
        q[0] = (R[k * 3 + j] - R[j * 3 + k]) * root;
        q[j + 1] = (R[j * 3 + i] + R[i * 3 + j]) * root;
        q[k + 1] = (R[k * 3 + i] + R[i * 3 + k]) * root;
    }
    return Quat{q[0], q[1], q[2], q[3]};
}

__device__ inline void quat_to_matrix(const Quat &q, double R[9]) {
    const double sw = q.w * q.w, sx = q.x * q.x, sy = q.y * q.y, sz = q.z * q.z;
    const double invs = 1 / (sx + sy + sz + sw);
    R[0] = (sx - sy - sz + sw) * invs;
    R[4] = (-sx + sy - sz + sw) * invs;
    R[8] = (-sx - sy + sz + sw) * invs;
    double a = q.x * q.y, b = q.z * q.w;
    R[3] = 2.0 * (a + b) * invs;
    R[1] = 2.0 * (a - b) * invs;
    a = q.x * q.z, b = q.y * q.w;
    R[6] = 2.0 * (a - b) * invs;
    R[2] = 2.0 * (a + b) * invs;
    a = q.y * q.z, b = q.x * q.w;
    R[7] = 2.0 * (a + b) * invs;
    R[5] = 2.0 * (a - b) * invs;
}

__device__ inline void rot_conj_pt(const Quat &q, const double p[3], double o[3]) {  // quatMult3DPt(quatConj(q), p)
    const double c0 = q.w, c1 = -q.x, c2 = -q.y, c3 = -q.z;
    const double s1 = c2 * p[2] - c3 * p[1] + c0 * p[0];
    const double s2 = c3 * p[0] - c1 * p[2] + c0 * p[1];
    const double s3 = c1 * p[1] - c2 * p[0] + c0 * p[2];
    const double s0 = -(c1 * p[0] + c2 * p[1] + c3 * p[2]);
    o[0] = ((s3 * c2 - s2 * c3) - s0 * c1) + c0 * s1;
    o[1] = ((s1 * c3 - s3 * c1) - s0 * c2) + c0 * s2;
    o[2] = ((s2 * c1 - s1 * c2) - s0 * c3) + c0 * s3;
}

__device__ inline void rt_quality(const Quat &a, const Quat &b, const double ta[3], const double tb[3], double &rdiff, double &tdiff) {
    double d[4] = {a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w, ((a.z * b.y - a.y * b.z) - a.w * b.x) + b.w * a.x,
                   ((a.x * b.z - a.z * b.x) - a.w * b.y) + b.w * a.y, ((a.y * b.x - a.x * b.y) - a.w * b.z) + b.w * a.z};
    const double length = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
    const double check = length - 1;
    if (check > 0.0000001 || check < -0.0000001) d[0] *= 1.0 / sqrt(length);
    double c = fabs(d[0]);
    if (c > 1.0) c = 1.0;
    double ang = 2 * acos(c);
    if (ang > M_PI) ang -= 2 * M_PI;
    rdiff = ang;
    double u[3], w[3];
    rot_conj_pt(a, ta, u);
    rot_conj_pt(b, tb, w);
    const double e0 = u[0] - w[0], e1 = u[1] - w[1], e2 = u[2] - w[2];
    tdiff = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
}

// ---- host: what the batch entries check before they touch the device, and the debug store of mu -----------------------------------------------------
// have_args: the entry's own pointers and strides; per_problem(b): its further checks of problem b, MLPL_OK to go on
template <class F>
int ba_check_batch(const char *who, bool have_args, int B, int stride, const int32_t *counts, F per_problem) {
    if (!have_args || B < 1 || stride < 1 || !counts) {
        set_error("%s: bad arguments", who);
        return MLPL_E_BAD_INPUT;
    }
    if (B > 65535) {
        set_error("%s: at most 65535 problems per call", who);
        return MLPL_E_BAD_INPUT;
    }
    if (!counts_in_range(who, B, counts, 0, stride)) return MLPL_E_BAD_INPUT;
    for (int b = 0; b < B; ++b)
        if (int rc = per_problem(b)) return rc;
    return MLPL_OK;
}

// mu at exit of the problems of the calling thread's last call, for the entry's mlpl_debug_*_last_mu
struct LastMu {
    std::vector<double> mu;
    int get(double *out, int max_items) const {
        if (!out || max_items < 0) return MLPL_E_BAD_INPUT;
        const int n = std::min<int>((int)mu.size(), max_items);
        for (int i = 0; i < n; ++i) out[i] = mu[(size_t)i];
        return n;
    }
};

}  // namespace
}  // namespace mlpl
