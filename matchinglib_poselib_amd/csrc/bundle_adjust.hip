// bundle_adjust.hip -- poselib::refineStereoBA, pointsInImgCoords == false (P/source/pose_estim.cpp:1083-1206, :1294-1348): motion and structure
// bundle adjustment of one stereo pair with the first camera fixed, i.e. SBAdriver::perform_sba (P/source/BA_driver.cpp:1878-2260) around
// sba_motstr_levmar_x (sba-1.6/sba_levmar.c:449-1400) with the pseudo-Huber cost of BA_driver.cpp:2612-2648.  tests/ba_oracle.py is the
// float64 restatement this file follows operation by operation; its header lists what is the reference's arithmetic and what is not (the
// Jacobian written from the quaternion algebra, the cofactor inverse of V*_i, the unblocked 6 x 6 Cholesky).
//
// One workgroup of 256 lanes per problem (blockIdx.x), the whole Levenberg-Marquardt iteration -- every outer step and every damping attempt
// -- inside ONE launch, the wrapper's acceptance rule and the scatter of the refined points included.  The valid rows are compacted (stable,
// ascending) into a list; slot k of the list belongs to lane k % 256 for the whole run, so the per-point state in the problem's workspace is
// only ever read by the lane that wrote it.  Every sum over points is: each lane over its slots in ascending order, a butterfly over the 64
// lanes of a wave, then (w0 + w1) + (w2 + w3) -- a fixed order, no atomics, so a problem gives the same bits alone and inside a batch.
//
// Per-point state (kBaSlots doubles per point, structure-of-arrays over the problem's stride): the point and the residual twice (the trial of
// a damping attempt is written beside the current one and the two swap on acceptance), V_i's strict upper triangle and working diagonal, W_i,
// eb_i, (V*_i)^-1 twice (a damping attempt reads the previous attempt's inverse: sba_levmar.c:1341-1355 is compiled out, so mu is added onto
// the DIAGONAL OF THE INVERSE that the previous, rejected attempt left in V_i's lower triangle).  The blocks are kept and not recomputed per
// pass: the simpler of the two options; recomputing them has not been measured.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "mlpl_internal.h"

namespace mlpl {
namespace {

constexpr int kBaThreads = 256;
constexpr int kBaMaxIter = 150;  // MAXITER2 (BA_driver.cpp:57)
// slots of the per-point state
constexpr int kSM = 0;     // 2 x 3: the point, current / trial
constexpr int kSE = 6;     // 2 x 4: the residual (frame 0 x, y, frame 1 x, y), current / trial
constexpr int kSVu = 14;   // 3: V_i (0,1) (0,2) (1,2)
constexpr int kSVd = 17;   // 3: V_i's working diagonal
constexpr int kSW = 20;    // 18: W_i, 6 x 3 row-major
constexpr int kSEb = 38;   // 3
constexpr int kSInv = 41;  // 2 x 6: (V*_i)^-1 as (00, 01, 02, 11, 12, 22)
constexpr int kBaSlots = 53;
constexpr int kBaIn = 16;   // per problem: R 9, t 3, th, angle_thresh, t_norm_thresh
constexpr int kBaOut = 24;  // per problem: R 9, t 3, info 10, mu, accepted

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

// upper Cholesky U^T U = S, U^T y = b, U x = y (ba_oracle._chol_solve6)
__device__ inline bool chol_solve6(const double S[6][6], const double b[6], double x[6]) {
    double U[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double ajj = S[j][j];
        for (int i = 0; i < j; ++i) ajj = ajj - U[i][j] * U[i][j];
        if (!(ajj > 0.0) || !isfinite(ajj)) return false;
        ajj = sqrt(ajj);
        U[j][j] = ajj;
        const double r = 1.0 / ajj;
        for (int k = j + 1; k < 6; ++k) {
            double s = S[j][k];
            for (int i = 0; i < j; ++i) s = s - U[i][j] * U[i][k];
            U[j][k] = s * r;
        }
    }
    double y[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = b[j];
        for (int i = 0; i < j; ++i) s = s - U[i][j] * y[i];
        y[j] = s / U[j][j];
    }
#pragma unroll
    for (int j = 5; j >= 0; --j) {
        double s = y[j];
        for (int i = j + 1; i < 6; ++i) s = s - U[j][i] * x[i];
        x[j] = s / U[j][j];
    }
    return true;
}

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

// ---- the kernel ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBaThreads) void bundle_adjust_kernel(const double *__restrict__ in /*[B][kBaIn]*/, const double *__restrict__ p1,
                                                                   const double *__restrict__ p2, const int32_t *__restrict__ counts, int stride,
                                                                   const uint8_t *__restrict__ masks /*[B][stride] or NULL*/,
                                                                   double *__restrict__ Q /*[B][stride][3] in / out*/,
                                                                   int32_t *__restrict__ idx_all /*[B][stride]*/,
                                                                   double *__restrict__ ws_all /*[B][kBaSlots][stride]*/,
                                                                   double *__restrict__ out /*[B][kBaOut]*/) {
    __shared__ double red[4 * 28];
    __shared__ int red_i[8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_rows = counts[b];
    const double *pin = in + (size_t)b * kBaIn;
    double *po = out + (size_t)b * kBaOut;
    const size_t row0 = (size_t)b * stride;
    int32_t *idx = idx_all + row0;
    double *ws = ws_all + row0 * kBaSlots;
    const size_t S = (size_t)stride;
#define WSV(slot, k) ws[(size_t)(slot)*S + (k)]

    // ---- stable compaction of the mask into an ascending list
    int n = 0;
    for (int base = 0; base < n_rows; base += kBaThreads) {
        const int i = base + tid;
        const bool want = i < n_rows && (!masks || masks[row0 + i]);
        const unsigned long long wb = __ballot(want);
        if (lane == 0) red_i[wv] = __popcll(wb);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wv; ++w) before += red_i[w];
        const int total = red_i[0] + red_i[1] + red_i[2] + red_i[3];
        if (want) idx[n + before + __popcll(wb & ((1ull << lane) - 1ull))] = i;
        n += total;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();

    double Rin[9], t0[3];
    for (int k = 0; k < 9; ++k) Rin[k] = pin[k];
    for (int k = 0; k < 3; ++k) t0[k] = pin[9 + k];
    const double th = pin[12], angle_thresh = pin[13], t_norm_thresh = pin[14];

    double info[10];
    for (int k = 0; k < 10; ++k) info[k] = 0.0;
    double mu = 0.0;
    bool sba_ok = false;
    double v[3] = {0.0, 0.0, 0.0}, t[3] = {t0[0], t0[1], t0[2]};
    int cur_m = 0;
    const Quat quat_old = mat_to_quat(Rin);
    Quat r0;
    {
        double mag = sqrt(quat_old.w * quat_old.w + quat_old.x * quat_old.x + quat_old.y * quat_old.y + quat_old.z * quat_old.z);
        mag = (quat_old.w >= 0.0 ? 1.0 : -1.0) / mag;
        r0 = Quat{quat_old.w * mag, quat_old.x * mag, quat_old.y * mag, quat_old.z * mag};
    }

    // fewer measurements than unknowns (4 n < 12 + 3 n): the optimiser refuses, as does an empty problem
    if (n >= 12) {
        const double tau = 1e-3, eps1 = 1e-12, eps2 = 1e-12, eps2_sq = 1e-12 * 1e-12, eps3_sq = 1e-12 * 1e-12, eps4_sq = 1E-05 * 1E-05;
        const double zero3[3] = {0.0, 0.0, 0.0};
        const Quat q_unit{1.0, 0.0, 0.0, 0.0};
        const Quat q_id = quat_mult_fast(local_quat(zero3), q_unit);
        CamJ cam0;
        cam_setup(q_unit, zero3, zero3, false, cam0);

        // the points into the workspace, the residual at the start
        int cur_e = 0;
        double p_eL2;
        {
            const Quat q1 = quat_mult_fast(local_quat(v), r0);
            double acc[1] = {0.0};
            for (int k = tid; k < n; k += kBaThreads) {
                const size_t at = row0 + idx[k];
                double M[3], e[4];
                for (int c = 0; c < 3; ++c) WSV(kSM + c, k) = M[c] = Q[at * 3 + c];
                const double x1[2] = {p1[at * 2], p1[at * 2 + 1]}, x2[2] = {p2[at * 2], p2[at * 2 + 1]};
                residual2(q_id, zero3, M, x1, th, e);
                residual2(q1, t, M, x2, th, e + 2);
                for (int c = 0; c < 4; ++c) {
                    WSV(kSE + c, k) = e[c];
                    acc[0] += e[c] * e[c];
                }
            }
            block_sum(acc, red);
            p_eL2 = acc[0];
        }
        const double init_p_eL2 = p_eL2;
        int nfev = 1, njev = 0, nlss = 0, nu = 2, stop = 0, itno = 0;
        double eab_inf = 0.0, dp_L2 = DBL_MAX, max_diag = 0.0;
        bool have_diag = false, failed = false;
        if (!isfinite(p_eL2)) stop = 7;

        for (; itno < kBaMaxIter && !stop; ++itno) {
            // ---- Jacobian blocks, V_i, W_i, eb_i; U, ea, ||J^T e||_inf, ||p||^2, the largest diagonal entry
            CamJ cam1;
            cam_setup(r0, v, t, true, cam1);
            ++njev;
            double sums[28];  // U upper 21, ea 6, ||points||^2
#pragma unroll
            for (int k = 0; k < 28; ++k) sums[k] = 0.0;
            double mx_e = 0.0, mx_d = DBL_MIN;
            for (int k = tid; k < n; k += kBaThreads) {
                double M[3], e[4], A[2][6], B0[2][3], B1[2][3];
                for (int c = 0; c < 3; ++c) M[c] = WSV(kSM + cur_m * 3 + c, k);
                for (int c = 0; c < 4; ++c) e[c] = WSV(kSE + cur_e * 4 + c, k);
                jac_blocks<false>(cam0, M, A, B0);
                jac_blocks<true>(cam1, M, A, B1);
                int s = 0;
#pragma unroll
                for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                    for (int jj = ii; jj < 6; ++jj) sums[s++] += A[0][ii] * A[0][jj] + A[1][ii] * A[1][jj];
#pragma unroll
                for (int ii = 0; ii < 6; ++ii) sums[21 + ii] += A[0][ii] * e[2] + A[1][ii] * e[3];
#pragma unroll
                for (int ii = 0; ii < 3; ++ii) {
#pragma unroll
                    for (int jj = ii; jj < 3; ++jj) {
                        const double val = (B0[0][ii] * B0[0][jj] + B0[1][ii] * B0[1][jj]) + (B1[0][ii] * B1[0][jj] + B1[1][ii] * B1[1][jj]);
                        if (ii == jj) {
                            WSV(kSVd + ii, k) = val;
                            if (val > mx_d) mx_d = val;
                        } else {
                            WSV(kSVu + ii + jj - 1, k) = val;
                        }
                    }
                    const double ebv = (B0[0][ii] * e[0] + B0[1][ii] * e[1]) + (B1[0][ii] * e[2] + B1[1][ii] * e[3]);
                    WSV(kSEb + ii, k) = ebv;
                    mx_e = fmax(mx_e, fabs(ebv));
                }
#pragma unroll
                for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                    for (int jj = 0; jj < 3; ++jj) WSV(kSW + ii * 3 + jj, k) = A[0][ii] * B1[0][jj] + A[1][ii] * B1[1][jj];
                sums[27] += M[0] * M[0];
                sums[27] += M[1] * M[1];
                sums[27] += M[2] * M[2];
            }
            block_sum(sums, red);
            mx_e = block_max(mx_e, red);
            mx_d = block_max(mx_d, red);
            double U[6][6], ea[6];
            {
                int s = 0;
                for (int ii = 0; ii < 6; ++ii)
                    for (int jj = ii; jj < 6; ++jj) U[ii][jj] = U[jj][ii] = sums[s++];
            }
            for (int ii = 0; ii < 6; ++ii) {
                ea[ii] = sums[21 + ii];
                mx_e = fmax(mx_e, fabs(ea[ii]));
                if (U[ii][ii] > mx_d) mx_d = U[ii][ii];
            }
            eab_inf = mx_e;
            double p_L2 = 0.0;
            for (int k = 0; k < 3; ++k) p_L2 += v[k] * v[k];
            for (int k = 0; k < 3; ++k) p_L2 += t[k] * t[k];
            p_L2 += sums[27];
            max_diag = mx_d, have_diag = true;
            if (eab_inf <= eps1) {
                dp_L2 = 0.0;
                stop = 1;
                break;
            }
            if (itno == 0) mu = tau * max_diag;

            // ---- the damping loop
            bool vd_from_inv = false;  // V_i's diagonal currently lives in the previous attempt's inverse
            int cur_inv = 0;
            while (true) {
                for (int i = 0; i < 6; ++i) U[i][i] += mu;
                double acc[27];  // sum Y W^T upper 21, sum Y eb 6
#pragma unroll
                for (int k = 0; k < 27; ++k) acc[k] = 0.0;
                int first_bad = INT_MAX;
                for (int k = tid; k < n; k += kBaThreads) {
                    double d[3], W[6][3], ebv[3];
                    for (int c = 0; c < 3; ++c)
                        d[c] = (vd_from_inv ? WSV(kSInv + cur_inv * 6 + (c == 0 ? 0 : c == 1 ? 3 : 5), k) : WSV(kSVd + c, k)) + mu;
                    const double vb = WSV(kSVu + 0, k), vc = WSV(kSVu + 1, k), ve = WSV(kSVu + 2, k);
                    const double c00 = d[1] * d[2] - ve * ve, c01 = vc * ve - vb * d[2], c02 = vb * ve - vc * d[1];
                    const double det = d[0] * c00 + vb * c01 + vc * c02;
                    if (!(isfinite(det) && det != 0)) {
                        if (k < first_bad) first_bad = k;
                        continue;
                    }
                    const double idet = 1 / det;
                    double inv[6] = {c00 * idet, c01 * idet, c02 * idet, (d[0] * d[2] - vc * vc) * idet, (vb * vc - d[0] * ve) * idet,
                                     (d[0] * d[1] - vb * vb) * idet};
                    for (int c = 0; c < 6; ++c) WSV(kSInv + (cur_inv ^ 1) * 6 + c, k) = inv[c];
#pragma unroll
                    for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                        for (int jj = 0; jj < 3; ++jj) W[ii][jj] = WSV(kSW + ii * 3 + jj, k);
                    for (int c = 0; c < 3; ++c) ebv[c] = WSV(kSEb + c, k);
                    const double im[3][3] = {{inv[0], inv[1], inv[2]}, {inv[1], inv[3], inv[4]}, {inv[2], inv[4], inv[5]}};
                    double Y[6][3];
#pragma unroll
                    for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                        for (int jj = 0; jj < 3; ++jj) Y[ii][jj] = W[ii][0] * im[0][jj] + W[ii][1] * im[1][jj] + W[ii][2] * im[2][jj];
                    int s = 0;
#pragma unroll
                    for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                        for (int jj = ii; jj < 6; ++jj) acc[s++] += Y[ii][0] * W[jj][0] + Y[ii][1] * W[jj][1] + Y[ii][2] * W[jj][2];
#pragma unroll
                    for (int ii = 0; ii < 6; ++ii) acc[21 + ii] += Y[ii][0] * ebv[0] + Y[ii][1] * ebv[1] + Y[ii][2] * ebv[2];
                }
                first_bad = block_min_int(first_bad, red_i);
                bool accepted = false;
                if (first_bad != INT_MAX) {
                    // the reference walks the points in order and leaves at the first V*_i it cannot invert: earlier points hold their new
                    // inverse's diagonal, the failing one its augmented diagonal, later ones are untouched
                    for (int k = tid; k < n; k += kBaThreads)
                        for (int c = 0; c < 3; ++c) {
                            const int dslot = c == 0 ? 0 : c == 1 ? 3 : 5;
                            const double old = vd_from_inv ? WSV(kSInv + cur_inv * 6 + dslot, k) : WSV(kSVd + c, k);
                            WSV(kSVd + c, k) = k < first_bad ? WSV(kSInv + (cur_inv ^ 1) * 6 + dslot, k) : k == first_bad ? old + mu : old;
                        }
                    vd_from_inv = false;
                } else {
                    cur_inv ^= 1, vd_from_inv = true;
                    block_sum(acc, red);
                    double Sm[6][6], E[6], da[6];
                    {
                        int s = 0;
                        for (int ii = 0; ii < 6; ++ii)
                            for (int jj = ii; jj < 6; ++jj) Sm[ii][jj] = Sm[jj][ii] = U[ii][jj] - acc[s++];
                    }
                    for (int ii = 0; ii < 6; ++ii) E[ii] = ea[ii] - acc[21 + ii];
                    const bool solved = chol_solve6(Sm, E, da);
                    ++nlss;
                    if (solved) {
                        // ---- db_i, the trial point, its residual; ||dp||^2, ||e(p + dp)||^2, dL
                        double vn[3], tn[3];
                        for (int k = 0; k < 3; ++k) vn[k] = v[k] + da[k], tn[k] = t[k] + da[3 + k];
                        const Quat q1 = quat_mult_fast(local_quat(vn), r0);
                        double s3[3] = {0.0, 0.0, 0.0};  // ||db||^2, ||e_new||^2, dL over the points
                        for (int k = tid; k < n; k += kBaThreads) {
                            double inv[6], ebv[3], r[3], db[3], Mn[3], e[4];
                            for (int c = 0; c < 6; ++c) inv[c] = WSV(kSInv + cur_inv * 6 + c, k);
                            const double im[3][3] = {{inv[0], inv[1], inv[2]}, {inv[1], inv[3], inv[4]}, {inv[2], inv[4], inv[5]}};
#pragma unroll
                            for (int ii = 0; ii < 3; ++ii) {
                                ebv[ii] = WSV(kSEb + ii, k);
                                double wt = WSV(kSW + ii, k) * da[0];
#pragma unroll
                                for (int jj = 1; jj < 6; ++jj) wt = wt + WSV(kSW + jj * 3 + ii, k) * da[jj];
                                r[ii] = ebv[ii] - wt;
                            }
#pragma unroll
                            for (int ii = 0; ii < 3; ++ii) {
                                db[ii] = im[ii][0] * r[0] + im[ii][1] * r[1] + im[ii][2] * r[2];
                                Mn[ii] = WSV(kSM + cur_m * 3 + ii, k) + db[ii];
                                WSV(kSM + (cur_m ^ 1) * 3 + ii, k) = Mn[ii];
                                s3[0] += db[ii] * db[ii];
                                s3[2] += db[ii] * (mu * db[ii] + ebv[ii]);
                            }
                            const size_t at = row0 + idx[k];
                            const double x1[2] = {p1[at * 2], p1[at * 2 + 1]}, x2[2] = {p2[at * 2], p2[at * 2 + 1]};
                            residual2(q_id, zero3, Mn, x1, th, e);
                            residual2(q1, tn, Mn, x2, th, e + 2);
                            for (int c = 0; c < 4; ++c) {
                                WSV(kSE + (cur_e ^ 1) * 4 + c, k) = e[c];
                                s3[1] += e[c] * e[c];
                            }
                        }
                        block_sum(s3, red);
                        dp_L2 = 0.0;
                        double dL = 0.0;
                        for (int k = 0; k < 6; ++k) {
                            dp_L2 += da[k] * da[k];
                            dL += da[k] * (mu * da[k] + ea[k]);
                        }
                        dp_L2 += s3[0];
                        dL += s3[2];
                        const double pdp_eL2 = s3[1];
                        if (dp_L2 <= eps2_sq * p_L2) {
                            stop = 2;
                            break;
                        }
                        if (dp_L2 >= (p_L2 + eps2) / (1E-12 * 1E-12)) {  // "almost singular": the optimiser fails, info stays unwritten
                            failed = true;
                            break;
                        }
                        ++nfev;
                        if (!isfinite(pdp_eL2)) {
                            stop = 7;
                            break;
                        }
                        const double dF = p_eL2 - pdp_eL2;
                        if (dL > 0.0 && dF > 0.0) {
                            double tmp = 2.0 * dF / dL - 1.0;
                            tmp = 1.0 - tmp * tmp * tmp;
                            mu = mu * ((tmp >= 0.3333333334) ? tmp : 0.3333333334);
                            nu = 2;
                            if (pdp_eL2 - 2.0 * sqrt(p_eL2 * pdp_eL2) < (eps4_sq - 1.0) * p_eL2) stop = 4;
                            for (int k = 0; k < 3; ++k) v[k] = vn[k], t[k] = tn[k];
                            cur_m ^= 1, cur_e ^= 1;
                            p_eL2 = pdp_eL2;
                            accepted = true;
                        }
                    }
                }
                if (accepted) break;
                mu *= nu;
                if (nu >= (1 << 30)) {  // 2 nu no longer fits an int
                    stop = 6;
                    break;
                }
                nu *= 2;
            }
            if (failed) break;
            if (p_eL2 <= eps3_sq) stop = 5;
        }
        if (!failed) {
            if (itno >= kBaMaxIter) stop = 3;
            info[0] = init_p_eL2, info[1] = p_eL2, info[2] = eab_inf, info[3] = dp_L2;
            if (have_diag) info[4] = mu / max_diag;
            info[5] = itno, info[6] = stop, info[7] = nfev, info[8] = njev, info[9] = nlss;
            sba_ok = stop != 7;
        } else {
            mu = 0.0;
        }
    }

    // ---- the wrapper: the refined pose, the acceptance rule, the scatter of the points
    bool accept = false;
    double Rout[9], tout[3];
    for (int k = 0; k < 9; ++k) Rout[k] = Rin[k];
    for (int k = 0; k < 3; ++k) tout[k] = t0[k];
    if (sba_ok) {
        Quat qn = quat_mult_fast(local_quat(v), r0);
        if (qn.w < 0.0) qn = Quat{qn.w * -1.0, qn.x * -1.0, qn.y * -1.0, qn.z * -1.0};
        double tn[3] = {t[0], t[1], t[2]};
        const double t_norm = sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]);
        if (!(t_norm < 1e-3 && t_norm > -1e-3) && fabs(t_norm - 1.0) > 1e-4)
            for (int k = 0; k < 3; ++k) tn[k] = tn[k] / t_norm;
        double r_diff, t_diff;
        rt_quality(quat_old, qn, t0, tn, r_diff, t_diff);
        r_diff = r_diff / M_PI * 180.0;
        if (!(fabs(r_diff) > angle_thresh || t_diff > t_norm_thresh || info[6] > 5)) {
            accept = true;
            quat_to_matrix(qn, Rout);
            for (int k = 0; k < 3; ++k) tout[k] = tn[k];
        }
    }
    if (accept)
        for (int k = tid; k < n; k += kBaThreads) {
            const size_t at = row0 + idx[k];
            for (int c = 0; c < 3; ++c) Q[at * 3 + c] = WSV(kSM + cur_m * 3 + c, k);
        }
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) po[k] = Rout[k];
        for (int k = 0; k < 3; ++k) po[9 + k] = tout[k];
        for (int k = 0; k < 10; ++k) po[12 + k] = info[k];
        po[22] = mu;
        po[23] = accept ? 1.0 : 0.0;
    }
#undef WSV
}

thread_local std::vector<double> g_last_mu;  // mu at exit of the problems of the calling thread's last call (mlpl_debug_ba_last_mu)

// One launch for B problems.  R, t (host, in / out), th [B], accepted [B], info [B][10] or NULL.
int ba_run(mlpl_ctx *ctx, const char *who, int B, const double *d_p1, const double *d_p2, int stride, const int32_t *counts,
           const uint8_t *d_masks, double *d_Q, double *R, double *t, const double *th, double angle_thresh, double t_norm_thresh,
           int32_t *accepted, double *info, hipStream_t s) {
    if (B < 1 || stride < 1 || !d_p1 || !d_p2 || !d_Q || !counts || !R || !t || !th || !accepted) {
        set_error("%s: bad arguments", who);
        return MLPL_E_BAD_INPUT;
    }
    if (B > 65535) {
        set_error("%s: at most 65535 problems per call", who);
        return MLPL_E_BAD_INPUT;
    }
    for (int b = 0; b < B; ++b)
        if (counts[b] < 0 || counts[b] > stride) {
            set_error("%s: counts[%d] = %d outside [0, stride = %d]", who, b, counts[b], stride);
            return MLPL_E_BAD_INPUT;
        }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    const size_t off_in = 0, off_out = off_in + (size_t)B * kBaIn * 8, off_counts = off_out + (size_t)B * kBaOut * 8,
                 small_bytes = off_counts + (size_t)B * 4;
    const size_t rows = (size_t)B * stride, off_idx = rows * kBaSlots * 8;
    void *d_small, *d_ws;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX2, small_bytes, &d_small))) return rc;
    if ((rc = ws_get(ctx, WS_BA, off_idx + rows * 4, &d_ws))) return rc;
    std::vector<char> h(small_bytes, 0);
    double *hin = (double *)(h.data() + off_in);
    for (int b = 0; b < B; ++b) {
        std::memcpy(hin + (size_t)b * kBaIn, R + 9 * b, 72);
        std::memcpy(hin + (size_t)b * kBaIn + 9, t + 3 * b, 24);
        hin[(size_t)b * kBaIn + 12] = th[b];
        hin[(size_t)b * kBaIn + 13] = angle_thresh;
        hin[(size_t)b * kBaIn + 14] = t_norm_thresh;
    }
    std::memcpy(h.data() + off_counts, counts, (size_t)B * 4);
    MLPL_HIP_TRY(hipMemcpyAsync(d_small, h.data(), small_bytes, hipMemcpyHostToDevice, s));
    char *sm = (char *)d_small;
    prof_mark(ctx, MLPL_PROF_BUNDLE_ADJUST, 0, s);
    hipLaunchKernelGGL(bundle_adjust_kernel, dim3(B), dim3(kBaThreads), 0, s, (const double *)(sm + off_in), d_p1, d_p2,
                       (const int32_t *)(sm + off_counts), stride, d_masks, d_Q, (int32_t *)((char *)d_ws + off_idx), (double *)d_ws,
                       (double *)(sm + off_out));
    prof_mark(ctx, MLPL_PROF_BUNDLE_ADJUST, 1, s);
    MLPL_HIP_TRY(hipGetLastError());
    std::vector<double> ho((size_t)B * kBaOut);
    MLPL_HIP_TRY(hipMemcpyAsync(ho.data(), sm + off_out, ho.size() * 8, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    g_last_mu.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        const double *o = ho.data() + (size_t)b * kBaOut;
        accepted[b] = o[23] != 0.0;
        if (accepted[b]) {  // a refused or failed problem leaves R and t as they came
            std::memcpy(R + 9 * b, o, 72);
            std::memcpy(t + 3 * b, o + 9, 24);
        }
        if (info) std::memcpy(info + 10 * b, o + 12, 80);
        g_last_mu[(size_t)b] = o[22];
    }
    return MLPL_OK;
}

}  // namespace
}  // namespace mlpl

using namespace mlpl;

extern "C" int mlpl_refine_stereo_ba_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride,
                                               const int32_t *counts, const uint8_t *d_masks, double *d_Q, double *R, double *t,
                                               const double *th, double angle_thresh, double t_norm_thresh, int32_t *accepted, double *info,
                                               void *stream) {
    if (!ctx) {
        set_error("mlpl_refine_stereo_ba_batch_dev: ctx is mandatory");
        return MLPL_E_BAD_INPUT;
    }
    return ba_run(ctx, "mlpl_refine_stereo_ba_batch_dev", n_problems, d_p1, d_p2, stride, counts, d_masks, d_Q, R, t, th, angle_thresh,
                  t_norm_thresh, accepted, info, pick_stream(ctx, stream));
}

extern "C" int mlpl_refine_stereo_ba_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const uint8_t *d_mask, double R[9],
                                         double t[3], double *d_Q, double th, double angle_thresh, double t_norm_thresh, double info[10],
                                         void *stream) {
    if (!ctx || n < 0) {
        set_error("mlpl_refine_stereo_ba_dev: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    if (info) std::memset(info, 0, 80);
    if (n == 0) return 0;
    const int32_t count = n;
    int32_t acc = 0;
    const int rc = ba_run(ctx, "mlpl_refine_stereo_ba_dev", 1, d_p1, d_p2, n, &count, d_mask, d_Q, R, t, &th, angle_thresh, t_norm_thresh, &acc,
                          info, pick_stream(ctx, stream));
    return rc ? rc : acc;
}

extern "C" int mlpl_refine_stereo_ba(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const uint8_t *mask, double R[9], double t[3],
                                     double *Q, double th, double angle_thresh, double t_norm_thresh, double info[10]) {
    if (!ctx || n < 0 || (n > 0 && (!p1 || !p2 || !Q)) || !R || !t) {
        set_error("mlpl_refine_stereo_ba: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    if (info) std::memset(info, 0, 80);
    if (n == 0) return 0;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    void *dp1, *dp2, *dQ, *dmask = nullptr;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, (size_t)n * 16, &dp1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX1, (size_t)n * 16, &dp2))) return rc;
    if ((rc = ws_get(ctx, WS_AUX5, (size_t)n * 24, &dQ))) return rc;
    if (mask && (rc = ws_get(ctx, WS_AUX6, (size_t)n, &dmask))) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(dp1, p1, (size_t)n * 16, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(dp2, p2, (size_t)n * 16, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(dQ, Q, (size_t)n * 24, hipMemcpyHostToDevice, s));
    if (mask) MLPL_HIP_TRY(hipMemcpyAsync(dmask, mask, (size_t)n, hipMemcpyHostToDevice, s));
    const int32_t count = n;
    int32_t acc = 0;
    if ((rc = ba_run(ctx, "mlpl_refine_stereo_ba", 1, (const double *)dp1, (const double *)dp2, n, &count, (const uint8_t *)dmask, (double *)dQ,
                     R, t, &th, angle_thresh, t_norm_thresh, &acc, info, s)))
        return rc;
    if (acc) MLPL_HIP_TRY(hipMemcpy(Q, dQ, (size_t)n * 24, hipMemcpyDeviceToHost));
    return acc;
}

extern "C" int mlpl_debug_ba_last_mu(double *mu, int max_items) {
    if (!mu || max_items < 0) return MLPL_E_BAD_INPUT;
    const int n = std::min<int>((int)g_last_mu.size(), max_items);
    for (int i = 0; i < n; ++i) mu[i] = g_last_mu[(size_t)i];
    return n;
}
