// ba_common.h -- what the bundle-adjustment kernels share (bundle_adjust.hip: the stereo pair; bundle_adjust_multicam.hip: m cameras): the
// quaternion algebra and projection of BA_driver.cpp / imgproj.c, the pseudo-Huber residual, the Jacobian blocks of one point in one frame,
// the fixed-order workgroup reductions and the wrapper's helpers of pose_helper.cpp.  tests/ba_oracle.py is the float64 restatement all of it
// follows operation by operation.
#pragma once
#include <cmath>

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

}  // namespace
}  // namespace mlpl
