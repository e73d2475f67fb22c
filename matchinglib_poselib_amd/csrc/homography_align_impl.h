// homography_align_impl.h -- the pose-from-planes half of poselib::estimatePoseHomographies on the MI355X: Homographys_Alignment
// (poselib/source/HomographyAlignment.cpp:197-360) and its caller's part (ComputeHomographyMotion :82-171, pose_homography.cpp:195-213).
// Included by ransac_5pt.hip inside namespace mlpl after homography_impl.h (its batch entry runs on that file's homography_batch_drive, a
// caller of batch_hub.h's hub_batch_drive).
//
// The algorithm is a long chain of small dependent solves, each fed by sums over all correspondences: two candidate motions from the
// Longuet-Higgins decomposition of plane 0's homography, and for each of them up to 4 outer turns of up to 40 rounds of {a 3 x 3 system
// per further plane (update_dn), one 11 x 11 system over all planes (update_h0_rt), the mean transfer error (check_error)}, a new
// decomposition after every turn.  Round by round that would be about a thousand launches with host hops; here ONE workgroup runs a
// whole problem in ONE launch (homog_align_body, HK_HOM_ALIGN), and a batch is one merged launch for all its problems.
//   * the correspondences are sorted by plane once (a stable compaction per plane, one wave per plane, the offsets come from the host's
//     num_inl) into LDS (up to kAlignCache rows) or, beyond that, into a global block that is then re-read from L2 every round;
//   * sums go in a fixed order: a thread walks the planes in order and a plane's rows with the block stride, the wave folds by
//     butterfly, one thread adds the waves' partial sums in wave order.  No atomics: the result does not depend on how it was launched;
//   * the 11 x 11 normal system is symmetric and each of a correspondence's two rows has five structural zeros: a thread keeps the
//     50 + 11 terms that can be non-zero in registers (of the 66 + 11 unique ones), nothing per thread is staged in LDS;
//   * the small serial parts (cyclic Jacobi of H^T H, the decomposition, the LU with row equilibration and implicit pivoting) run on one
//     lane; the eleven unit-vector solves that make the reference's inverse run on eleven lanes.
// fp64 throughout.  Pinned by tests: this code against the sequential restatement tests/cpp/homography_align_oracle.cpp (whose head lists
// what is restated from memory of OpenCV and the defined failures); not pinned: that restatement against a build of the reference.

namespace {

constexpr int kAlignThreads = 256;
constexpr int kAlignWaves = kAlignThreads / 64;
constexpr int kAlignCache = 1536;      // rows kept in LDS (48 KiB)
constexpr int kAlignMaxPlanes = 64;    // (estimatePoseHomographies asks for at most 50)
constexpr int kAlignInfo = 24;
constexpr int kAlignOutHead = kAlignInfo + 21;  // info, R, t, E; then 3 P normals and 9 P homographies

struct HomAlignArgs {  // one workgroup of kAlignThreads
    KHdr hdr;
    const double *p1, *p2;
    const int32_t *labels;
    int n, P;
    double H0[9];
    double tol;
    double4 *pts;  // off[P] rows: the sorted correspondences when they do not fit LDS
    double *out;   // kAlignOutHead + 12 P doubles
    int32_t *zero;  // optional: a counter the launch clears (the final mask's, launched behind it)
    int32_t off[kAlignMaxPlanes + 1];
};

__device__ __forceinline__ void hal_mul33(const double *a, const double *b, double *c) {
    double r[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j];
            r[i * 3 + j] = s;
        }
    for (int i = 0; i < 9; ++i) c[i] = r[i];
}
__device__ __forceinline__ void hal_mulv(const double *a, const double *x, double *y) {
    double r[3];
    for (int i = 0; i < 3; ++i) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * x[k];
        r[i] = s;
    }
    y[0] = r[0], y[1] = r[1], y[2] = r[2];
}
__device__ __forceinline__ double hal_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ double hal_norm3(const double *a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
__device__ __forceinline__ double hal_det33(const double *m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ __forceinline__ void hal_inv33(const double *s, double *t) {  // cv::Mat::inv() of a 3 x 3: the zero matrix when det == 0
    double d = hal_det33(s);
    if (d != 0.) {
        d = 1. / d;
        const double r[9] = {(s[4] * s[8] - s[5] * s[7]) * d, (s[2] * s[7] - s[1] * s[8]) * d, (s[1] * s[5] - s[2] * s[4]) * d,
                             (s[5] * s[6] - s[3] * s[8]) * d, (s[0] * s[8] - s[2] * s[6]) * d, (s[2] * s[3] - s[0] * s[5]) * d,
                             (s[3] * s[7] - s[4] * s[6]) * d, (s[1] * s[6] - s[0] * s[7]) * d, (s[0] * s[4] - s[1] * s[3]) * d};
        for (int i = 0; i < 9; ++i) t[i] = r[i];
    } else {
        for (int i = 0; i < 9; ++i) t[i] = 0;
    }
}

__device__ __forceinline__ void hal_rot_pair(double *a, int i, int j, int k, int l, double s, double tau) {
    const double g = a[i * 3 + j], h = a[k * 3 + l];
    a[i * 3 + j] = g - s * (h + g * tau);
    a[k * 3 + l] = h + s * (g - h * tau);
}
__device__ __forceinline__ void hal_swap_cols(double *v, int c0, int c1) {
    for (int r = 0; r < 3; ++r) {
        const double t = v[r * 3 + c0];
        v[r * 3 + c0] = v[r * 3 + c1], v[r * 3 + c1] = t;
    }
}
// (Every helper below is force-inlined on purpose: a kernel that CALLS a function takes part in the module-wide LDS layout of this
// translation unit, and with 61 KiB of its own this one pushed the noinline helpers of homog_sample onto a run-time offset table.)
// jacobi_mat_33 (:873-1009): cyclic Jacobi, at most 50 sweeps, ended by an off-diagonal sum below 1e-6; eigenvalues descending
__device__ __forceinline__ void hal_jacobi33(const double *a_in, double *d, double *v) {
    double a[9], b[3], z[3];
    for (int i = 0; i < 9; ++i) a[i] = a_in[i], v[i] = 0.0;
    for (int p = 0; p < 3; ++p) v[p * 3 + p] = 1.0, b[p] = d[p] = a[p * 3 + p], z[p] = 0.0;
    for (int sweep = 1; sweep <= 50; ++sweep) {
        const double sm = fabs(a[1]) + fabs(a[2]) + fabs(a[5]);
        if (sm < 0.000001) {
            if (d[1] > d[0]) { const double c = d[0]; d[0] = d[1], d[1] = c; hal_swap_cols(v, 0, 1); }
            if (d[2] > d[1]) { const double c = d[1]; d[1] = d[2], d[2] = c; hal_swap_cols(v, 1, 2); }
            if (d[1] > d[0]) { const double c = d[0]; d[0] = d[1], d[1] = c; hal_swap_cols(v, 0, 1); }
            return;
        }
        const double tresh = sweep < 4 ? 0.2 * sm / 9 : 0.0;
        for (int k = 0; k < 3; ++k) {
            const int ip = k == 2 ? 1 : 0, iq = k == 0 ? 1 : 2;
            const double g = 100.0 * fabs(a[ip * 3 + iq]);
            if (sweep > 4 && (fabs(d[ip]) + g) == fabs(d[ip]) && (fabs(d[iq]) + g) == fabs(d[iq])) {
                a[ip * 3 + iq] = 0.0;
            } else if (fabs(a[ip * 3 + iq]) > tresh) {
                double h = d[iq] - d[ip], t;
                if ((fabs(h) + g) == fabs(h)) {
                    t = a[ip * 3 + iq] / h;
                } else {
                    const double theta = 0.5 * h / a[ip * 3 + iq];
                    t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / sqrt(1 + t * t), s = t * c, tau = s / (1.0 + c);
                h = t * a[ip * 3 + iq];
                z[ip] -= h, z[iq] += h, d[ip] -= h, d[iq] += h;
                a[ip * 3 + iq] = 0.0;
                for (int j = 0; j <= ip - 1; ++j) hal_rot_pair(a, j, ip, j, iq, s, tau);
                for (int j = ip + 1; j <= iq - 1; ++j) hal_rot_pair(a, ip, j, j, iq, s, tau);
                for (int j = iq + 1; j < 3; ++j) hal_rot_pair(a, ip, j, iq, j, s, tau);
                for (int j = 0; j < 3; ++j) hal_rot_pair(v, j, ip, j, iq, s, tau);
            }
        }
        for (int p = 0; p < 3; ++p) b[p] += z[p], d[p] = b[p], z[p] = 0.0;
    }
}

// Longuet_Higgins_Solution (:577-718) / ..._with_initial (:733-856): the candidates (R, t, n) with n(2) > 0 of H ~ R (I - t n^T).
// Returns 1, 2 for the degenerate-rotation branch (both candidates R = H / sqrt(d1), t = n = 0), 0 when H is refused, -1 when fewer
// than two candidates pass (the last two are -3 for the caller: reasons 1 and 2).
__device__ __forceinline__ int hal_decompose(const double *H, double *R2, double *t2, double *n2) {
    double W[9], u[9], hn[9], d[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += H[k * 3 + i] * H[k * 3 + j];
            W[i * 3 + j] = s;
        }
    hal_jacobi33(W, d, u);
    const double d2 = 1.0 / sqrt(d[1]);
    for (int i = 0; i < 9; ++i) hn[i] = d2 * H[i];
    d[0] = d[0] / d[1], d[2] = d[2] / d[1], d[1] = 1.0;
    if (d[0] - d[1] < 0.000001 && d[1] - d[2] < 0.000001) {
        for (int c = 0; c < 2; ++c) {
            for (int i = 0; i < 9; ++i) R2[c * 9 + i] = hn[i];
            for (int j = 0; j < 3; ++j) t2[c * 3 + j] = 0, n2[c * 3 + j] = 0;
        }
        return 2;
    }
    if (!(d[0] > 1.0 && d[2] <= 1.0)) return 0;
    const double den = d[0] - d[2];
    const double t0 = sqrt((d[0] - 1.0) * d[2] / den), tz = sqrt((1.0 - d[2]) * d[0] / den);
    const double q0 = sqrt((d[0] - 1.0) * d[0] / den), qz = sqrt((1.0 - d[2]) * d[2] / den);
    int nc = 0;
    for (int s1 = -1; s1 <= 1; s1 += 2)
        for (int s2 = -1; s2 <= 1; s2 += 2) {
            const double ps0 = -s1 * q0, ps2 = -s2 * qz;
            const double nv[3] = {s1 * t0 + ps0, 0.0, s2 * tz + ps2}, ts[3] = {s1 * t0, 0.0, s2 * tz};
            double trans[3], plane[3];
            hal_mulv(u, ts, trans);
            hal_mulv(u, nv, plane);
            if (plane[2] > 0.0) {
                if (nc < 2)
                    for (int j = 0; j < 3; ++j) t2[nc * 3 + j] = trans[j], n2[nc * 3 + j] = plane[j];
                ++nc;
            }
        }
    if (nc < 2) return -1;
    for (int c = 0; c < 2; ++c) {
        double tn[9], inv[9];
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) tn[j * 3 + k] = t2[c * 3 + j] * n2[c * 3 + k];
        tn[0] -= 1.0, tn[4] -= 1.0, tn[8] -= 1.0;
        for (int j = 0; j < 9; ++j) tn[j] = -1.0 * tn[j];
        hal_inv33(tn, inv);
        hal_mul33(hn, inv, R2 + c * 9);
        if (hal_det33(R2 + c * 9) < 0.0)
            for (int j = 0; j < 9; ++j) R2[c * 9 + j] = -1.0 * R2[c * 9 + j];
    }
    return 1;
}

// LU_decompose_D (:1399-1456) on the TRANSPOSE of a (11 x 11 in LDS): row equilibration, implicit pivoting.  0 = singular.
__device__ __forceinline__ int hal_lu11(const double *a, double *lu, int *ps, double *scales) {
    constexpr int n = 11;
    for (int i = 0; i < n; ++i) {
        double biggest = 0.0;
        for (int j = 0; j < n; ++j) {
            const double v = fabs(lu[i * n + j] = a[j * n + i]);
            if (biggest < v) biggest = v;
        }
        if (biggest == 0.0) return 0;
        scales[i] = 1.0 / biggest;
        ps[i] = i;
    }
    for (int k = 0; k < n - 1; ++k) {
        double biggest = 0.0;
        int pivotindex = k;
        for (int i = k; i < n; ++i) {
            const double v = fabs(lu[ps[i] * n + k]) * scales[ps[i]];
            if (biggest < v) biggest = v, pivotindex = i;
        }
        if (biggest == 0.0) return 0;
        if (pivotindex != k) {
            const int j = ps[k];
            ps[k] = ps[pivotindex], ps[pivotindex] = j;
        }
        const double pivot = lu[ps[k] * n + k];
        for (int i = k + 1; i < n; ++i) {
            const double mult = lu[ps[i] * n + k] = lu[ps[i] * n + k] / pivot;
            if (mult != 0.0)
                for (int j = k + 1; j < n; ++j) lu[ps[i] * n + j] -= mult * lu[ps[k] * n + j];
        }
    }
    return lu[ps[n - 1] * n + n - 1] != 0.0;
}

__host__ __device__ constexpr bool hal_in_x(int j) { return j == 0 || j == 1 || j == 2 || j == 6 || j == 7 || j == 8 || j == 10; }
__host__ __device__ constexpr bool hal_in_y(int j) { return j == 3 || j == 4 || j == 5 || j == 6 || j == 7 || j == 9 || j == 10; }
__host__ __device__ constexpr int hal_tri(int j, int l) { return j * 11 - j * (j - 1) / 2 + (l - j); }  // j <= l < 11

__device__ __forceinline__ void homog_align_body(const HomAlignArgs &a, int, int) {
    __shared__ double4 s_pts[kAlignCache];
    __shared__ double s_red[kAlignWaves][78];
    __shared__ double s_a[121], s_b[11], s_lu[121], s_x[11][12], s_scales[11];
    __shared__ int s_ps[11];
    __shared__ double s_dn[3 * kAlignMaxPlanes], s_dn0[3 * kAlignMaxPlanes], s_hk[9 * kAlignMaxPlanes];
    __shared__ double s_h0[9], s_rt0[3], s_rot[9], s_dt[3], s_nb[3];
    __shared__ double s_cR[18], s_ct[6], s_cn[6];        // the two initial candidates
    __shared__ double s_rR[18], s_rt[6], s_rn[6];        // the two results
    __shared__ double s_val[2], s_info[kAlignInfo];
    __shared__ int s_cnt[kAlignMaxPlanes], s_flag[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.P, n = a.n, n_used = a.off[P];
    const bool cached = n_used <= kAlignCache;
    double *__restrict__ out = a.out;
    const double tol = a.tol;

    auto finish = [&](int reason) {  // every thread calls it at the same point
        __syncthreads();
        if (tid == 0) {
            if (reason) s_info[0] = -3, s_info[17] = reason;
        }
        __syncthreads();
        if (tid < kAlignInfo) out[tid] = s_info[tid];
    };
    auto row = [&](int i) -> double4 { return cached ? s_pts[i] : a.pts[i]; };
    // (sum, count) over the block in a fixed order; every thread gets the totals
    auto block_sum2 = [&](double v0, double v1, double &r0, double &r1) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v0 += __shfl_xor(v0, off), v1 += __shfl_xor(v1, off);
        __syncthreads();
        if (lane == 0) s_red[wave][0] = v0, s_red[wave][1] = v1;
        __syncthreads();
        if (tid == 0) {
            double t0 = s_red[0][0], t1 = s_red[0][1];
            for (int w = 1; w < kAlignWaves; ++w) t0 += s_red[w][0], t1 += s_red[w][1];
            s_val[0] = t0, s_val[1] = t1;
        }
        __syncthreads();
        r0 = s_val[0], r1 = s_val[1];
    };
    // Check_motion_error (:1012-1084): mean distance of the closest points of the two viewing rays; false when no pair counted
    auto motion_error = [&](const double *Rs, const double *ts, double &err) -> bool {
        double R[9], t[3];
        for (int i = 0; i < 9; ++i) R[i] = Rs[i];
        for (int i = 0; i < 3; ++i) t[i] = ts[i];
        double sum = 0, cnt = 0;
        for (int i = tid; i < n_used; i += kAlignThreads) {
            const double4 p = row(i);
            const double va[3] = {p.x, p.y, 1.0}, vb[3] = {p.z, p.w, 1.0};
            const double ia = 1. / hal_norm3(va);
            const double r1[3] = {va[0] * ia, va[1] * ia, va[2] * ia};
            double pb[3];
            for (int j = 0; j < 3; ++j) {
                double s = 0;
                for (int k = 0; k < 3; ++k) s += R[k * 3 + j] * vb[k];
                pb[j] = s;
            }
            const double ib = 1. / hal_norm3(pb);
            const double r2[3] = {pb[0] * ib, pb[1] * ib, pb[2] * ib};
            const double dotp = hal_dot3(r1, r2);
            if (fabs(dotp) > 0.9999999) continue;
            const double bv1 = hal_dot3(t, r1), bv2 = hal_dot3(t, r2);
            double m1, m2;
            if (dotp == 0.0) {
                m1 = bv1, m2 = bv2;
            } else {
                m1 = (bv1 - bv2 * dotp) / (1.0 - dotp * dotp);
                m2 = dotp * m1 - bv2;
            }
            const double dp[3] = {m1 * r1[0] - (t[0] + m2 * r2[0]), m1 * r1[1] - (t[1] + m2 * r2[1]), m1 * r1[2] - (t[2] + m2 * r2[2])};
            sum += hal_norm3(dp);
            cnt += 1.0;
        }
        double S, C;
        block_sum2(sum, cnt, S, C);
        if (!(C > 0)) return false;
        err = S / C;
        return true;
    };
    // check_error (:1493-1539): mean transfer error under the planes' homographies h0 + rt dn_k^T (note the float cast of the count)
    auto transfer_error = [&]() -> double {
        __syncthreads();
        if (tid < P) {
            double h[9];
            for (int j = 0; j < 3; ++j)
                for (int l = 0; l < 3; ++l) h[3 * j + l] = s_h0[3 * j + l] + s_rt0[j] * s_dn[3 * tid + l];
            const double s = 1.0 / h[8];
            for (int j = 0; j < 9; ++j) s_hk[9 * tid + j] = s * h[j];
        }
        __syncthreads();
        double sum = 0;
        for (int k = 0; k < P; ++k) {
            double h[9];
            for (int j = 0; j < 9; ++j) h[j] = s_hk[9 * k + j];
            for (int i = a.off[k] + tid; i < a.off[k + 1]; i += kAlignThreads) {
                const double4 p = row(i);
                const double w0 = h[0] * p.x + h[1] * p.y + h[2] * 1.0, w1 = h[3] * p.x + h[4] * p.y + h[5] * 1.0,
                             w2 = h[6] * p.x + h[7] * p.y + h[8] * 1.0;
                const double dx = w0 / w2 - p.z, dy = w1 / w2 - p.w;
                sum += sqrt(dx * dx + dy * dy);
            }
        }
        double S, C;
        block_sum2(sum, 0.0, S, C);
        return S / (float)n_used;
    };
    // update_dn (:1086-1143): plane k's offset from plane 0 by a 3 x 3 system, two rows per correspondence; one wave per plane
    auto update_dn = [&]() {
        __syncthreads();
        double h[9], k0[3];
        for (int j = 0; j < 9; ++j) h[j] = s_h0[j];
        for (int j = 0; j < 3; ++j) k0[j] = s_rt0[j];
        if (tid < 3) s_dn[tid] = 0;
        for (int k = 1 + wave; k < P; k += kAlignWaves) {
            double A[6] = {0, 0, 0, 0, 0, 0}, B[3] = {0, 0, 0};  // A: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
            for (int i = a.off[k] + lane; i < a.off[k + 1]; i += 64) {
                const double4 pt = row(i);
                const double p[3] = {pt.x, pt.y, 1.0};
                double hp[3];
                for (int j = 0; j < 3; ++j) hp[j] = h[3 * j] * p[0] + h[3 * j + 1] * p[1] + h[3 * j + 2] * p[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const double m = r ? pt.w : pt.z, d = k0[2] * m;
                    double t[3];
                    for (int j = 0; j < 3; ++j) t[j] = k0[r] * p[j] - d * p[j];
                    const double y = m * hp[2] - hp[r];
                    A[0] = t[0] * t[0] + A[0], A[1] = t[0] * t[1] + A[1], A[2] = t[0] * t[2] + A[2];
                    A[3] = t[1] * t[1] + A[3], A[4] = t[1] * t[2] + A[4], A[5] = t[2] * t[2] + A[5];
                    for (int j = 0; j < 3; ++j) B[j] = y * t[j] + B[j];
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int j = 0; j < 6; ++j) A[j] += __shfl_xor(A[j], off);
#pragma unroll
                for (int j = 0; j < 3; ++j) B[j] += __shfl_xor(B[j], off);
            }
            if (lane == 0) {
                const double M[9] = {A[0], A[1], A[2], A[1], A[3], A[4], A[2], A[4], A[5]};
                double inv[9], dn[3];
                hal_inv33(M, inv);
                hal_mulv(inv, B, dn);
                s_dn[3 * k] = dn[0], s_dn[3 * k + 1] = dn[1], s_dn[3 * k + 2] = dn[2];
            }
        }
        __syncthreads();
    };
    // update_h0_rt (:1145-1248): h0 (8 unknowns) and rt (3) from all planes; a singular system leaves both as they were
    auto update_h0_rt = [&]() {
        double acc[77];
#pragma unroll
        for (int j = 0; j < 77; ++j) acc[j] = 0;
        for (int k = 0; k < P; ++k) {
            const double d0 = s_dn[3 * k], d1 = s_dn[3 * k + 1], d2 = s_dn[3 * k + 2];
            for (int i = a.off[k] + tid; i < a.off[k + 1]; i += kAlignThreads) {
                const double4 p = row(i);
                const double dnp = p.x * d0 + p.y * d1 + 1.0 * d2;
                const double rx[11] = {p.x, p.y, 1.0, 0, 0, 0, -p.x * p.z, -p.y * p.z, dnp, 0, -p.z * dnp};
                const double ry[11] = {0, 0, 0, p.x, p.y, 1.0, -p.x * p.w, -p.y * p.w, 0, dnp, -p.w * dnp};
#pragma unroll
                for (int j = 0; j < 11; ++j) {
#pragma unroll
                    for (int l = j; l < 11; ++l) {
                        if (hal_in_x(j) && hal_in_x(l)) acc[hal_tri(j, l)] = rx[j] * rx[l] + acc[hal_tri(j, l)];
                        if (hal_in_y(j) && hal_in_y(l)) acc[hal_tri(j, l)] = ry[j] * ry[l] + acc[hal_tri(j, l)];
                    }
                    if (hal_in_x(j)) acc[66 + j] = p.z * rx[j] + acc[66 + j];
                    if (hal_in_y(j)) acc[66 + j] = p.w * ry[j] + acc[66 + j];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 11; ++j) {
#pragma unroll
            for (int l = j; l < 12; ++l) {  // l == 11: the right-hand side
                const int idx = l < 11 ? hal_tri(j, l) : 66 + j;
                if (l < 11 && !((hal_in_x(j) && hal_in_x(l)) || (hal_in_y(j) && hal_in_y(l)))) {  // structurally zero
                    if (tid == 0) s_red[0][idx] = 0;
                    continue;
                }
                double v = acc[idx];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                if (lane == 0) s_red[wave][idx] = v;
            }
        }
        __syncthreads();
        if (tid < 77) {
            double v = s_red[0][tid];
            int j = 0, rem = tid;
            if (tid < 66) {
                while (rem >= 11 - j) rem -= 11 - j, ++j;
                const bool live = (hal_in_x(j) && hal_in_x(j + rem)) || (hal_in_y(j) && hal_in_y(j + rem));
                if (live)
                    for (int w = 1; w < kAlignWaves; ++w) v += s_red[w][tid];
                s_a[j * 11 + j + rem] = v;
                s_a[(j + rem) * 11 + j] = v;
            } else {
                for (int w = 1; w < kAlignWaves; ++w) v += s_red[w][tid];
                s_b[tid - 66] = v;
            }
        }
        __syncthreads();
        if (tid == 0) s_flag[1] = hal_lu11(s_a, s_lu, s_ps, s_scales);
        __syncthreads();
        if (s_flag[1] && tid < 11) {  // row tid of the inverse (LU_solve_D on unit vector tid), then its product with b
            double *x = s_x[tid];
            for (int i = 0; i < 11; ++i) {
                double dot = 0.0;
                for (int j = 0; j < i; ++j) dot += s_lu[s_ps[i] * 11 + j] * x[j];
                x[i] = (s_ps[i] == tid ? 1.0 : 0.0) - dot;
            }
            for (int i = 10; i >= 0; --i) {
                double dot = 0.0;
                for (int j = i + 1; j < 11; ++j) dot += s_lu[s_ps[i] * 11 + j] * x[j];
                x[i] = (x[i] - dot) / s_lu[s_ps[i] * 11 + i];
            }
            double m = 0;
            for (int j = 0; j < 11; ++j) m += x[j] * s_b[j];
            if (tid < 8) s_h0[tid] = m;
            else s_rt0[tid - 8] = m;
            if (tid == 0) s_h0[8] = 1.0;
        }
        __syncthreads();
    };

    if (tid < kAlignInfo) s_info[tid] = 0;
    if (tid == 0 && a.zero) a.zero[0] = 0;
    // ---- the correspondences of plane k, in index order, to rows off[k] ...: one wave per plane
    for (int k = wave; k < P; k += kAlignWaves) {
        int fill = a.off[k];
        const int end = a.off[k + 1];
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            const bool m = i < n && a.labels[i] == k;
            const unsigned long long b = __ballot(m);
            if (m) {
                const int d = fill + __popcll(b & ((1ull << lane) - 1ull));
                if (d < end) {
                    const double4 v = make_double4(a.p1[2 * i], a.p1[2 * i + 1], a.p2[2 * i], a.p2[2 * i + 1]);
                    if (cached) s_pts[d] = v;
                    else a.pts[d] = v;
                }
            }
            fill += __popcll(b);
        }
        if (lane == 0) s_cnt[k] = fill - a.off[k];
    }
    __syncthreads();
    {
        int bad = 0;
        for (int k = 0; k < P; ++k) bad |= (s_cnt[k] != a.off[k + 1] - a.off[k]) || s_cnt[k] == 0;
        if (bad) return finish(6);
    }

    if (tid == 0) s_flag[0] = hal_decompose(a.H0, s_cR, s_ct, s_cn);
    __syncthreads();
    if (s_flag[0] <= 0) return finish(s_flag[0] == 0 ? 1 : 2);
    for (int c = 0; c < 2; ++c) {
        double e;
        if (!motion_error(s_cR + 9 * c, s_ct + 3 * c, e)) return finish(3);
        if (tid == 0) s_info[12 + c] = e;
    }
    int choice_bits = 0;  // thread 0's
    for (int q = 0; q < 2; ++q) {
        __syncthreads();
        if (tid == 0) {
            for (int j = 0; j < 9; ++j) s_h0[j] = a.H0[j], s_rot[j] = s_cR[9 * q + j];
            for (int j = 0; j < 3; ++j) s_dt[j] = s_ct[3 * q + j], s_nb[j] = 0;
            hal_mulv(s_cR + 9 * q, s_ct + 3 * q, s_rt0);
        }
        for (int k = tid; k < 3 * P; k += kAlignThreads) s_dn[k] = 0;
        double e1 = 0, e2 = 100000.0;
        for (int turn = 0; turn < 4; ++turn) {
            int iter;
            for (iter = 0; iter < 40; ++iter) {
                update_dn();
                update_h0_rt();
                e1 = transfer_error();
                if ((fabs(e1 - e2) < 0.00001 || e1 < tol) && iter > 2) break;
                e2 = e1;
            }
            __syncthreads();
            if (tid == 0) {
                s_info[2 + 4 * q + turn] = iter < 40 ? iter + 1 : 40;
                double R2[18], t2[6], n2[6];
                const int dr = hal_decompose(s_h0, R2, t2, n2);
                s_flag[0] = dr;
                if (dr > 0) {
                    const int pick = dr == 2 ? 0 : (hal_dot3(t2, s_dt) > hal_dot3(t2 + 3, s_dt) ? 0 : 1);
                    if (pick) choice_bits |= 1 << (4 * q + turn);
                    for (int j = 0; j < 3; ++j) s_dt[j] = t2[3 * pick + j], s_nb[j] = n2[3 * pick + j];
                    for (int j = 0; j < 9; ++j) s_rot[j] = R2[9 * pick + j];
                    hal_mulv(s_rot, s_dt, s_rt0);
                }
            }
            __syncthreads();
            if (s_flag[0] <= 0) return finish(s_flag[0] == 0 ? 1 : 2);
            e1 = transfer_error();
            if ((fabs(e1 - e2) < 0.000001 || e1 < tol) && iter > 2) break;
            e2 = e1;
        }
        __syncthreads();
        if (tid == 0) {
            for (int j = 0; j < 9; ++j) s_rR[9 * q + j] = s_rot[j];
            for (int j = 0; j < 3; ++j) s_rt[3 * q + j] = s_dt[j], s_rn[3 * q + j] = s_nb[j];
            s_info[10 + q] = e1;
        }
        if (q == 0)
            for (int k = tid; k < 3 * P; k += kAlignThreads) s_dn0[k] = s_dn[k];
    }
    __syncthreads();
    double errs[2];
    for (int c = 0; c < 2; ++c) {
        if (!motion_error(s_rR + 9 * c, s_rt + 3 * c, errs[c])) return finish(3);
        if (tid == 0) s_info[14 + c] = errs[c];
    }
    const int q = errs[0] < errs[1] ? 0 : 1;
    // ---- the chosen motion, the planes' normals and homographies (ComputeHomographyMotion, pose_homography.cpp:195-213): one lane
    if (tid == 0) {
        s_info[1] = q, s_info[16] = choice_bits;
        const double *t12 = s_rt + 3 * q, *n0 = s_rn + 3 * q, *R = s_rR + 9 * q;
        double hh[9], RI[9];
        for (int j = 0; j < 3; ++j)
            for (int l = 0; l < 3; ++l) hh[3 * j + l] = (j == l ? 1.0 : 0.0) - t12[j] * n0[l];
        hal_mul33(R, hh, RI);
        const double s1 = RI[8];
        bool ok = true;
        double *norms = out + kAlignOutHead, *Hs = norms + 3 * P;
        // (the reference takes the plane offsets of the FIRST candidate's run whichever q it chose: dn2.rowRange(0, num_patches))
        for (int k = 0; k < P; ++k) {
            double nk[3], tp[9], h[9];
            for (int l = 0; l < 3; ++l) nk[l] = k == 0 ? n0[l] : n0[l] - s1 * s_dn0[3 * k + l];
            for (int j = 0; j < 3; ++j)
                for (int l = 0; l < 3; ++l) tp[3 * j + l] = (j == l ? 1.0 : 0.0) - t12[j] * nk[l];
            hal_mul33(R, tp, h);
            if (fabs(h[8]) > 0.0) {
                const double s = 1.0 / h[8];
                for (int j = 0; j < 9; ++j) h[j] = s * h[j];
            }
            for (int l = 0; l < 3; ++l) norms[3 * k + l] = nk[l], ok = ok && isfinite(nk[l]);
            for (int j = 0; j < 9; ++j) Hs[9 * k + j] = h[j], ok = ok && isfinite(h[j]);
        }
        double t[3] = {-1.0 * t12[0], -1.0 * t12[1], -1.0 * t12[2]};
        const double normt = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        if (fabs(normt - 1.0) > 1e-4) {
            const double s = 1. / normt;
            for (int j = 0; j < 3; ++j) t[j] = t[j] * s;
        }
        const double su = 1. / sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        const double u[3] = {t[0] * su, t[1] * su, t[2] * su};
        const double sk[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
        double E[9];
        hal_mul33(sk, R, E);
        for (int j = 0; j < 9; ++j) out[kAlignInfo + j] = R[j], out[kAlignInfo + 12 + j] = E[j], ok = ok && isfinite(R[j]) && isfinite(E[j]);
        for (int j = 0; j < 3; ++j) out[kAlignInfo + 9 + j] = t[j], ok = ok && isfinite(t[j]);
        s_flag[0] = ok ? 1 : 0;
    }
    __syncthreads();
    finish(s_flag[0] ? 0 : 4);
}
MLPL_HUB_KERNEL(HK_HOM_ALIGN, HomAlignArgs, homog_align_body, kAlignThreads);

// The rows an input mask keeps, in their order (estimatePoseHomographies' first step, pose_homography.cpp:153-164): one wave.
struct HomMaskRowsArgs {
    KHdr hdr;
    const double *p1, *p2;
    const uint8_t *mask;
    int n;
    double *o1, *o2;
    int32_t *count;
};
__device__ __forceinline__ void homog_mask_rows_body(const HomMaskRowsArgs &a, int, int) {
    const int lane = threadIdx.x;
    int fill = 0;
    for (int base = 0; base < a.n; base += 64) {
        const int i = base + lane;
        const bool m = i < a.n && a.mask[i] != 0;
        const unsigned long long b = __ballot(m);
        if (m) {
            const int d = fill + __popcll(b & ((1ull << lane) - 1ull));
            a.o1[2 * d] = a.p1[2 * i], a.o1[2 * d + 1] = a.p1[2 * i + 1];
            a.o2[2 * d] = a.p2[2 * i], a.o2[2 * d + 1] = a.p2[2 * i + 1];
        }
        fill += __popcll(b);
    }
    if (lane == 0) a.count[0] = fill;
}
MLPL_HUB_KERNEL(HK_HOM_MASK_ROWS, HomMaskRowsArgs, homog_mask_rows_body, 64);

// estimatePoseHomographies' final mask (pose_homography.cpp:221-231): computeReprojError2 < th^2, strict, over all n rows under the E the
// alignment launched before it left in its result block (nothing is written when that block's code is not 0).  The arithmetic is
// inliers_strict_kernel's (reproj_error2.h); *count was cleared by the alignment launch.
struct HomStrictArgs {  // 256 threads per block
    KHdr hdr;
    const double *p1, *p2;
    int n;
    const double *align_out;
    double th2;
    uint8_t *mask;
    int32_t *count;
};
__device__ __forceinline__ void homog_strict_body(const HomStrictArgs &a, int bx, int) {
    if (a.align_out[0] != 0) return;
    const double *__restrict__ E = a.align_out + kAlignInfo + 12;
    const int i = bx * 256 + threadIdx.x;
    bool in = false;
    if (i < a.n) {
        in = reproj_error2_point(E, a.p1[2 * i], a.p1[2 * i + 1], a.p2[2 * i], a.p2[2 * i + 1]) < a.th2;
        a.mask[i] = in ? 1 : 0;
    }
    const unsigned long long b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.count, __popcll(b));
}
MLPL_HUB_KERNEL(HK_HOM_STRICT, HomStrictArgs, homog_strict_body, 256);

}  // namespace

// Homography alignment of one problem.  d_p1 / d_p2 / d_labels: device; num_inl, H0 and every output: host.  The outputs are written
// only when info[0] == 0; info (kAlignInfo doubles) always.  Returns MLPL_OK also for the code -3 (a result, not an error).
int homography_alignment_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, const int32_t *d_labels, int n, int P, const int32_t *num_inl,
                             const double *H0, double tol, double *R, double *t, double *E, double *norms, double *Hs_out, double *info, hipStream_t s) {
    if (P < 2) {  // ComputeHomographyMotion returns 0: t1_2 is empty (one plane), or there is no plane
        for (int i = 0; i < kAlignInfo; ++i) info[i] = 0;
        info[0] = -3, info[17] = 5;
        return MLPL_OK;
    }
    HomAlignArgs aa{};
    aa.hdr.gx = 1, aa.hdr.gy = 1;
    aa.p1 = d_p1, aa.p2 = d_p2, aa.labels = d_labels, aa.n = n, aa.P = P, aa.tol = tol;
    std::memcpy(aa.H0, H0, 72);
    aa.off[0] = 0;
    for (int k = 0; k < P; ++k) aa.off[k + 1] = aa.off[k] + num_inl[k];
    const size_t out_doubles = (size_t)kAlignOutHead + 12 * (size_t)P, out_bytes = ((out_doubles * 8 + 255) / 256) * 256;
    void *blk;
    int rc;
    if ((rc = ws_get(ctx, WS_HOMOG_ALIGN, out_bytes + (size_t)aa.off[P] * 32, &blk))) return rc;
    aa.out = (double *)blk;
    aa.pts = (double4 *)((char *)blk + out_bytes);
    Launcher L;
    L.s = s;
    L.launch(HK_HOM_ALIGN, aa);
    std::vector<double> h(out_doubles);
    MLPL_HIP_TRY(hipGetLastError());
    MLPL_HIP_TRY(hipMemcpyAsync(h.data(), aa.out, out_doubles * 8, hipMemcpyDeviceToHost, s));
    if ((rc = L.sync())) return rc;
    std::memcpy(info, h.data(), kAlignInfo * 8);
    if (info[0] != 0) return MLPL_OK;
    std::memcpy(R, h.data() + kAlignInfo, 72);
    std::memcpy(t, h.data() + kAlignInfo + 9, 24);
    std::memcpy(E, h.data() + kAlignInfo + 12, 72);
    std::memcpy(norms, h.data() + kAlignOutHead, (size_t)P * 24);
    std::memcpy(Hs_out, h.data() + kAlignOutHead + 3 * (size_t)P, (size_t)P * 72);
    return MLPL_OK;
}

// poselib::estimatePoseHomographies (pose_homography.cpp:127-269) behind its optional input mask, as ONE sequential program that a call
// alone and a run of a batch both execute (L launches now or records for the hub): the planes of the m kept rows q1 / q2
// (estimateMultHomographys with MAX_PLANES_PER_PAIR = 50, MIN_PTS_PLANE = 15), the plane-strength gate, then one chain of launches --
// the alignment, the strict mask over ALL n rows d_p1 / d_p2 under its E, the copies of the result block and of the count into the
// run's mapped block -- and one wait.  The alignment re-uses blocks of B the plane search is done with (the model table for its result,
// the packed-point block for the rows sorted by plane, a round's point buffer for the labels when the caller wants none).
// *result = the reference's 0 / -1 / -2 / -3; R, t, E, *n_inliers and d_mask_out are written only with 0.  n_planes / H / num_inl /
// strength (cap entries; all null or all set) and d_labels (m int32) describe the planes whenever the plane search ran.  Fewer than 4
// kept rows: the reference's loop does not run and reports no plane.
constexpr unsigned kPoseHomMaxPlanes = 50, kPoseHomMinPts = 15;

namespace {
static int pose_homographies_run(mlpl_ctx *ctx, const HomBufs &B, const double *d_p1, const double *d_p2, int n, const double *q1, const double *q2, int m,
                                 double th, int check_strength, int var_th, uint64_t *rng_state, int *result, double *R, double *t, double *E,
                                 int *n_inliers, uint8_t *d_mask_out, int cap, int *n_planes, double *H, int32_t *num_inl, double *strength,
                                 int32_t *d_labels, double *info, Launcher L) {
    const uint64_t rng_in[2] = {rng_state[0], rng_state[1]};
    int rc, np = 0;
    double Hs[kPoseHomMaxPlanes * 9], str[kPoseHomMaxPlanes], thu[kPoseHomMaxPlanes], info_local[kAlignInfo];
    int32_t num[kPoseHomMaxPlanes];
    if (!d_labels) d_labels = (int32_t *)(B.planes + B.pl_bufs);  // (the rounds' point buffers are free once the labels are written)
    if (m >= 4) {
        if ((rc = mult_homographies_run(ctx, B, q1, q2, m, th, var_th, kPoseHomMaxPlanes, kPoseHomMinPts, rng_state, (int)kPoseHomMaxPlanes, &np, Hs, num, str,
                                        thu, nullptr, d_labels, nullptr, L)))
            return rc;
    }
    if (!info) info = info_local;
    for (int i = 0; i < kAlignInfo; ++i) info[i] = 0;
    if (np < 0) {
        if (n_planes) *n_planes = -1;
        *result = -1;
        return MLPL_OK;
    }
    if (n_planes) {
        if (np > cap) {
            rng_state[0] = rng_in[0], rng_state[1] = rng_in[1];
            set_error("mlpl_pose_homographies: more than cap = %d planes found (the stream states were put back)", cap);
            return MLPL_E_BAD_INPUT;
        }
        *n_planes = np;
        std::memcpy(H, Hs, (size_t)np * 72);
        std::memcpy(num_inl, num, (size_t)np * 4);
        std::memcpy(strength, str, (size_t)np * 8);
    }
    if (check_strength) {
        double sum = 0;
        for (int k = 0; k < np; ++k)
            if (str[k] > 0.1) sum += str[k];
        if (!(sum > 0.5)) {
            *result = -2;
            return MLPL_OK;
        }
    }
    if (np < 2) {  // ComputeHomographyMotion returns 0: one plane only, or none
        info[0] = -3, info[17] = 5;
        *result = -3;
        return MLPL_OK;
    }
    HomAlignArgs aa{};
    aa.hdr.gx = 1, aa.hdr.gy = 1;
    aa.p1 = q1, aa.p2 = q2, aa.labels = d_labels, aa.n = m, aa.P = np, aa.tol = th;
    std::memcpy(aa.H0, Hs, 72);
    aa.off[0] = 0;
    for (int k = 0; k < np; ++k) aa.off[k + 1] = aa.off[k] + num[k];
    const size_t out_doubles = (size_t)kAlignOutHead + 12 * (size_t)np, out_b = HomBufs::up(out_doubles * 8);
    aa.out = (double *)(B.dev + B.d_H);
    aa.pts = (double4 *)(B.dev + B.d_pts);
    aa.zero = (int32_t *)(B.dev + B.d_ok);
    L.launch(HK_HOM_ALIGN, aa);
    HomStrictArgs sa{{(n + 255) / 256, 1}, d_p1, d_p2, n, aa.out, th * th, d_mask_out, aa.zero};
    L.launch(HK_HOM_STRICT, sa);
    hub_copy_bytes(L, aa.out, B.pin_dev + B.p_smp, out_doubles * 8);
    hub_copy_bytes(L, aa.zero, B.pin_dev + B.p_smp + out_b, 4);
    if ((rc = L.sync())) return rc;
    const double *h = (const double *)(B.pin + B.p_smp);
    std::memcpy(info, h, kAlignInfo * 8);
    if (info[0] != 0) {
        *result = -3;
        return MLPL_OK;
    }
    std::memcpy(R, h + kAlignInfo, 72);
    std::memcpy(t, h + kAlignInfo + 9, 24);
    std::memcpy(E, h + kAlignInfo + 12, 72);
    *n_inliers = *(const int32_t *)(B.pin + B.p_smp + out_b);
    *result = 0;
    return MLPL_OK;
}
}  // namespace

int pose_homographies_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const uint8_t *d_mask_in, double th, int check_strength, int var_th,
                          uint64_t *rng_state, int *result, double *R, double *t, double *E, int *n_inliers, uint8_t *d_mask_out, int cap, int *n_planes,
                          double *H, int32_t *num_inl, double *strength, int32_t *d_labels, double *info, hipStream_t s) {
    int rc, m = n;
    const double *q1 = d_p1, *q2 = d_p2;
    Launcher L;
    L.s = s;
    if (d_mask_in) {
        void *b1, *b2;
        const size_t pts_b = HomBufs::up((size_t)n * 16);
        if ((rc = ws_get(ctx, WS_AUX3, pts_b + 256, &b1))) return rc;
        if ((rc = ws_get(ctx, WS_AUX4, pts_b, &b2))) return rc;
        int32_t *d_cnt = (int32_t *)((char *)b1 + pts_b);
        HomMaskRowsArgs ma{{1, 1}, d_p1, d_p2, d_mask_in, n, (double *)b1, (double *)b2, d_cnt};
        L.launch(HK_HOM_MASK_ROWS, ma);
        MLPL_HIP_TRY(hipGetLastError());
        int32_t cnt = 0;
        MLPL_HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, s));
        MLPL_HIP_TRY(hipStreamSynchronize(s));
        m = cnt, q1 = (const double *)b1, q2 = (const double *)b2;
    }
    HomBufs B;
    if ((rc = B.get(ctx, n, true))) return rc;
    return pose_homographies_run(ctx, B, d_p1, d_p2, n, q1, q2, m, th, check_strength, var_th, rng_state, result, R, t, E, n_inliers, d_mask_out, cap,
                                 n_planes, H, num_inl, strength, d_labels, info, L);
}

// A batch of estimatePoseHomographies problems laid out as mult_homographies_batch_dev (no input masks): every problem a fiber running
// pose_homographies_run, the alignment / mask / copy launches of a cohort merged into one launch each.  Outputs per problem b: results[b],
// R + 9 b, t + 3 b, E + 9 b, n_inliers[b], its mask at d_masks + b * stride, n_planes[b], cap planes each of H / num_inl / strength,
// labels at d_labels + b * stride (may be null), info + 24 b (may be null).
int pose_homographies_batch_dev(mlpl_ctx *ctx, int nb, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, double th, int check_strength,
                                int var_th, uint64_t *rng_states, int32_t *results, double *R, double *t, double *E, int32_t *n_inliers, uint8_t *d_masks,
                                int cap, int32_t *n_planes, double *H, int32_t *num_inl, double *strength, int32_t *d_labels, double *info, int32_t *status,
                                hipStream_t s) {
    return homography_batch_drive(ctx, nb, counts, true, true, status, s, "mlpl_pose_homographies_batch_dev", [&](int b, const HomBufs &Bf, const Launcher &L) {
        const double *p1 = d_p1 + (size_t)b * stride * 2, *p2 = d_p2 + (size_t)b * stride * 2;
        const size_t at = (size_t)b * cap;
        int res = 0, ninl = 0, np = 0;
        const int r = pose_homographies_run(ctx, Bf, p1, p2, counts[b], p1, p2, counts[b], th, check_strength, var_th, rng_states + 2 * (size_t)b, &res,
                                            R + 9 * (size_t)b, t + 3 * (size_t)b, E + 9 * (size_t)b, &ninl, d_masks + (size_t)b * stride, cap, &np, H + at * 9,
                                            num_inl + at, strength + at, d_labels ? d_labels + (size_t)b * stride : nullptr,
                                            info ? info + (size_t)kAlignInfo * b : nullptr, L);
        results[b] = res, n_planes[b] = np;
        if (res == 0) n_inliers[b] = ninl;
        return r;
    });
}
