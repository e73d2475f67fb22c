// bundle_adjust_multicam.hip -- poselib::refineMultCamBA, pointsInImgCoords == false, optimMotionOnly == false (P/source/pose_estim.cpp:1384-1735):
// motion and structure bundle adjustment of m cameras over one shared structure with the first camera fixed AT THE POSE GIVEN, i.e.
// SBAdriver::perform_sba (P/source/BA_driver.cpp:1878-2260, nconstframes = 1, one visibility map per camera) around sba_motstr_levmar_x
// (sba-1.6/sba_levmar.c:449-1400, mcon = 1) with the pseudo-Huber cost of BA_driver.cpp:2612-2648.  tests/ba_multicam_oracle.py is the float64
// restatement this file follows operation by operation; bundle_adjust.hip is its two-camera, full-visibility special case and shares
// ba_common.h with it.
//
// One workgroup of 256 lanes per problem (blockIdx.x), the whole Levenberg-Marquardt iteration inside ONE launch, the wrapper's acceptance
// rule and the write-back of the points included.  Point k belongs to lane k % 256 for the whole run, so the per-point state in the problem's
// workspace (the point and the residuals of the cameras that see it twice -- current / trial --, V_i, eb_i, (V*_i)^-1 twice, W_ij of every
// free camera) is only ever read by the lane that wrote it.  What all lanes share lives in LDS, sized by m through dynamic shared memory:
// the cameras' quaternions and parameters, U_j and ea_j of the free cameras, the reduced camera system S (6 (m - 1) square), its right-hand
// side and the solution.
//
// Every sum over points is: each lane over its points in ascending order, a butterfly over the 64 lanes of a wave, then
// (w0 + w1) + (w2 + w3) -- a fixed order, no atomics.  The sums over the CAMERAS of one point (V_i, eb_i, sum_j W_ij^T da_j) run in ascending
// camera order inside the owning lane, as the reference has them.  The Cholesky factorisation of S runs row by row over the workgroup with
// every dot product in the oracle's order (ascending row index); so does the forward substitution (column-oriented: the same order per
// unknown); the backward substitution's dot products run ascending from j + 1 in the oracle, which a column-oriented sweep would reverse, so
// one lane walks them.  The only freedom taken against the oracle is therefore the association of the sums over points.
//
// ba_common.h holds what this kernel shares with bundle_adjust.hip: the geometry, the reductions, and the Levenberg-Marquardt core (the slots
// up to kPCam, the damped inverse of V*_i with the reference's damping quirk, the first_bad repair, the point update, the optimiser's state
// and every stop).  U's diagonal keeps every earlier rejected mu here as it does there.
#include <climits>
#include <cstring>

#include "ba_common.h"
#include "mlpl_internal.h"

namespace mlpl {
namespace {

constexpr int kMcMaxCams = MLPL_BA_MAX_CAMS;
// this kernel's slots of the per-point state, behind the shared ones
constexpr int kPE = kPCam;  // per camera 2 x 2: the residual, current / trial; then per free camera 18: W_ij, 6 x 3 row-major
__host__ __device__ constexpr int mc_slots(int cams) { return kPE + 4 * cams + 18 * cams; }
__host__ __device__ constexpr int mc_in(int cams_stride) { return 4 + 12 * cams_stride; }    // th, angle_thresh, t_norm_thresh, -, R, t
__host__ __device__ constexpr int mc_out(int cams_stride) { return 12 + 12 * cams_stride; }  // info 10, mu, accepted, R, t
// doubles of dynamic LDS for m cameras: r0 4, the old quaternion 4, v 3, t 3, trial v 3, trial t 3, the projecting quaternion 4 per camera;
// U 36 per free camera; S, ea, E, da
__host__ __device__ constexpr int mc_lds_doubles(int m) { return 24 * m + 36 * (m - 1) + 36 * (m - 1) * (m - 1) + 18 * (m - 1); }

__device__ inline Quat lds_quat(const double *q) { return Quat{q[0], q[1], q[2], q[3]}; }
__device__ inline void quat_lds(double *q, const Quat &a) { q[0] = a.w, q[1] = a.x, q[2] = a.y, q[3] = a.z; }

__global__ __launch_bounds__(kBaThreads) void bundle_adjust_multicam_kernel(
    const double *__restrict__ in /*[B][mc_in]*/, const double *__restrict__ p /*[B][cams_stride][stride][2]*/,
    const uint8_t *__restrict__ vis_all /*[B][cams_stride][stride]*/, const int32_t *__restrict__ n_cams, const int32_t *__restrict__ counts,
    int cams_stride, int stride, double *__restrict__ Q /*[B][stride][3] in / out*/, double *__restrict__ ws_all /*[B][mc_slots(cams_stride)][stride]*/,
    double *__restrict__ out /*[B][mc_out]*/) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[4 * 42];
    __shared__ int red_i[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int m = n_cams[b], n = counts[b];
    const double *pin = in + (size_t)b * mc_in(cams_stride);
    double *po = out + (size_t)b * mc_out(cams_stride);
    if (m < 2 || m > kMcMaxCams || n < 1) {  // nothing to do: not accepted, info zero (the host leaves R and t alone)
        if (tid < 12) po[tid] = 0.0;
        return;
    }
    const int dim = 6 * (m - 1);
    double *r0 = lds, *qold = r0 + 4 * m, *v = qold + 4 * m, *t = v + 3 * m, *vn = t + 3 * m, *tn = vn + 3 * m, *qc = tn + 3 * m;
    double *U = qc + 4 * m, *Sm = U + 36 * (m - 1), *ea = Sm + dim * dim, *E = ea + dim, *da = E + dim;
    const size_t S = (size_t)stride;
    const size_t row0 = (size_t)b * stride;
    const PointWs pw{ws_all + row0 * mc_slots(cams_stride), S};
    const uint8_t *vis = vis_all + (size_t)b * cams_stride * S;
    const double *px = p + (size_t)b * cams_stride * S * 2;
    const int kPW = kPE + 4 * m;
#define SLOT_E(j, which) (kPE + ((j)*2 + (which)) * 2)
#define SLOT_W(j) (kPW + ((j)-1) * 18)
#define SEEN(j, k) (vis[(size_t)(j)*S + (k)] != 0)

    const double th = pin[0], angle_thresh = pin[1], t_norm_thresh = pin[2];
    if (tid < m) {
        const double *Rj = pin + 4 + 9 * tid;
        double Rin[9];
        for (int k = 0; k < 9; ++k) Rin[k] = Rj[k];
        const Quat qo = mat_to_quat(Rin);
        double mag = sqrt(qo.w * qo.w + qo.x * qo.x + qo.y * qo.y + qo.z * qo.z);
        mag = (qo.w >= 0.0 ? 1.0 : -1.0) / mag;
        quat_lds(qold + 4 * tid, qo);
        quat_lds(r0 + 4 * tid, Quat{qo.w * mag, qo.x * mag, qo.y * mag, qo.z * mag});
        for (int k = 0; k < 3; ++k) v[3 * tid + k] = 0.0, t[3 * tid + k] = pin[4 + 9 * cams_stride + 3 * tid + k];
    }
    __syncthreads();

    double info[10];
    for (int k = 0; k < 10; ++k) info[k] = 0.0;
    LmState lm;
    bool sba_ok = false;
    int cur_m = 0;

    // the number of measurements: fewer than unknowns (2 nvis < 6 m + 3 n, the fixed camera counted) and the optimiser refuses
    long long nvis;
    {
        double cnt[1] = {0.0};
        for (int k = tid; k < n; k += kBaThreads)
            for (int j = 0; j < m; ++j) cnt[0] += SEEN(j, k) ? 1.0 : 0.0;
        block_sum(cnt, red);
        nvis = (long long)cnt[0];
    }
    if (2 * nvis >= 6LL * m + 3LL * n) {
        // the points into the workspace, the residual at the start
        int cur_e = 0;
        if (tid < m) {
            double vv[3] = {v[3 * tid], v[3 * tid + 1], v[3 * tid + 2]};
            quat_lds(qc + 4 * tid, quat_mult_fast(local_quat(vv), lds_quat(r0 + 4 * tid)));
        }
        __syncthreads();
        {
            double acc[1] = {0.0};
            for (int k = tid; k < n; k += kBaThreads) {
                double M[3], e[2];
                for (int c = 0; c < 3; ++c) pw(kPM + c, k) = M[c] = Q[(row0 + k) * 3 + c];
                for (int j = 0; j < m; ++j) {
                    if (!SEEN(j, k)) continue;
                    const double x[2] = {px[((size_t)j * S + k) * 2], px[((size_t)j * S + k) * 2 + 1]};
                    const double tj[3] = {t[3 * j], t[3 * j + 1], t[3 * j + 2]};
                    residual2(lds_quat(qc + 4 * j), tj, M, x, th, e);
                    for (int c = 0; c < 2; ++c) {
                        pw(SLOT_E(j, 0) + c, k) = e[c];
                        acc[0] += e[c] * e[c];
                    }
                }
            }
            block_sum(acc, red);
            lm.start(acc[0]);
        }

        for (; lm.itno < kBaMaxIter && !lm.stop; ++lm.itno) {
            // ---- Jacobian blocks camera by camera: V_i, eb_i (all cameras), U_j, ea_j, W_ij (free cameras)
            ++lm.njev;
            for (int k = tid; k < n; k += kBaThreads)
                for (int c = 0; c < 3; ++c) pw(kPVu + c, k) = 0.0, pw(kPVd + c, k) = 0.0, pw(kPEb + c, k) = 0.0;
            for (int j = 0; j < m; ++j) {
                CamJ cam;
                {
                    const double vv[3] = {v[3 * j], v[3 * j + 1], v[3 * j + 2]}, tt[3] = {t[3 * j], t[3 * j + 1], t[3 * j + 2]};
                    cam_setup(lds_quat(r0 + 4 * j), vv, tt, j > 0, cam);
                }
                double sums[27];  // U_j upper 21, ea_j 6
#pragma unroll
                for (int k = 0; k < 27; ++k) sums[k] = 0.0;
                for (int k = tid; k < n; k += kBaThreads) {
                    if (!SEEN(j, k)) continue;
                    double M[3], e[2], A[2][6], B[2][3];
                    for (int c = 0; c < 3; ++c) M[c] = pw(kPM + cur_m * 3 + c, k);
                    for (int c = 0; c < 2; ++c) e[c] = pw(SLOT_E(j, cur_e) + c, k);
                    if (j > 0) {
                        jac_blocks<true>(cam, M, A, B);
                        int s = 0;
#pragma unroll
                        for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                            for (int jj = ii; jj < 6; ++jj) sums[s++] += A[0][ii] * A[0][jj] + A[1][ii] * A[1][jj];
#pragma unroll
                        for (int ii = 0; ii < 6; ++ii) sums[21 + ii] += A[0][ii] * e[0] + A[1][ii] * e[1];
#pragma unroll
                        for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                            for (int jj = 0; jj < 3; ++jj) pw(SLOT_W(j) + ii * 3 + jj, k) = A[0][ii] * B[0][jj] + A[1][ii] * B[1][jj];
                    } else {
                        jac_blocks<false>(cam, M, A, B);
                    }
#pragma unroll
                    for (int ii = 0; ii < 3; ++ii) {
#pragma unroll
                        for (int jj = ii; jj < 3; ++jj) {
                            const double val = B[0][ii] * B[0][jj] + B[1][ii] * B[1][jj];
                            const int slot = ii == jj ? kPVd + ii : kPVu + ii + jj - 1;
                            pw(slot, k) = pw(slot, k) + val;
                        }
                        pw(kPEb + ii, k) = pw(kPEb + ii, k) + (B[0][ii] * e[0] + B[1][ii] * e[1]);
                    }
                }
                if (j > 0) {
                    block_sum(sums, red);
                    if (tid == 0) {
                        double *Uj = U + 36 * (j - 1);
                        int s = 0;
#pragma unroll
                        for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                            for (int jj = ii; jj < 6; ++jj) Uj[ii * 6 + jj] = Uj[jj * 6 + ii] = sums[s++];
#pragma unroll
                        for (int ii = 0; ii < 6; ++ii) ea[6 * (j - 1) + ii] = sums[21 + ii];
                    }
                }
            }
            __syncthreads();
            // ---- ||J^T e||_inf, ||p||^2, the largest diagonal entry
            double mx_e = 0.0, mx_d = DBL_MIN;
            double sq[1] = {0.0};
            for (int k = tid; k < n; k += kBaThreads) {
                for (int c = 0; c < 3; ++c) {
                    const double d = pw(kPVd + c, k);
                    if (d > mx_d) mx_d = d;
                    mx_e = fmax(mx_e, fabs(pw(kPEb + c, k)));
                }
                for (int c = 0; c < 3; ++c) {
                    const double Mc = pw(kPM + cur_m * 3 + c, k);
                    sq[0] += Mc * Mc;
                }
            }
            block_sum(sq, red);
            mx_e = block_max(mx_e, red);
            mx_d = block_max(mx_d, red);
            for (int i = 0; i < dim; ++i) {
                mx_e = fmax(mx_e, fabs(ea[i]));
                const double d = U[36 * (i / 6) + (i % 6) * 7];
                if (d > mx_d) mx_d = d;
            }
            double p_L2 = 0.0;
            for (int j = 0; j < m; ++j) {
                for (int k = 0; k < 3; ++k) p_L2 += v[3 * j + k] * v[3 * j + k];
                for (int k = 0; k < 3; ++k) p_L2 += t[3 * j + k] * t[3 * j + k];
            }
            p_L2 += sq[0];
            if (!lm.after_gradient(mx_e, mx_d)) break;

            // ---- the damping loop
            bool vd_from_inv = false;  // V_i's diagonal currently lives in the previous attempt's inverse
            int cur_inv = 0;
            while (true) {
                __syncthreads();
                if (tid < dim) U[36 * (tid / 6) + (tid % 6) * 7] += lm.mu;
                int first_bad = INT_MAX;
                for (int k = tid; k < n; k += kBaThreads) {
                    double inv[6];
                    if (!damped_inverse(pw, k, vd_from_inv, cur_inv, lm.mu, inv) && k < first_bad) first_bad = k;
                }
                first_bad = block_min_int(first_bad, red_i);  // (its barriers also publish U's new diagonal)
                bool accepted = false;
                if (first_bad != INT_MAX) {
                    repair_first_bad(pw, n, first_bad, vd_from_inv, cur_inv, lm.mu);
                    vd_from_inv = false;
                } else {
                    cur_inv ^= 1, vd_from_inv = true;
                    // ---- S_jk = delta_jk U*_j - sum_i Y_ij W_ik^T, E_j = ea_j - sum_i Y_ij eb_i
                    for (int j = 1; j < m; ++j)
                        for (int kc = j; kc < m; ++kc) {
                            double acc[42];  // Y W^T 36 row-major, Y eb 6 (the diagonal block only)
#pragma unroll
                            for (int k = 0; k < 42; ++k) acc[k] = 0.0;
                            for (int k = tid; k < n; k += kBaThreads) {
                                if (!SEEN(j, k) || !SEEN(kc, k)) continue;
                                double inv[6], Y[6][3], Wk[6][3];
                                for (int c = 0; c < 6; ++c) inv[c] = pw(kPInv + cur_inv * 6 + c, k);
                                const double im[3][3] = {{inv[0], inv[1], inv[2]}, {inv[1], inv[3], inv[4]}, {inv[2], inv[4], inv[5]}};
#pragma unroll
                                for (int ii = 0; ii < 6; ++ii) {
                                    const double w0 = pw(SLOT_W(j) + ii * 3, k), w1 = pw(SLOT_W(j) + ii * 3 + 1, k), w2 = pw(SLOT_W(j) + ii * 3 + 2, k);
#pragma unroll
                                    for (int jj = 0; jj < 3; ++jj) Y[ii][jj] = w0 * im[0][jj] + w1 * im[1][jj] + w2 * im[2][jj];
                                }
#pragma unroll
                                for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                                    for (int jj = 0; jj < 3; ++jj) Wk[ii][jj] = pw(SLOT_W(kc) + ii * 3 + jj, k);
#pragma unroll
                                for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                                    for (int jj = 0; jj < 6; ++jj) acc[ii * 6 + jj] += Y[ii][0] * Wk[jj][0] + Y[ii][1] * Wk[jj][1] + Y[ii][2] * Wk[jj][2];
                                if (kc == j) {
                                    const double e0 = pw(kPEb, k), e1 = pw(kPEb + 1, k), e2 = pw(kPEb + 2, k);
#pragma unroll
                                    for (int ii = 0; ii < 6; ++ii) acc[36 + ii] += Y[ii][0] * e0 + Y[ii][1] * e1 + Y[ii][2] * e2;
                                }
                            }
                            block_sum(acc, red);
                            if (tid == 0) {
                                double *blk = Sm + (size_t)(6 * (j - 1)) * dim + 6 * (kc - 1);
                                const double *Uj = U + 36 * (j - 1);
#pragma unroll
                                for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                                    for (int jj = 0; jj < 6; ++jj) blk[ii * dim + jj] = kc == j ? Uj[ii * 6 + jj] - acc[ii * 6 + jj] : -acc[ii * 6 + jj];
                                if (kc == j)
#pragma unroll
                                    for (int ii = 0; ii < 6; ++ii) E[6 * (j - 1) + ii] = ea[6 * (j - 1) + ii] - acc[36 + ii];
                            }
                        }
                    __syncthreads();
                    // ---- upper Cholesky U^T U = S in place (ba_multicam_oracle.chol_solve), row by row: the diagonal entry by every lane, entry
                    // (j, j + 1 + tid) by lane tid, every dot product ascending in the row index
                    bool solved = true;
                    for (int j = 0; j < dim; ++j) {
                        double ajj = Sm[j * dim + j];
                        for (int i = 0; i < j; ++i) ajj = ajj - Sm[i * dim + j] * Sm[i * dim + j];
                        if (!(ajj > 0.0) || !isfinite(ajj)) {
                            solved = false;
                            break;
                        }
                        ajj = sqrt(ajj);
                        const double r = 1.0 / ajj;
                        const int kk = j + 1 + tid;
                        double val = 0.0;
                        if (kk < dim) {
                            double s = Sm[j * dim + kk];
                            for (int i = 0; i < j; ++i) s = s - Sm[i * dim + j] * Sm[i * dim + kk];
                            val = s * r;
                        }
                        __syncthreads();
                        if (tid == 0) Sm[j * dim + j] = ajj;
                        if (kk < dim) Sm[j * dim + kk] = val;
                        __syncthreads();
                    }
                    ++lm.nlss;
                    if (solved) {
                        // U^T y = E column by column (lane jj keeps its running right-hand side; y into E), then U x = y by one lane
                        double rhs = tid < dim ? E[tid] : 0.0;
                        for (int i = 0; i < dim; ++i) {
                            if (tid == i) E[i] = rhs / Sm[i * dim + i];
                            __syncthreads();
                            if (tid > i && tid < dim) rhs = rhs - Sm[i * dim + tid] * E[i];
                        }
                        if (tid == 0)
                            for (int j = dim - 1; j >= 0; --j) {
                                double s = E[j];
                                for (int i = j + 1; i < dim; ++i) s = s - Sm[j * dim + i] * da[i];
                                da[j] = s / Sm[j * dim + j];
                            }
                        __syncthreads();
                        // ---- the trial cameras
                        if (tid < m) {
                            double vv[3];
                            for (int k = 0; k < 3; ++k) {
                                vn[3 * tid + k] = vv[k] = v[3 * tid + k] + (tid > 0 ? da[6 * (tid - 1) + k] : 0.0);
                                tn[3 * tid + k] = t[3 * tid + k] + (tid > 0 ? da[6 * (tid - 1) + 3 + k] : 0.0);
                            }
                            quat_lds(qc + 4 * tid, quat_mult_fast(local_quat(vv), lds_quat(r0 + 4 * tid)));
                        }
                        __syncthreads();
                        // ---- db_i, the trial point, its residuals; ||db||^2, ||e(p + dp)||^2, dL over the points
                        double s3[3] = {0.0, 0.0, 0.0};
                        for (int k = tid; k < n; k += kBaThreads) {
                            double inv[6], ebv[3], wtda[3] = {0.0, 0.0, 0.0}, r[3], Mn[3], e[2];
                            load_inverse(pw, k, cur_inv, inv);
                            for (int j = 1; j < m; ++j) {
                                if (!SEEN(j, k)) continue;
                                const double *dj = da + 6 * (j - 1);
#pragma unroll
                                for (int ii = 0; ii < 3; ++ii) {
                                    double wt = pw(SLOT_W(j) + ii, k) * dj[0];
#pragma unroll
                                    for (int jj = 1; jj < 6; ++jj) wt = wt + pw(SLOT_W(j) + jj * 3 + ii, k) * dj[jj];
                                    wtda[ii] = wtda[ii] + wt;
                                }
                            }
#pragma unroll
                            for (int ii = 0; ii < 3; ++ii) {
                                ebv[ii] = pw(kPEb + ii, k);
                                r[ii] = ebv[ii] - wtda[ii];
                            }
                            point_update(pw, k, cur_m, inv, r, ebv, lm.mu, Mn, s3);
                            for (int j = 0; j < m; ++j) {
                                if (!SEEN(j, k)) continue;
                                const double x[2] = {px[((size_t)j * S + k) * 2], px[((size_t)j * S + k) * 2 + 1]};
                                const double tj[3] = {tn[3 * j], tn[3 * j + 1], tn[3 * j + 2]};
                                residual2(lds_quat(qc + 4 * j), tj, Mn, x, th, e);
                                for (int c = 0; c < 2; ++c) {
                                    pw(SLOT_E(j, cur_e ^ 1) + c, k) = e[c];
                                    s3[1] += e[c] * e[c];
                                }
                            }
                        }
                        block_sum(s3, red);
                        double dp_L2 = 0.0, dL = 0.0;  // the cameras' part
                        for (int k = 0; k < dim; ++k) {
                            dp_L2 += da[k] * da[k];
                            dL += da[k] * (lm.mu * da[k] + ea[k]);
                        }
                        const LmVerdict verdict = lm.verdict(dp_L2, dL, s3, p_L2);
                        if (verdict == kLmLeave) break;
                        if (verdict == kLmAccepted) {
                            __syncthreads();
                            if (tid < 3 * m) v[tid] = vn[tid], t[tid] = tn[tid];
                            __syncthreads();
                            cur_m ^= 1, cur_e ^= 1;
                            accepted = true;
                        }
                    }
                }
                if (accepted || !lm.reject()) break;
            }
            if (!lm.end_step()) break;
        }
        sba_ok = lm.finish(info);
    }
    __syncthreads();

    // ---- the wrapper: every camera's refined pose against its start, the acceptance rule, the write-back
    bool accept = sba_ok && !(info[6] > 5);
    if (tid < 4) red_i[tid] = 0;
    __syncthreads();
    Quat qn{1.0, 0.0, 0.0, 0.0};
    if (accept && tid < m) {
        const double vv[3] = {v[3 * tid], v[3 * tid + 1], v[3 * tid + 2]};
        qn = quat_mult_fast(local_quat(vv), lds_quat(r0 + 4 * tid));
        if (qn.w < 0.0) qn = Quat{qn.w * -1.0, qn.x * -1.0, qn.y * -1.0, qn.z * -1.0};
        double ta[3], tb[3];
        for (int k = 0; k < 3; ++k) ta[k] = pin[4 + 9 * cams_stride + 3 * tid + k], tb[k] = t[3 * tid + k];
        const double na = sqrt(ta[0] * ta[0] + ta[1] * ta[1] + ta[2] * ta[2]), nb = sqrt(tb[0] * tb[0] + tb[1] * tb[1] + tb[2] * tb[2]);
        if (!(nb < 1e-3 && nb > -1e-3) && fabs(nb - 1.0) > 1e-4)
            for (int k = 0; k < 3; ++k) tb[k] = tb[k] / nb;
        if (!(na < 1e-3 && na > -1e-3) && fabs(na - 1.0) > 1e-4)
            for (int k = 0; k < 3; ++k) ta[k] = ta[k] / na;
        double r_diff, t_diff;
        rt_quality(lds_quat(qold + 4 * tid), qn, ta, tb, r_diff, t_diff);
        r_diff = r_diff / M_PI * 180.0;
        if (fabs(r_diff) > angle_thresh || t_diff > t_norm_thresh) red_i[0] = 1;  // (any camera: the same value from every writer)
    }
    __syncthreads();
    accept = accept && red_i[0] == 0;
    if (accept) {
        for (int k = tid; k < n; k += kBaThreads)
            for (int c = 0; c < 3; ++c) Q[(row0 + k) * 3 + c] = pw(kPM + cur_m * 3 + c, k);
        if (tid < m) {
            double Rout[9];
            quat_to_matrix(qn, Rout);
            for (int k = 0; k < 9; ++k) po[12 + 9 * tid + k] = Rout[k];
            for (int k = 0; k < 3; ++k) po[12 + 9 * cams_stride + 3 * tid + k] = t[3 * tid + k];
        }
    }
    if (tid == 0) {
        for (int k = 0; k < 10; ++k) po[k] = info[k];
        po[10] = lm.mu;
        po[11] = accept ? 1.0 : 0.0;
    }
#undef SLOT_E
#undef SLOT_W
#undef SEEN
}

thread_local LastMu g_last_mu_mc;  // mlpl_debug_ba_multicam_last_mu

// One launch for B problems.  R [B][cams_stride][9], t [B][cams_stride][3] (host, in / out), th [B], accepted [B], info [B][10] or NULL.
int mc_run(mlpl_ctx *ctx, const char *who, int B, const double *d_p, const uint8_t *d_vis, int cams_stride, int stride, const int32_t *n_cams,
           const int32_t *counts, double *d_Q, double *R, double *t, const double *th, double angle_thresh, double t_norm_thresh,
           int32_t *accepted, double *info, hipStream_t s) {
    int max_m = 2;
    int rc = ba_check_batch(who, cams_stride >= 1 && d_p && d_vis && d_Q && n_cams && R && t && th && accepted, B, stride, counts, [&](int b) {
        if (n_cams[b] < 0 || n_cams[b] > cams_stride) {
            set_error("%s: n_cams[%d] = %d outside [0, cams_stride = %d]", who, b, n_cams[b], cams_stride);
            return (int)MLPL_E_BAD_INPUT;
        }
        if (n_cams[b] > kMcMaxCams) {
            set_error("%s: n_cams[%d] = %d: at most MLPL_BA_MAX_CAMS = %d cameras are built", who, b, n_cams[b], kMcMaxCams);
            return (int)MLPL_E_UNSUPPORTED;
        }
        max_m = std::max(max_m, (int)n_cams[b]);
        return (int)MLPL_OK;
    });
    if (rc) return rc;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    const size_t n_in = (size_t)mc_in(cams_stride), n_out = (size_t)mc_out(cams_stride);
    const size_t off_in = 0, off_out = off_in + (size_t)B * n_in * 8, off_cams = off_out + (size_t)B * n_out * 8, off_counts = off_cams + (size_t)B * 4,
                 small_bytes = off_counts + (size_t)B * 4;
    void *d_small, *d_ws;
    if ((rc = ws_get(ctx, WS_BA_MULTICAM_IO, small_bytes, &d_small))) return rc;
    if ((rc = ws_get(ctx, WS_BA_MULTICAM, (size_t)B * stride * mc_slots(cams_stride) * 8, &d_ws))) return rc;
    std::vector<char> h(off_out, 0);
    double *hin = (double *)h.data();
    for (int b = 0; b < B; ++b) {
        double *hb = hin + (size_t)b * n_in;
        hb[0] = th[b], hb[1] = angle_thresh, hb[2] = t_norm_thresh;
        std::memcpy(hb + 4, R + (size_t)b * cams_stride * 9, (size_t)n_cams[b] * 72);
        std::memcpy(hb + 4 + 9 * cams_stride, t + (size_t)b * cams_stride * 3, (size_t)n_cams[b] * 24);
    }
    char *sm = (char *)d_small;
    MLPL_HIP_TRY(hipMemcpyAsync(sm + off_in, h.data(), off_out, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(sm + off_cams, n_cams, (size_t)B * 4, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(sm + off_counts, counts, (size_t)B * 4, hipMemcpyHostToDevice, s));
    const size_t lds_bytes = (size_t)mc_lds_doubles(max_m) * 8;
    if (lds_bytes > 48 * 1024)
        MLPL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(bundle_adjust_multicam_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)((size_t)mc_lds_doubles(kMcMaxCams) * 8)));
    prof_mark(ctx, MLPL_PROF_BA_MULTICAM, 0, s);
    hipLaunchKernelGGL(bundle_adjust_multicam_kernel, dim3(B), dim3(kBaThreads), lds_bytes, s, (const double *)(sm + off_in), d_p, d_vis,
                       (const int32_t *)(sm + off_cams), (const int32_t *)(sm + off_counts), cams_stride, stride, d_Q, (double *)d_ws,
                       (double *)(sm + off_out));
    prof_mark(ctx, MLPL_PROF_BA_MULTICAM, 1, s);
    MLPL_HIP_TRY(hipGetLastError());
    std::vector<double> ho((size_t)B * n_out);
    MLPL_HIP_TRY(hipMemcpyAsync(ho.data(), sm + off_out, ho.size() * 8, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    g_last_mu_mc.mu.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        const double *o = ho.data() + (size_t)b * n_out;
        accepted[b] = o[11] != 0.0;
        if (accepted[b]) {  // a refused or failed problem leaves R and t as they came; cameras beyond n_cams[b] are never written
            std::memcpy(R + (size_t)b * cams_stride * 9, o + 12, (size_t)n_cams[b] * 72);
            std::memcpy(t + (size_t)b * cams_stride * 3, o + 12 + 9 * cams_stride, (size_t)n_cams[b] * 24);
        }
        if (info) std::memcpy(info + 10 * b, o, 80);
        g_last_mu_mc.mu[(size_t)b] = o[10];
    }
    return MLPL_OK;
}

// the single entries' camera count: < 2 is bad input, > MLPL_BA_MAX_CAMS is not built; nothing is written either way
int mc_check_cams(const char *who, int m) {
    if (m < 2) {
        set_error("%s: at least two cameras", who);
        return MLPL_E_BAD_INPUT;
    }
    if (m > kMcMaxCams) {
        set_error("%s: %d cameras: at most MLPL_BA_MAX_CAMS = %d are built", who, m, kMcMaxCams);
        return MLPL_E_UNSUPPORTED;
    }
    return MLPL_OK;
}

}  // namespace
}  // namespace mlpl

using namespace mlpl;

extern "C" int mlpl_refine_multicam_ba_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p, const uint8_t *d_vis, int cams_stride,
                                                 int stride, const int32_t *n_cams, const int32_t *counts, double *d_Q, double *R, double *t,
                                                 const double *th, double angle_thresh, double t_norm_thresh, int32_t *accepted, double *info,
                                                 void *stream) try {
    if (!ctx) {
        set_error("mlpl_refine_multicam_ba_batch_dev: ctx is mandatory");
        return MLPL_E_BAD_INPUT;
    }
    return mc_run(ctx, "mlpl_refine_multicam_ba_batch_dev", n_problems, d_p, d_vis, cams_stride, stride, n_cams, counts, d_Q, R, t, th,
                  angle_thresh, t_norm_thresh, accepted, info, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_refine_multicam_ba_batch_dev")

extern "C" int mlpl_refine_multicam_ba_dev(mlpl_ctx *ctx, const double *d_p, const uint8_t *d_vis, int m, int n, double *R, double *t,
                                           double *d_Q, double th, double angle_thresh, double t_norm_thresh, double info[10], void *stream) try {
    if (!ctx || n < 0) {
        set_error("mlpl_refine_multicam_ba_dev: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    if (int rc = mc_check_cams("mlpl_refine_multicam_ba_dev", m)) return rc;
    if (info) std::memset(info, 0, 80);
    if (n == 0) return 0;
    const int32_t count = n, cams = m;
    int32_t acc = 0;
    const int rc = mc_run(ctx, "mlpl_refine_multicam_ba_dev", 1, d_p, d_vis, m, n, &cams, &count, d_Q, R, t, &th, angle_thresh, t_norm_thresh,
                          &acc, info, pick_stream(ctx, stream));
    return rc ? rc : acc;
} MLPL_ENTRY_END("mlpl_refine_multicam_ba_dev")

extern "C" int mlpl_refine_multicam_ba(mlpl_ctx *ctx, const double *p, const uint8_t *vis, int m, int n, double *R, double *t, double *Q,
                                       double th, double angle_thresh, double t_norm_thresh, double info[10]) try {
    if (!ctx || n < 0 || (n > 0 && (!p || !vis || !Q)) || !R || !t) {
        set_error("mlpl_refine_multicam_ba: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    if (int rc = mc_check_cams("mlpl_refine_multicam_ba", m)) return rc;
    if (info) std::memset(info, 0, 80);
    if (n == 0) return 0;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t mn = (size_t)m * n;
    void *dp, *dvis, *dQ;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, mn * 16, &dp))) return rc;
    if ((rc = ws_get(ctx, WS_AUX6, mn, &dvis))) return rc;
    if ((rc = ws_get(ctx, WS_AUX5, (size_t)n * 24, &dQ))) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(dp, p, mn * 16, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(dvis, vis, mn, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(dQ, Q, (size_t)n * 24, hipMemcpyHostToDevice, s));
    const int32_t count = n, cams = m;
    int32_t acc = 0;
    if ((rc = mc_run(ctx, "mlpl_refine_multicam_ba", 1, (const double *)dp, (const uint8_t *)dvis, m, n, &cams, &count, (double *)dQ, R, t, &th,
                     angle_thresh, t_norm_thresh, &acc, info, s)))
        return rc;
    if (acc) MLPL_HIP_TRY(hipMemcpy(Q, dQ, (size_t)n * 24, hipMemcpyDeviceToHost));
    return acc;
} MLPL_ENTRY_END("mlpl_refine_multicam_ba")

extern "C" int mlpl_debug_ba_multicam_last_mu(double *mu, int max_items) { return g_last_mu_mc.get(mu, max_items); }
