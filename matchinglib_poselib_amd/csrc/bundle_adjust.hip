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
// eb_i, (V*_i)^-1 twice (a damping attempt reads the previous attempt's inverse).  The blocks are kept and not recomputed per pass: the simpler
// of the two options; recomputing them has not been measured.
//
// ba_common.h holds what this kernel shares with bundle_adjust_multicam.hip: the geometry, the reductions, and the Levenberg-Marquardt core
// (the slots up to kPCam, the damped inverse, the first_bad repair, the point update, the optimiser's state and every stop).
#include <climits>
#include <cstring>

#include "ba_common.h"
#include "mlpl_internal.h"

namespace mlpl {
namespace {

// this kernel's slots of the per-point state, behind the shared ones
constexpr int kSE = kPCam;    // 2 x 4: the residual (frame 0 x, y, frame 1 x, y), current / trial
constexpr int kSW = kSE + 8;  // 18: W_i, 6 x 3 row-major
constexpr int kBaSlots = kSW + 18;
static_assert(kBaSlots == 53, "WS_BA is sized by it");
constexpr int kBaIn = 16;   // per problem: R 9, t 3, th, angle_thresh, t_norm_thresh
constexpr int kBaOut = 24;  // per problem: R 9, t 3, info 10, mu, accepted

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
    const PointWs pw{ws_all + row0 * kBaSlots, (size_t)stride};

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
    LmState lm;
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
        const double zero3[3] = {0.0, 0.0, 0.0};
        const Quat q_unit{1.0, 0.0, 0.0, 0.0};
        const Quat q_id = quat_mult_fast(local_quat(zero3), q_unit);
        CamJ cam0;
        cam_setup(q_unit, zero3, zero3, false, cam0);

        // the points into the workspace, the residual at the start
        int cur_e = 0;
        {
            const Quat q1 = quat_mult_fast(local_quat(v), r0);
            double acc[1] = {0.0};
            for (int k = tid; k < n; k += kBaThreads) {
                const size_t at = row0 + idx[k];
                double M[3], e[4];
                for (int c = 0; c < 3; ++c) pw(kPM + c, k) = M[c] = Q[at * 3 + c];
                const double x1[2] = {p1[at * 2], p1[at * 2 + 1]}, x2[2] = {p2[at * 2], p2[at * 2 + 1]};
                residual2(q_id, zero3, M, x1, th, e);
                residual2(q1, t, M, x2, th, e + 2);
                for (int c = 0; c < 4; ++c) {
                    pw(kSE + c, k) = e[c];
                    acc[0] += e[c] * e[c];
                }
            }
            block_sum(acc, red);
            lm.start(acc[0]);
        }

        for (; lm.itno < kBaMaxIter && !lm.stop; ++lm.itno) {
            // ---- Jacobian blocks, V_i, W_i, eb_i; U, ea, ||J^T e||_inf, ||p||^2, the largest diagonal entry
            CamJ cam1;
            cam_setup(r0, v, t, true, cam1);
            ++lm.njev;
            double sums[28];  // U upper 21, ea 6, ||points||^2
#pragma unroll
            for (int k = 0; k < 28; ++k) sums[k] = 0.0;
            double mx_e = 0.0, mx_d = DBL_MIN;
            for (int k = tid; k < n; k += kBaThreads) {
                double M[3], e[4], A[2][6], B0[2][3], B1[2][3];
                for (int c = 0; c < 3; ++c) M[c] = pw(kPM + cur_m * 3 + c, k);
                for (int c = 0; c < 4; ++c) e[c] = pw(kSE + cur_e * 4 + c, k);
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
                            pw(kPVd + ii, k) = val;
                            if (val > mx_d) mx_d = val;
                        } else {
                            pw(kPVu + ii + jj - 1, k) = val;
                        }
                    }
                    const double ebv = (B0[0][ii] * e[0] + B0[1][ii] * e[1]) + (B1[0][ii] * e[2] + B1[1][ii] * e[3]);
                    pw(kPEb + ii, k) = ebv;
                    mx_e = fmax(mx_e, fabs(ebv));
                }
#pragma unroll
                for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                    for (int jj = 0; jj < 3; ++jj) pw(kSW + ii * 3 + jj, k) = A[0][ii] * B1[0][jj] + A[1][ii] * B1[1][jj];
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
            double p_L2 = 0.0;
            for (int k = 0; k < 3; ++k) p_L2 += v[k] * v[k];
            for (int k = 0; k < 3; ++k) p_L2 += t[k] * t[k];
            p_L2 += sums[27];
            if (!lm.after_gradient(mx_e, mx_d)) break;

            // ---- the damping loop
            bool vd_from_inv = false;  // V_i's diagonal currently lives in the previous attempt's inverse
            int cur_inv = 0;
            while (true) {
                for (int i = 0; i < 6; ++i) U[i][i] += lm.mu;
                double acc[27];  // sum Y W^T upper 21, sum Y eb 6
#pragma unroll
                for (int k = 0; k < 27; ++k) acc[k] = 0.0;
                int first_bad = INT_MAX;
                for (int k = tid; k < n; k += kBaThreads) {
                    double inv[6], W[6][3], ebv[3];
                    if (!damped_inverse(pw, k, vd_from_inv, cur_inv, lm.mu, inv)) {
                        if (k < first_bad) first_bad = k;
                        continue;
                    }
#pragma unroll
                    for (int ii = 0; ii < 6; ++ii)
#pragma unroll
                        for (int jj = 0; jj < 3; ++jj) W[ii][jj] = pw(kSW + ii * 3 + jj, k);
                    for (int c = 0; c < 3; ++c) ebv[c] = pw(kPEb + c, k);
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
                    repair_first_bad(pw, n, first_bad, vd_from_inv, cur_inv, lm.mu);
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
                    ++lm.nlss;
                    if (solved) {
                        // ---- db_i, the trial point, its residual; ||dp||^2, ||e(p + dp)||^2, dL
                        double vn[3], tn[3];
                        for (int k = 0; k < 3; ++k) vn[k] = v[k] + da[k], tn[k] = t[k] + da[3 + k];
                        const Quat q1 = quat_mult_fast(local_quat(vn), r0);
                        double s3[3] = {0.0, 0.0, 0.0};  // ||db||^2, ||e_new||^2, dL over the points
                        for (int k = tid; k < n; k += kBaThreads) {
                            double inv[6], ebv[3], r[3], Mn[3], e[4];
                            load_inverse(pw, k, cur_inv, inv);
#pragma unroll
                            for (int ii = 0; ii < 3; ++ii) {
                                ebv[ii] = pw(kPEb + ii, k);
                                double wt = pw(kSW + ii, k) * da[0];
#pragma unroll
                                for (int jj = 1; jj < 6; ++jj) wt = wt + pw(kSW + jj * 3 + ii, k) * da[jj];
                                r[ii] = ebv[ii] - wt;
                            }
                            point_update(pw, k, cur_m, inv, r, ebv, lm.mu, Mn, s3);
                            const size_t at = row0 + idx[k];
                            const double x1[2] = {p1[at * 2], p1[at * 2 + 1]}, x2[2] = {p2[at * 2], p2[at * 2 + 1]};
                            residual2(q_id, zero3, Mn, x1, th, e);
                            residual2(q1, tn, Mn, x2, th, e + 2);
                            for (int c = 0; c < 4; ++c) {
                                pw(kSE + (cur_e ^ 1) * 4 + c, k) = e[c];
                                s3[1] += e[c] * e[c];
                            }
                        }
                        block_sum(s3, red);
                        double dp_L2 = 0.0, dL = 0.0;  // the camera's part
                        for (int k = 0; k < 6; ++k) {
                            dp_L2 += da[k] * da[k];
                            dL += da[k] * (lm.mu * da[k] + ea[k]);
                        }
                        const LmVerdict verdict = lm.verdict(dp_L2, dL, s3, p_L2);
                        if (verdict == kLmLeave) break;
                        if (verdict == kLmAccepted) {
                            for (int k = 0; k < 3; ++k) v[k] = vn[k], t[k] = tn[k];
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
            for (int c = 0; c < 3; ++c) Q[at * 3 + c] = pw(kPM + cur_m * 3 + c, k);
        }
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) po[k] = Rout[k];
        for (int k = 0; k < 3; ++k) po[9 + k] = tout[k];
        for (int k = 0; k < 10; ++k) po[12 + k] = info[k];
        po[22] = lm.mu;
        po[23] = accept ? 1.0 : 0.0;
    }
}

thread_local LastMu g_last_mu;  // mlpl_debug_ba_last_mu

// One launch for B problems.  R, t (host, in / out), th [B], accepted [B], info [B][10] or NULL.
int ba_run(mlpl_ctx *ctx, const char *who, int B, const double *d_p1, const double *d_p2, int stride, const int32_t *counts,
           const uint8_t *d_masks, double *d_Q, double *R, double *t, const double *th, double angle_thresh, double t_norm_thresh,
           int32_t *accepted, double *info, hipStream_t s) {
    int rc = ba_check_batch(who, d_p1 && d_p2 && d_Q && R && t && th && accepted, B, stride, counts, [](int) { return (int)MLPL_OK; });
    if (rc) return rc;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    const size_t off_in = 0, off_out = off_in + (size_t)B * kBaIn * 8, off_counts = off_out + (size_t)B * kBaOut * 8,
                 small_bytes = off_counts + (size_t)B * 4;
    const size_t rows = (size_t)B * stride, off_idx = rows * kBaSlots * 8;
    void *d_small, *d_ws;
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
    g_last_mu.mu.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        const double *o = ho.data() + (size_t)b * kBaOut;
        accepted[b] = o[23] != 0.0;
        if (accepted[b]) {  // a refused or failed problem leaves R and t as they came
            std::memcpy(R + 9 * b, o, 72);
            std::memcpy(t + 3 * b, o + 9, 24);
        }
        if (info) std::memcpy(info + 10 * b, o + 12, 80);
        g_last_mu.mu[(size_t)b] = o[22];
    }
    return MLPL_OK;
}

}  // namespace
}  // namespace mlpl

using namespace mlpl;

extern "C" int mlpl_refine_stereo_ba_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride,
                                               const int32_t *counts, const uint8_t *d_masks, double *d_Q, double *R, double *t,
                                               const double *th, double angle_thresh, double t_norm_thresh, int32_t *accepted, double *info,
                                               void *stream) try {
    if (!ctx) {
        set_error("mlpl_refine_stereo_ba_batch_dev: ctx is mandatory");
        return MLPL_E_BAD_INPUT;
    }
    return ba_run(ctx, "mlpl_refine_stereo_ba_batch_dev", n_problems, d_p1, d_p2, stride, counts, d_masks, d_Q, R, t, th, angle_thresh,
                  t_norm_thresh, accepted, info, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_refine_stereo_ba_batch_dev")

extern "C" int mlpl_refine_stereo_ba_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const uint8_t *d_mask, double R[9],
                                         double t[3], double *d_Q, double th, double angle_thresh, double t_norm_thresh, double info[10],
                                         void *stream) try {
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
} MLPL_ENTRY_END("mlpl_refine_stereo_ba_dev")

extern "C" int mlpl_refine_stereo_ba(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const uint8_t *mask, double R[9], double t[3],
                                     double *Q, double th, double angle_thresh, double t_norm_thresh, double info[10]) try {
    if (!ctx || n < 0 || (n > 0 && (!p1 || !p2 || !Q)) || !R || !t) {
        set_error("mlpl_refine_stereo_ba: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    if (info) std::memset(info, 0, 80);
    if (n == 0) return 0;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const double *dp1, *dp2;
    void *dQ, *dmask = nullptr;
    int rc;
    if ((rc = upload_points(ctx, p1, p2, n, &dp1, &dp2))) return rc;
    if ((rc = ws_get(ctx, WS_AUX5, (size_t)n * 24, &dQ))) return rc;
    if (mask && (rc = ws_get(ctx, WS_AUX6, (size_t)n, &dmask))) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(dQ, Q, (size_t)n * 24, hipMemcpyHostToDevice, s));
    if (mask) MLPL_HIP_TRY(hipMemcpyAsync(dmask, mask, (size_t)n, hipMemcpyHostToDevice, s));
    const int32_t count = n;
    int32_t acc = 0;
    if ((rc = ba_run(ctx, "mlpl_refine_stereo_ba", 1, dp1, dp2, n, &count, (const uint8_t *)dmask, (double *)dQ, R, t, &th, angle_thresh,
                     t_norm_thresh, &acc, info, s)))
        return rc;
    if (acc) MLPL_HIP_TRY(hipMemcpy(Q, dQ, (size_t)n * 24, hipMemcpyDeviceToHost));
    return acc;
} MLPL_ENTRY_END("mlpl_refine_stereo_ba")

extern "C" int mlpl_debug_ba_last_mu(double *mu, int max_items) { return g_last_mu.get(mu, max_items); }
