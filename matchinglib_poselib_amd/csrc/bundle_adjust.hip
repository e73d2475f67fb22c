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

#include "ba_common.h"
#include "mlpl_internal.h"

namespace mlpl {
namespace {

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
