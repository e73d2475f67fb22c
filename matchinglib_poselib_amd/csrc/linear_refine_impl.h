// linear_refine_impl.h -- poselib::refineEssentialLinear on the MI355X: the iteratively re-weighted linear refit of an essential matrix
// (8-point, Nister or Stewenius on the inliers; Torr, pseudo-Huber or no weights), one workgroup per problem, every step inside ONE launch.
// Included by ransac_5pt.hip inside namespace mlpl, after usac_impl.h: it reuses usac5_row / usac5_weight / usac5_key / usac5_wave_min /
// usac_sampson / dg_bearing (usac_impl.h), refit_solve_body + roots_body (Gram matrix -> Jacobi -> four-vector basis -> 10 x 20
// elimination -> roots, ransac_5pt.hip), jacobi9_wave and null_vector_3x3.
//
// Replaces, under reference poselib/ :
//   source/pose_linear_refinement.cpp:85-309   refineEssentialLinear (the loop)
//   source/pose_linear_refinement.cpp:314-345  findRefinementWeights
//   source/pose_linear_refinement.cpp:347-602  refineModel (PR_8PT, PR_NISTER, PR_STEWENIUS; PR_KNEIP is not built)
//   source/pose_linear_refinement.cpp:608-635  evaluateModelE (getSampsonL2Error on bearing vectors, pose_helper.cpp:3011-3020)
//   source/usac/utils/weightingEssential.cpp:56-148, 210-330   fivept_*_weight, computeTorrWeight, eightpt_weight, solveUsingEigenVectors
//
// linear_refine_kernel<k8pt> (grid = problems, ONE wave per problem; the solver bodies order their LDS traffic with wave_sync()):
//   0. the starting inliers (mask != 0) as an ascending list (ballot compaction); fewer than 6: status FAILED, nothing written.
//   per step j < steps:
//   1. weights of the listed points under the current model and the Gram matrix of the rows f2 (x) f1 scaled by w / ||w|| (the reference's
//      row scaling): every lane accumulates the positions lane, lane + 64, ... in order, then a butterfly reduction -- a fixed order, so
//      a problem's result does not depend on the launch or on the other problems;
//   2. the fit: 8-point = the eigenvector of the smallest eigenvalue of the Gram matrix (jacobi9_wave), F = that vector as rows, E = F
//      without its smallest singular direction (= U diag(s0, s1, 0) V^T); 5-point = refit_solve_body + roots_body<true> on the Gram
//      matrix, then of several real solutions the one with the smallest Sampson-error sum over the list, with the reference's early exit
//      tested at every 4th LIST POSITION (lr_pick);
//   3. evaluation of every point against the step's threshold, stable compaction into the other list;
//   4. acceptance: count >= (1 - max_loss) * current count; else FAILED at j = 0 (nothing written) or stop.
//   A fit without a model (no real solution, fewer than 8 points for the 8-point fit, weights that are all zero, an unsupported solver) stops
//   the loop with the last accepted model.  On success: E, mask = 0/1 of the last accepted list, the count and the accepted steps.

constexpr int kLinRefineMinInliers = 6;

struct LinRefineProb {  // device, one per problem
    double E[9];        // in: starting model; out: the refined one (status 0)
    double th;          // inlier threshold (not squared)
    int32_t n;          // correspondences
    int32_t status;     // out: 0 (reference: true) or MLPL_E_FAILED (reference: false; E and the mask untouched)
    int32_t n_inliers;  // out
    int32_t steps_done; // out: accepted refinement steps
};

struct LinRefineArgs {
    const double *p1, *p2;  // [problems][stride][2]
    int stride;
    LinRefineProb *prob;
    uint8_t *masks;         // [problems][stride], in / out
    int32_t *lists;         // [problems][2][stride] workspace
    double *gram;           // [problems][48] workspace (5-point instance)
    PolyRec *recs;          // [problems]
    double *E_tab;          // [problems][90]
    int32_t *n_models;      // [problems]
    int fit;                // 0 = no solver (reference: "not supported"), 1 = 8-point, 2 = five-point
    int wmode;              // 0 = none, 1 = Torr, 2 = pseudo-Huber
    int steps;
    double th_mult, ph_mult, max_loss;
};

// computeTorrWeight(f, fprime, E) (weightingEssential.cpp:210-227) on the unit bearing vectors f (first image) and fprime (second)
__device__ __forceinline__ double lr_torr_weight(const double *E, double x1, double y1, double x2, double y2) {
    double f[3], fp[3];
    dg_bearing(x1, y1, f);
    dg_bearing(x2, y2, fp);
    const double rxc = E[0] * fp[0] + E[3] * fp[1] + E[6] * fp[2];
    const double ryc = E[1] * fp[0] + E[4] * fp[1] + E[7] * fp[2];
    const double rx = E[0] * f[0] + E[1] * f[1] + E[2] * f[2];
    const double ry = E[3] * f[0] + E[4] * f[1] + E[5] * f[2];
    return 1 / sqrt(rxc * rxc + ryc * ryc + rx * rx + ry * ry);
}

// getSampsonL2Error(E, x1, x2) (pose_helper.cpp:3011-3020) on the unit bearing vectors, Eigen's order of the products
__device__ __forceinline__ double lr_sampson_l2(const double *E, double x1, double y1, double x2, double y2) {
    double f[3], fp[3];
    dg_bearing(x1, y1, f);
    dg_bearing(x2, y2, fp);
    double x2E[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) x2E[c] = fp[0] * E[c] + fp[1] * E[3 + c] + fp[2] * E[6 + c];
    const double r = x2E[0] * f[0] + x2E[1] * f[1] + x2E[2] * f[2];
    const double rx = E[0] * f[0] + E[1] * f[1] + E[2] * f[2];
    const double ry = E[3] * f[0] + E[4] * f[1] + E[5] * f[2];
    return r * r / (x2E[0] * x2E[0] + x2E[1] * x2E[1] + rx * rx + ry * ry);
}

// refineModel's choice among several real five-point solutions (pose_linear_refinement.cpp:437-470 / :513-546): PoseTools::getSampsonError
// on the bearing vectors divided by their third component, summed over the fit list in list order, every 4th LIST POSITION (> 3) the
// test smallest < 0.66 * second smallest ends the loop; then the smallest sum.  The pass structure is usac5_pick's (chunks of 64 list
// entries: errors per (solution, entry) in LDS, running sums per solution lane in order, the exit test per entry lane); the difference is
// that the test is keyed on the position in the list, not on the point index.  Ties of the sums go to the smaller usac5_key.
__device__ __forceinline__ int lr_pick(const double *E, double key, int nm, int lane, const double *__restrict__ p1,
                                       const double *__restrict__ p2, const int32_t *__restrict__ list, int cnt) {
    __shared__ Usac5PickLds L;
    int pos = 0;
    for (int k = 0; k < nm; ++k) {
        const double kk = __shfl(key, k);
        pos += (kk < key || (kk == key && k < lane)) ? 1 : 0;
    }
    if (lane < nm) {
#pragma unroll
        for (int k = 0; k < 9; ++k) L.E[lane][k] = E[k];
    }
    wave_sync();
    double sum = 0;
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int at = i0 + lane, m = min(64, cnt - i0);
        if (at < cnt) {
            const int i = list[at];
            double f[3], fp[3];
            dg_bearing(p1[2 * i], p1[2 * i + 1], f);
            dg_bearing(p2[2 * i], p2[2 * i + 1], fp);
            const double x1 = f[0] / f[2], y1 = f[1] / f[2], x2 = fp[0] / fp[2], y2 = fp[1] / fp[2];
            for (int s = 0; s < nm; ++s) L.err[s][lane] = usac_sampson(L.E[s], x1, y1, x2, y2);
        }
        wave_sync();
        if (lane < nm) {
            double run = sum;
            for (int r = 0; r < m; ++r) {
                run += L.err[lane][r];
                L.err[lane][r] = run;
            }
        }
        wave_sync();
        bool hit = false;
        if (lane < m && at > 3 && at % 4 == 0) {
            double m1 = INFINITY;
            for (int s = 0; s < nm; ++s) m1 = fmin(m1, L.err[s][lane]);
            int first = nm;
            for (int s = nm - 1; s >= 0; --s)
                if (L.err[s][lane] == m1) first = s;
            double m2 = INFINITY;
            for (int s = 0; s < nm; ++s)
                if (s != first) m2 = fmin(m2, L.err[s][lane]);
            hit = m1 < 0.66 * m2;
        }
        const unsigned long long hits = __ballot(hit);
        const int last = hits ? __ffsll((long long)hits) - 1 : m - 1;
        if (lane < nm) sum = L.err[lane][last];
        wave_sync();
        if (hits) break;
    }
    const double v = lane < nm ? sum : INFINITY;
    const double m1 = usac5_wave_min(v);
    int cand = (lane < nm && v == m1) ? pos : 64;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cand = min(cand, __shfl_xor(cand, off));
    const unsigned long long who = __ballot(lane < nm && pos == cand);
    return who ? __ffsll((long long)who) - 1 : 0;
}

// Stable compaction of the points i < n with pred(i) into list (ascending); returns the count (wave-uniform).
template <class Pred>
__device__ __forceinline__ int lr_compact(int n, int lane, int32_t *__restrict__ list, Pred pred) {
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < n && pred(i);
        const unsigned long long bal = __ballot(in);
        if (in) list[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        cnt += __popcll(bal);
    }
    return cnt;
}

template <bool k8pt>  // compile-time: the 8-point instance does not carry the root finder's registers
__global__ __launch_bounds__(64) void linear_refine_kernel(const LinRefineArgs A) {
    __shared__ double sE[9];
    __shared__ Jacobi9Lds J;
    __shared__ double sG[45];
    if (blockDim.x != kSolverThreads) __builtin_trap();  // wave_sync() is a one-wave ordering
    const int b = blockIdx.x, lane = threadIdx.x;
    LinRefineProb &P = A.prob[b];
    const int n = P.n;
    const double th = P.th;
    const double *__restrict__ p1 = A.p1 + (size_t)b * A.stride * 2;
    const double *__restrict__ p2 = A.p2 + (size_t)b * A.stride * 2;
    uint8_t *__restrict__ mask = A.masks + (size_t)b * A.stride;
    int32_t *cur = A.lists + (size_t)b * 2 * A.stride, *nxt = cur + A.stride;

    int cnt = lr_compact(n, lane, cur, [&](int i) { return mask[i] != 0; });
    if (cnt < kLinRefineMinInliers) {
        if (lane == 0) P.status = MLPL_E_FAILED, P.n_inliers = 0, P.steps_done = 0;
        return;
    }
    if (lane < 9) sE[lane] = P.E[lane];
    __syncthreads();  // the list (global) and sE are read by other lanes below
    const double th2 = th * th;
    const double step_size = (A.th_mult * th2 - th2) / A.steps;
    const double ph_th = th * A.ph_mult;
    int steps_done = 0;
    for (int j = 0; j < A.steps; ++j) {
        double E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = sE[k];
        // ---- 1. weights + Gram matrix of the scaled rows ----
        bool fit_ok = A.fit != 0 && (A.fit != 1 || cnt >= 8);
        double wn = 1.0;
        if (fit_ok) {
            if (A.wmode) {
                double w2 = 0;
                for (int at = lane; at < cnt; at += 64) {
                    const int i = cur[at];
                    const double w = A.wmode == 1 ? lr_torr_weight(E, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1])
                                                  : usac5_weight(E, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1], ph_th);
                    w2 += w * w;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) w2 += __shfl_xor(w2, off);
                wn = sqrt(w2);
                fit_ok = wn > 0 && wn <= DBL_MAX;  // all weights zero (a model exact to rounding under pseudo-Huber): 0 / 0 rows, no fit
            }
        }
        if (fit_ok) {
            double acc[45];
#pragma unroll
            for (int t = 0; t < 45; ++t) acc[t] = 0;
            for (int at = lane; at < cnt; at += 64) {
                const int i = cur[at];
                const double x1 = p1[2 * i], y1 = p1[2 * i + 1], x2 = p2[2 * i], y2 = p2[2 * i + 1];
                double q[9];
                usac5_row(x1, y1, x2, y2, q);
                if (A.wmode) {
                    const double w = A.wmode == 1 ? lr_torr_weight(E, x1, y1, x2, y2) : usac5_weight(E, x1, y1, x2, y2, ph_th);
                    const double sc = w / wn;
#pragma unroll
                    for (int k = 0; k < 9; ++k) q[k] *= sc;
                }
                int t = 0;
#pragma unroll
                for (int a = 0; a < 9; ++a)
#pragma unroll
                    for (int c = a; c < 9; ++c) acc[t++] += q[a] * q[c];
            }
#pragma unroll
            for (int t = 0; t < 45; ++t) {
                double v = acc[t];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);  // butterfly: every lane holds the same sum
                acc[t] = v;
            }
            if (lane == 0) {
#pragma unroll
                for (int t = 0; t < 45; ++t) {
                    sG[t] = acc[t];
                    if constexpr (!k8pt) A.gram[(size_t)b * 48 + t] = acc[t];
                }
            }
            __syncthreads();
        }
        // ---- 2. the fit ----
        double En[9];
        if (fit_ok) {
            if constexpr (k8pt) {
                // solveUsingEigenVectors: the eigenvector of the smallest eigenvalue of A^T A
                for (int e = lane; e < 81; e += 64) {
                    const int a = e / 9, c = e - a * 9, lo = a < c ? a : c, hi = a < c ? c : a;
                    J.G[a][c] = sG[lo * 9 - lo * (lo - 1) / 2 + (hi - lo)];
                    J.Vv[a][c] = (a == c) ? 1.0 : 0.0;
                }
                wave_sync();
                jacobi9_wave(J, lane);
                int m = 0;
                for (int a = 1; a < 9; ++a)
                    if (J.G[a][a] < J.G[m][m]) m = a;
                double F[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) F[k] = J.Vv[k][m];  // F(a, c) = f[3 a + c]
                // U diag(s0, s1, 0) V^T = F - (F v) v^T with v the right singular vector of the smallest singular value
                double v[3];
                null_vector_3x3(F, v);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double Fv = F[3 * a] * v[0] + F[3 * a + 1] * v[1] + F[3 * a + 2] * v[2];
#pragma unroll
                    for (int c = 0; c < 3; ++c) En[3 * a + c] = F[3 * a + c] - Fv * v[c];
                }
                bool finite = true;
#pragma unroll
                for (int k = 0; k < 9; ++k) finite = finite && (En[k] == En[k]) && fabs(En[k]) <= DBL_MAX;
                fit_ok = finite;
                wave_sync();
            } else {
                refit_solve_body(A.gram + (size_t)b * 48, 1, A.recs + b, 0, nullptr, 0, 0);
                __syncthreads();  // the record (global) is read by roots_body's lanes
                roots_body<true>(A.recs + b, 0, 1, A.E_tab + (size_t)b * 90, A.n_models + b, nullptr, nullptr, nullptr, nullptr, 0, 0);
                __syncthreads();
                const int nm = A.n_models[b];
                if (nm < 1) {
                    fit_ok = false;
                } else {
                    double Es[9];
                    const int s = lane < nm ? lane : 0;
#pragma unroll
                    for (int k = 0; k < 9; ++k) Es[k] = A.E_tab[(size_t)b * 90 + s * 9 + k];
                    const int take = nm == 1 ? 0 : lr_pick(Es, usac5_key(Es), nm, lane, p1, p2, cur, cnt);
#pragma unroll
                    for (int k = 0; k < 9; ++k) En[k] = A.E_tab[(size_t)b * 90 + take * 9 + k];
                }
            }
        }
        if (!fit_ok) break;  // wave-uniform: the model of the last accepted step stays
        // ---- 3. evaluation against the step's threshold ----
        const double thr = (A.th_mult * th2) - (double)(j + 1) * step_size;
        const int cnt2 = lr_compact(n, lane, nxt, [&](int i) { return lr_sampson_l2(En, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]) < thr; });
        __syncthreads();
        // ---- 4. acceptance ----
        if ((double)cnt2 >= (1.0 - A.max_loss) * (double)cnt) {
            if (lane < 9) sE[lane] = En[lane];
            int32_t *t = cur;
            cur = nxt, nxt = t;
            cnt = cnt2;
            ++steps_done;
            __syncthreads();
        } else if (j == 0) {
            if (lane == 0) P.status = MLPL_E_FAILED, P.n_inliers = 0, P.steps_done = 0;
            return;
        } else {
            break;
        }
    }
    // ---- outputs: E, the 0/1 mask of the last accepted list, the count ----
    for (int i = lane; i < n; i += 64) mask[i] = 0;
    __syncthreads();
    for (int at = lane; at < cnt; at += 64) mask[cur[at]] = 1;
    if (lane < 9) P.E[lane] = sE[lane];
    if (lane == 0) P.status = 0, P.n_inliers = cnt, P.steps_done = steps_done;
}

// Validates the method and fills the solver fields of A: MLPL_OK, MLPL_E_UNSUPPORTED (PR_KNEIP) or MLPL_E_BAD_INPUT (PR_8PT with weight bits
// the reference reads uninitialised weights for).
inline int linear_refine_method(int method, LinRefineArgs &A, const char *who) {
    const int solver = method & 0xF, wbits = method & 0xF0;
    if (method < 0 || method > 0xFF) {
        set_error("%s: refineMethod 0x%x outside one byte", who, method);
        return MLPL_E_BAD_INPUT;
    }
    if (solver == 4) {
        set_error("%s: PR_KNEIP (OpenGV's eigensolver) is not built", who);
        return MLPL_E_UNSUPPORTED;
    }
    if (solver == 1 && wbits != 0x10 && wbits != 0x20 && wbits != 0x30) {
        set_error("%s: PR_8PT needs PR_TORR_WEIGHTS, PR_PSEUDOHUBER_WEIGHTS or PR_NO_WEIGHTS (weight bits 0x%x)", who, wbits);
        return MLPL_E_BAD_INPUT;
    }
    A.fit = solver == 1 ? 1 : ((solver == 2 || solver == 3) ? 2 : 0);
    A.wmode = (A.fit != 0 && wbits == 0x10) ? 1 : ((A.fit != 0 && wbits == 0x20) ? 2 : 0);
    return MLPL_OK;
}

// The batch on the device.  E: host, 9 per problem (in / out); th: host, one per problem; counts: host.  n_inliers / status / steps_done: host
// (steps_done optional).  d_masks: [n_problems][stride] on the device (in / out).
inline int linear_refine_batch(mlpl_ctx *ctx, int B, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, const double *th,
                               int method, int steps, double th_mult, double ph_mult, double max_loss, double *E, uint8_t *d_masks,
                               int32_t *n_inliers, int32_t *status, int32_t *steps_done, hipStream_t s, const char *who) {
    LinRefineArgs A{};
    int rc;
    if ((rc = linear_refine_method(method, A, who))) return rc;
    if (B < 1 || stride < 1 || !d_p1 || !d_p2 || !counts || !th || !E || !d_masks || !n_inliers || !status || steps < 0 ||
        !std::isfinite(th_mult) || !std::isfinite(ph_mult) || !std::isfinite(max_loss)) {
        set_error("%s: bad arguments", who);
        return MLPL_E_BAD_INPUT;
    }
    if (!counts_in_range(who, B, counts, 0, stride)) return MLPL_E_BAD_INPUT;
    for (int b = 0; b < B; ++b)
        if (!(th[b] > 0) || !std::isfinite(th[b])) {
            set_error("%s: th[%d] must be positive and finite", who, b);
            return MLPL_E_BAD_INPUT;
        }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    void *d_prob, *d_lists, *d_work;
    const size_t prob_bytes = (size_t)B * sizeof(LinRefineProb);
    const size_t gram_off = 0, recs_off = (size_t)B * 48 * 8, etab_off = recs_off + (size_t)B * sizeof(PolyRec),
                 nm_off = etab_off + (size_t)B * 90 * 8, work_bytes = nm_off + (size_t)B * 4;
    if ((rc = ws_get(ctx, WS_AUX2, prob_bytes, &d_prob))) return rc;
    if ((rc = ws_get(ctx, WS_AUX3, (size_t)B * 2 * stride * 4, &d_lists))) return rc;
    if ((rc = ws_get(ctx, WS_AUX4, work_bytes, &d_work))) return rc;
    std::vector<LinRefineProb> h((size_t)B);
    for (int b = 0; b < B; ++b) {
        std::memcpy(h[b].E, E + (size_t)b * 9, 72);
        h[b].th = th[b], h[b].n = counts[b], h[b].status = MLPL_E_INTERNAL, h[b].n_inliers = 0, h[b].steps_done = 0;
    }
    MLPL_HIP_TRY(hipMemcpyAsync(d_prob, h.data(), prob_bytes, hipMemcpyHostToDevice, s));
    A.p1 = d_p1, A.p2 = d_p2, A.stride = stride, A.prob = (LinRefineProb *)d_prob, A.masks = d_masks, A.lists = (int32_t *)d_lists;
    char *w = (char *)d_work;
    A.gram = (double *)(w + gram_off), A.recs = (PolyRec *)(w + recs_off), A.E_tab = (double *)(w + etab_off), A.n_models = (int32_t *)(w + nm_off);
    A.steps = steps, A.th_mult = th_mult, A.ph_mult = ph_mult, A.max_loss = max_loss;
    if (A.fit == 2) hipLaunchKernelGGL(linear_refine_kernel<false>, dim3(B), dim3(kSolverThreads), 0, s, A);
    else hipLaunchKernelGGL(linear_refine_kernel<true>, dim3(B), dim3(kSolverThreads), 0, s, A);
    MLPL_HIP_TRY(hipGetLastError());
    MLPL_HIP_TRY(hipMemcpyAsync(h.data(), d_prob, prob_bytes, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        if (h[b].status == MLPL_E_INTERNAL) {
            set_error("%s: problem %d was not processed", who, b);
            return MLPL_E_INTERNAL;
        }
        status[b] = h[b].status;
        n_inliers[b] = h[b].status == 0 ? h[b].n_inliers : 0;
        if (steps_done) steps_done[b] = h[b].status == 0 ? h[b].steps_done : 0;
        if (h[b].status == 0) std::memcpy(E + (size_t)b * 9, h[b].E, 72);
    }
    return MLPL_OK;
}

// The cheirality step of a batch (launch_recover_pose_batch) behind a public interface: E host, 9 per problem; d_masks NULL (all points) or
// [n_problems][stride] on the device (in / out, as mlpl_recover_pose_dev's mask).
inline int recover_pose_batch(mlpl_ctx *ctx, int B, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, const double *E,
                              double dist, uint8_t *d_masks, int32_t *n_good, double *R, double *t, hipStream_t s) {
    static const char *who = "mlpl_recover_pose_batch_dev";
    if (B < 1 || stride < 1 || !d_p1 || !d_p2 || !counts || !E || !n_good || !R || !t) {
        set_error("%s: bad arguments", who);
        return MLPL_E_BAD_INPUT;
    }
    if (!counts_in_range(who, B, counts, 0, stride)) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    int rc;
    void *d_small, *d_cmask, *d_ones = nullptr;
    const size_t off_E = 0, off_P = off_E + (size_t)B * 72, off_counts = off_P + (size_t)B * 69 * 8, off_active = off_counts + (size_t)B * 4,
                 off_cc = off_active + (size_t)B * 4, off_pose = (off_cc + (size_t)B * 16 + 15) / 16 * 16, small_bytes = off_pose + (size_t)B * sizeof(PairPoseDev);
    if ((rc = ws_get(ctx, WS_AUX2, small_bytes, &d_small))) return rc;
    if ((rc = ws_get(ctx, WS_AUX3, (size_t)B * 4 * stride, &d_cmask))) return rc;
    if (!d_masks) {
        if ((rc = ws_get(ctx, WS_AUX4, (size_t)B * stride, &d_ones))) return rc;
        MLPL_HIP_TRY(hipMemsetAsync(d_ones, 1, (size_t)B * stride, s));
    }
    char *sm = (char *)d_small;
    std::vector<int32_t> active((size_t)B, 1);
    MLPL_HIP_TRY(hipMemcpyAsync(sm + off_E, E, (size_t)B * 72, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(sm + off_counts, counts, (size_t)B * 4, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(sm + off_active, active.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    if ((rc = launch_recover_pose_batch(sm + off_E, 72, d_p1, d_p2, (const int32_t *)(sm + off_counts), (const int32_t *)(sm + off_active), B, stride, dist,
                                        d_masks ? d_masks : (uint8_t *)d_ones, (double *)(sm + off_P), (uint8_t *)d_cmask, (int32_t *)(sm + off_cc),
                                        (PairPoseDev *)(sm + off_pose), s)))
        return rc;
    std::vector<PairPoseDev> pose((size_t)B);
    MLPL_HIP_TRY(hipMemcpyAsync(pose.data(), sm + off_pose, (size_t)B * sizeof(PairPoseDev), hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        n_good[b] = pose[b].n_good;
        std::memcpy(R + (size_t)b * 9, pose[b].R, 72);
        std::memcpy(t + (size_t)b * 3, pose[b].t, 24);
    }
    return MLPL_OK;
}
