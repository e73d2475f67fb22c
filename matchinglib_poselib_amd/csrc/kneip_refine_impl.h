// kneip_refine_impl.h -- the PR_KNEIP solver of poselib::refineEssentialLinear on the MI355X: OpenGV's eigensolver (Kneip & Lynen) on the
// current inliers, which returns R and t directly.  Included by ransac_5pt.hip inside namespace mlpl, after linear_refine_impl.h: it reuses
// lr_compact, lr_sampson_l2, linear_refine_batch (the other three solvers), dg_bearing and GlibcRand.
//
// Replaces, under reference poselib/ :
//   source/pose_linear_refinement.cpp:85-309    refineEssentialLinear: the loop with PR_KNEIP, the retry loop at step 0 (:194-239), the
//                                               output rule for R and t (:272-293)
//   source/pose_linear_refinement.cpp:535-590   refineModel, PR_KNEIP
//   source/usac/utils/PoseFunctions.cpp:30-41   getPerturbedRotation
//   source/pose_helper.cpp:2947-2954            isMatRoationMat
//   thirdparty/opengv/src/relative_pose/methods.cpp:496-549   eigensolver: the summation terms (device) and the sign of the translation
//
// Division of the work.  Per step and problem the device accumulates the summation terms over the inlier list (kneip_sums_kernel), the host
// runs dgm::eigensolver_sums on them (usac_degen_math.h: Levenberg-Marquardt on the eigenvalue gradient, a few dozen evaluations of 3 x 3
// algebra; a per-lane device build of that header measured 5-10 ms, docs/DESIGN_HISTORY.md section 8), and the device evaluates the
// resulting model(s) against every correspondence (kneip_eval_kernel).  A batch moves in lockstep over the steps; its problems are solved by
// a few host threads, as USAC's upgrade candidates are.
//
// The sums are the bits dgm::eig_sums produces on the same list: the solver differentiates a gradient carrying 1e-15 of noise by forward
// differences, so its path follows rounding.  Hence one lane per accumulator, adding the list's terms in list order; this file is compiled
// with contraction off like the host (Makefile), sqrt and divide of doubles are IEEE on the device.
//
// Stated deviation: with weight bits other than PR_TORR_WEIGHTS / PR_PSEUDOHUBER_WEIGHTS the reference hands OpenGV its whole `inliers`
// vector, which until the first accepted step is as long as the point set and zero-padded: the sums then hold n - count extra copies of
// correspondence 0.  Here every method byte sums the list itself -- what 0x14 / 0x24 (the harness default, 52) do in the reference.

constexpr int kKneipAttempts = 12;  // MAX_SOLS_KNEIP

struct KneipProb {       // device, one per problem; rewritten by the host before every launch
    double thr_gate;     // eval: th^2, the threshold of the retry loop's own acceptance test
    double thr;          // eval: the step's threshold
    int32_t n;           // correspondences
    int32_t cnt;         // length of the current list (sums, act 1: out)
    int32_t side;        // which half of lists[b] holds the current list
    int32_t act;         // sums: 0 skip, 1 build the list from the mask, then sum, 2 sum the current list
                         // eval: 0 skip, 1 evaluate, 2 write the 0/1 mask of the current list, 3 count the mask and make it 0/1 (no step ran)
    int32_t K;           // eval: candidate models
    uint32_t valid;      // eval: bit a = candidate a is a model
    int32_t gate;        // eval: 1 = retry loop: the first valid candidate with count(thr_gate) >= (1 - max_loss) cnt is taken
    int32_t chosen;      // eval out: the candidate taken, -1 none
    int32_t cnt2;        // eval out: its count under thr (the list is in the other half)
    int32_t accepted;    // eval out: cnt2 >= (1 - max_loss) cnt
};

struct KneipArgs {
    const double *p1, *p2;  // [problems][stride][2]
    int stride;
    KneipProb *prob;
    uint8_t *masks;         // [problems][stride]
    int32_t *lists;         // [problems][2][stride]
    double *sums;           // [problems][88]: EigSums (81), then the first list entry's bearing vectors f1, f2
    const double *E;        // [problems][e_stride]: the candidates, 9 each
    int e_stride;
    double max_loss;
};

constexpr int kKneipSumsStride = 88;

__device__ __forceinline__ int kneip_tri(int a, int b) {  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -> 0..5
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo * 3 - lo * (lo - 1) / 2 + (hi - lo);
}

// grid = problems, one wave per problem.  Lane 6 p + q < 36 owns the sum of (f1 f1^T)_p (f2 f2^T)_q, p and q over the six distinct entries
// of a symmetric 3 x 3 matrix; the list goes through LDS in chunks of 64 entries (lane = entry: bearing vectors and their twelve products),
// then every owner adds the chunk's terms in order.  f1 = the adapter's first view = the bearing vector of the SECOND image.
__global__ __launch_bounds__(64) void kneip_sums_kernel(const KneipArgs A) {
    __shared__ double sW[6][65], sF[6][65], sS[36];  // 65: the six rows an owner group reads lie in different banks
    if (blockDim.x != kSolverThreads) __builtin_trap();
    const int b = blockIdx.x, lane = threadIdx.x;
    KneipProb &P = A.prob[b];
    if (P.act == 0) return;
    const int n = min(P.n, A.stride);
    const double *__restrict__ p1 = A.p1 + (size_t)b * A.stride * 2;
    const double *__restrict__ p2 = A.p2 + (size_t)b * A.stride * 2;
    const uint8_t *__restrict__ mask = A.masks + (size_t)b * A.stride;
    int32_t *cur = A.lists + ((size_t)b * 2 + (P.side & 1)) * A.stride;
    double *__restrict__ out = A.sums + (size_t)b * kKneipSumsStride;
    int cnt;
    if (P.act == 1) {
        cnt = lr_compact(n, lane, cur, [&](int i) { return mask[i] != 0; });
        if (lane == 0) P.cnt = cnt;
        if (cnt < kLinRefineMinInliers) return;
        __syncthreads();  // the list (global) is read by other lanes below
    } else {
        cnt = max(0, min(P.cnt, n));
    }
    const int pw = lane / 6, pf = lane - 6 * pw;
    double acc = 0;
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int at = i0 + lane, m = min(64, cnt - i0);
        if (at < cnt) {
            const int i = cur[at];
            double f1[3], f2[3];
            dg_bearing(p2[2 * i], p2[2 * i + 1], f1);
            dg_bearing(p1[2 * i], p1[2 * i + 1], f2);
            sW[0][lane] = f1[0] * f1[0], sW[1][lane] = f1[0] * f1[1], sW[2][lane] = f1[0] * f1[2];
            sW[3][lane] = f1[1] * f1[1], sW[4][lane] = f1[1] * f1[2], sW[5][lane] = f1[2] * f1[2];
            sF[0][lane] = f2[0] * f2[0], sF[1][lane] = f2[0] * f2[1], sF[2][lane] = f2[0] * f2[2];
            sF[3][lane] = f2[1] * f2[1], sF[4][lane] = f2[1] * f2[2], sF[5][lane] = f2[2] * f2[2];
            if (at == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out[81 + k] = f1[k], out[84 + k] = f2[k];
            }
        }
        wave_sync();
        if (lane < 36) {
            for (int r = 0; r < m; ++r) acc += sW[pw][r] * sF[pf][r];
        }
        wave_sync();
    }
    if (lane < 36) sS[lane] = acc;
    wave_sync();
    for (int e = lane; e < 81; e += 64) {  // EigSums::G[b][e][3 r + c]
        const int k = e % 9;
        out[e] = sS[kneip_tri(e / 27, (e / 9) % 3) * 6 + kneip_tri(k / 3, k % 3)];
    }
}

// grid = problems, one wave per problem.  Every list index is below n <= stride and every list position below cnt <= n.
__global__ __launch_bounds__(64) void kneip_eval_kernel(const KneipArgs A) {
    if (blockDim.x != kSolverThreads) __builtin_trap();
    const int b = blockIdx.x, lane = threadIdx.x;
    KneipProb &P = A.prob[b];
    const int act = P.act;
    if (act == 0) return;
    const int n = min(P.n, A.stride);
    const double *__restrict__ p1 = A.p1 + (size_t)b * A.stride * 2;
    const double *__restrict__ p2 = A.p2 + (size_t)b * A.stride * 2;
    uint8_t *__restrict__ mask = A.masks + (size_t)b * A.stride;
    const int side = P.side & 1;
    const int32_t *cur = A.lists + ((size_t)b * 2 + side) * A.stride;
    int32_t *nxt = A.lists + ((size_t)b * 2 + (side ^ 1)) * A.stride;
    const int cnt = max(0, min(P.cnt, n));
    if (act == 2) {
        for (int i = lane; i < n; i += 64) mask[i] = 0;
        __syncthreads();
        for (int at = lane; at < cnt; at += 64) mask[cur[at]] = 1;
        return;
    }
    if (act == 3) {
        int c = 0;
        for (int i0 = 0; i0 < n; i0 += 64) c += __popcll(__ballot(i0 + lane < n && mask[i0 + lane] != 0));
        if (lane == 0) P.cnt = c;
        if (c >= kLinRefineMinInliers)
            for (int i = lane; i < n; i += 64) mask[i] = mask[i] != 0 ? 1 : 0;
        return;
    }
    const double *__restrict__ Ec = A.E + (size_t)b * A.e_stride;
    const int K = max(0, min(P.K, min(kKneipAttempts, A.e_stride / 9)));
    const uint32_t valid = P.valid;
    const double need = (1.0 - A.max_loss) * (double)cnt;
    int chosen = -1;
    if (P.gate) {
        const double thr_gate = P.thr_gate;
        for (int a = 0; a < K && chosen < 0; ++a) {
            if (!((valid >> a) & 1u)) continue;
            double E[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) E[k] = Ec[a * 9 + k];
            int c = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                c += __popcll(__ballot(i < n && lr_sampson_l2(E, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]) < thr_gate));
            }
            if ((double)c >= need) chosen = a;
        }
    } else if (K > 0 && (valid & 1u)) {
        chosen = 0;
    }
    int cnt2 = 0, accepted = 0;
    if (chosen >= 0) {
        double E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = Ec[chosen * 9 + k];
        const double thr = P.thr;
        cnt2 = lr_compact(n, lane, nxt, [&](int i) { return lr_sampson_l2(E, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]) < thr; });
        accepted = (double)cnt2 >= need ? 1 : 0;
    }
    if (lane == 0) P.chosen = chosen, P.cnt2 = cnt2, P.accepted = accepted;
}

// poselib::isMatRoationMat: R^T R - I within 1e-3 in every entry, det R - 1 within 1e-3 (a NaN fails both)
inline bool kneip_is_rotation(const double *R) {
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
            const double v = (R[a] * R[c] + R[3 + a] * R[3 + c] + R[6 + a] * R[6 + c]) - (a == c ? 1.0 : 0.0);
            if (!(std::fabs(v) <= 1e-3)) return false;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    const double d = det - 1.0;
    return d < 1e-3 && d > -1e-3;
}

// getPerturbedRotation(identity, 0.1) from three raw rand() values: the Cayley parameters of the identity are zero
inline void kneip_perturbed_identity(const int32_t *raw, double *R) {
    double c[3], Rr[9];
    for (int k = 0; k < 3; ++k) c[k] = 0.0 + (((double)raw[k]) / ((double)2147483647) - 0.5) * 2.0 * 0.1;
    dgm::cayley_reduced(c, Rr);
    const double scale = 1 + c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    for (int k = 0; k < 9; ++k) R[k] = (1 / scale) * Rr[k];
}

// refineModel, PR_KNEIP (pose_linear_refinement.cpp:535-590) from the sums: false = the step is rejected.  t has unit length.
inline bool kneip_solve(const double *sums, const double *R_start, double *R, double *t, double *E) {
    dgm::EigSums Sx;
    std::memcpy(&Sx, sums, sizeof(Sx));
    double tt[3];
    dgm::eigensolver_sums(Sx, sums + 81, sums + 84, R_start, R, tt);
    const double inv = 1.0 / std::sqrt(tt[0] * tt[0] + (tt[1] * tt[1] + tt[2] * tt[2]));  // Eigen: t /= t.norm() multiplies by the reciprocal
    for (int k = 0; k < 3; ++k) t[k] = tt[k] * inv;
    for (int k = 0; k < 9; ++k)
        if (R[k] != R[k]) return false;
    if (!kneip_is_rotation(R)) return false;
    if (std::fabs(t[0]) <= 1e-3 && std::fabs(t[1]) <= 1e-3 && std::fabs(t[2]) <= 1e-3) return false;  // t.isZero(1e-3)
    if (!(t[0] == t[0] && t[1] == t[1] && t[2] == t[2])) return false;  // a NaN translation: the reference would go on with a NaN model
    dgm::e_from_rt(R, t, E);
    return true;
}

// fn(i) for i < items on a few host threads (the policy of USAC's upgrade candidates: at most 8, at least 16 items each)
template <class Fn>
inline void kneip_parallel(size_t items, Fn fn) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t workers = std::min<size_t>(std::min<size_t>(hw ? hw : 1, 8), items / 16);
    auto slice = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) fn(i);
    };
    if (workers >= 2) {
        std::vector<std::thread> pool;
        for (size_t w = 1; w < workers; ++w) pool.emplace_back(slice, items * w / workers, items * (w + 1) / workers);
        slice(0, items / workers);
        for (auto &th : pool) th.join();
    } else {
        slice(0, items);
    }
}

struct KneipTimes {  // optional, seconds: where a call's time goes (tools/linear_refine_timing.py)
    double sums, solve, eval, hops;
};

// The batch.  Arguments as linear_refine_batch; R [B][9] in / out, t [B][3] out, rt_valid [B] in (R holds a start rotation) / out (R and t
// were written), seeds [B] or NULL (1), attempts_used [B] or NULL.
inline int kneip_refine_batch(mlpl_ctx *ctx, int B, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, const double *th,
                              int method, int steps, double th_mult, double ph_mult, double max_loss, double *E, uint8_t *d_masks, int32_t *n_inliers,
                              int32_t *status, int32_t *steps_done, double *R, double *t, int32_t *rt_valid, const uint32_t *seeds,
                              int32_t *attempts_used, hipStream_t s, const char *who, KneipTimes *times) {
    if (method < 0 || method > 0xFF) {
        set_error("%s: refineMethod 0x%x outside one byte", who, method);
        return MLPL_E_BAD_INPUT;
    }
    if (!R || !t || !rt_valid) {
        set_error("%s: R, t and rt_valid are mandatory", who);
        return MLPL_E_BAD_INPUT;
    }
    if ((method & 0xF) != 4) {  // the other solvers know no rotation: R and t stay, rt_valid is cleared
        const int rc = linear_refine_batch(ctx, B, d_p1, d_p2, stride, counts, th, method, steps, th_mult, ph_mult, max_loss, E, d_masks, n_inliers, status,
                                           steps_done, s, who);
        if (rc) return rc;
        for (int b = 0; b < B; ++b) {
            rt_valid[b] = 0;
            if (attempts_used) attempts_used[b] = 0;
        }
        return MLPL_OK;
    }
    if (B < 1 || stride < 1 || !d_p1 || !d_p2 || !counts || !th || !E || !d_masks || !n_inliers || !status || steps < 0 || !std::isfinite(th_mult) ||
        !std::isfinite(ph_mult) || !std::isfinite(max_loss)) {
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
    int rc;
    void *d_prob, *d_lists, *d_work;
    const size_t prob_bytes = (size_t)B * sizeof(KneipProb), sums_bytes = (size_t)B * kKneipSumsStride * 8, cand_bytes = (size_t)B * kKneipAttempts * 72;
    if ((rc = ws_get(ctx, WS_AUX2, prob_bytes, &d_prob))) return rc;
    if ((rc = ws_get(ctx, WS_AUX3, (size_t)B * 2 * stride * 4, &d_lists))) return rc;
    if ((rc = ws_get(ctx, WS_AUX4, sums_bytes + cand_bytes, &d_work))) return rc;
    KneipArgs A{};
    A.p1 = d_p1, A.p2 = d_p2, A.stride = stride, A.prob = (KneipProb *)d_prob, A.masks = d_masks, A.lists = (int32_t *)d_lists;
    A.sums = (double *)d_work, A.E = (const double *)((char *)d_work + sums_bytes), A.e_stride = 9, A.max_loss = max_loss;

    struct Host {
        bool active = true, have_rot = false, posed = false;
        int st = MLPL_OK, cnt = 0, side = 0, done = 0, attempts = 0, K = 0;
        uint32_t valid = 0;
        double E[9], R_start[9], R_acc[9], t_acc[3];
        double cR[kKneipAttempts][9], ct[kKneipAttempts][3], cE[kKneipAttempts][9];
    };
    std::vector<Host> H((size_t)B);
    std::vector<KneipProb> P((size_t)B);
    std::vector<double> sums((size_t)B * kKneipSumsStride), cand((size_t)B * kKneipAttempts * 9);
    for (int b = 0; b < B; ++b) {
        std::memcpy(H[b].E, E + (size_t)b * 9, 72);
        if (rt_valid[b]) std::memcpy(H[b].R_start, R + (size_t)b * 9, 72);
        else std::memset(H[b].R_start, 0, 72);  // the reference's R_inout stays zero when no R is handed in
        H[b].have_rot = kneip_is_rotation(H[b].R_start);
        std::memset(&P[b], 0, sizeof(KneipProb));
        P[b].n = counts[b];
    }
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point c) { return std::chrono::duration<double>(c - a).count(); };
    if (times) *times = KneipTimes{0, 0, 0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (times) {
        MLPL_HIP_TRY(hipEventCreate(&ev[0]));
        MLPL_HIP_TRY(hipEventCreate(&ev[1]));
    }
    // one launch between an upload of the problem records and their download; returns with the stream idle
    auto round = [&](bool eval, bool with_cand, bool want_sums) -> int {
        const auto t0 = clk::now();
        MLPL_HIP_TRY(hipMemcpyAsync(d_prob, P.data(), prob_bytes, hipMemcpyHostToDevice, s));
        if (with_cand) MLPL_HIP_TRY(hipMemcpyAsync((void *)A.E, cand.data(), (size_t)B * A.e_stride * 8, hipMemcpyHostToDevice, s));
        if (times) MLPL_HIP_TRY(hipEventRecord(ev[0], s));
        if (eval) hipLaunchKernelGGL(kneip_eval_kernel, dim3(B), dim3(kSolverThreads), 0, s, A);
        else hipLaunchKernelGGL(kneip_sums_kernel, dim3(B), dim3(kSolverThreads), 0, s, A);
        MLPL_HIP_TRY(hipGetLastError());
        if (times) MLPL_HIP_TRY(hipEventRecord(ev[1], s));
        MLPL_HIP_TRY(hipMemcpyAsync(P.data(), d_prob, prob_bytes, hipMemcpyDeviceToHost, s));
        if (want_sums) MLPL_HIP_TRY(hipMemcpyAsync(sums.data(), A.sums, sums_bytes, hipMemcpyDeviceToHost, s));
        MLPL_HIP_TRY(hipStreamSynchronize(s));
        if (times) {
            float ms = 0;
            MLPL_HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
            (eval ? times->eval : times->sums) += ms * 1e-3;
            times->hops += secs(t0, clk::now()) - ms * 1e-3;
        }
        return MLPL_OK;
    };
    auto finish = [&]() {
        if (ev[0]) (void)hipEventDestroy(ev[0]);
        if (ev[1]) (void)hipEventDestroy(ev[1]);
    };
    GlibcRand gen;
    std::vector<int> todo;
    for (int j = 0; j < steps; ++j) {
        bool any = false;
        for (int b = 0; b < B; ++b) {
            P[b].act = H[b].active ? (j == 0 ? 1 : 2) : 0;
            P[b].cnt = H[b].cnt, P[b].side = H[b].side;
            any = any || H[b].active;
        }
        if (!any) break;
        if ((rc = round(false, false, true))) return finish(), rc;
        todo.clear();
        for (int b = 0; b < B; ++b) {
            if (!H[b].active) continue;
            if (j == 0) {
                H[b].cnt = P[b].cnt;
                if (H[b].cnt < kLinRefineMinInliers) {
                    H[b].active = false, H[b].st = MLPL_E_FAILED;
                    continue;
                }
            }
            todo.push_back(b);
        }
        // ---- the solves: twelve perturbed starts where step 0 has no rotation to start from, else one ----
        std::vector<int32_t> raw((size_t)B * 3 * kKneipAttempts);
        if (j == 0)
            for (int b : todo)
                if (!H[b].have_rot) {
                    gen.seed(seeds ? seeds[b] : 1u);
                    for (int k = 0; k < 3 * kKneipAttempts; ++k) raw[(size_t)b * 3 * kKneipAttempts + k] = gen.next();
                }
        const auto t_solve = clk::now();
        kneip_parallel(todo.size(), [&](size_t at) {
            const int b = todo[at];
            Host &h = H[b];
            const double *sm = sums.data() + (size_t)b * kKneipSumsStride;
            h.valid = 0;
            if (j == 0 && !h.have_rot) {
                h.K = kKneipAttempts;
                for (int a = 0; a < kKneipAttempts; ++a) {
                    double R0[9];
                    kneip_perturbed_identity(raw.data() + ((size_t)b * kKneipAttempts + a) * 3, R0);
                    if (kneip_solve(sm, R0, h.cR[a], h.ct[a], h.cE[a])) h.valid |= 1u << a;
                    else std::memset(h.cE[a], 0, 72);
                }
            } else {
                h.K = 1;
                if (kneip_solve(sm, h.R_start, h.cR[0], h.ct[0], h.cE[0])) h.valid = 1u;
            }
        });
        if (times) times->solve += secs(t_solve, clk::now());
        int kmax = 0;
        any = false;
        for (int b = 0; b < B; ++b) P[b].act = 0;
        for (int b : todo) {
            Host &h = H[b];
            if (!h.valid) {  // no model: the loop is left with what was accepted so far (at step 0: E unchanged, no pose)
                h.active = false;
                if (h.K == kKneipAttempts) h.attempts = kKneipAttempts;
                continue;
            }
            kmax = std::max(kmax, h.K);
            any = true;
        }
        if (!any) continue;
        A.e_stride = 9 * kmax;
        for (int b : todo) {
            Host &h = H[b];
            if (!h.valid) continue;
            const double th2 = th[b] * th[b];
            const double step_size = (th_mult * th2 - th2) / steps;
            P[b].act = 1, P[b].K = h.K, P[b].valid = h.valid, P[b].gate = h.K == kKneipAttempts ? 1 : 0;
            P[b].thr_gate = th2, P[b].thr = (th_mult * th2) - (double)(j + 1) * step_size;
            P[b].cnt = h.cnt, P[b].side = h.side, P[b].chosen = -1, P[b].cnt2 = 0, P[b].accepted = 0;
            for (int a = 0; a < h.K; ++a) std::memcpy(cand.data() + (size_t)b * A.e_stride + a * 9, h.cE[a], 72);
        }
        if ((rc = round(true, true, false))) return finish(), rc;
        for (int b : todo) {
            Host &h = H[b];
            if (!h.valid) continue;
            const int c = P[b].chosen;
            if (h.K == kKneipAttempts) h.attempts = c < 0 ? kKneipAttempts : c + 1;
            if (c < 0) {  // every attempt failed its own test: the reference leaves the loop and returns true
                h.active = false;
                continue;
            }
            if (c >= h.K) return finish(), set_error("%s: problem %d: candidate %d of %d", who, b, c, h.K), MLPL_E_INTERNAL;
            if (P[b].accepted) {
                std::memcpy(h.E, h.cE[c], 72);
                std::memcpy(h.R_acc, h.cR[c], 72);
                std::memcpy(h.t_acc, h.ct[c], 24);
                std::memcpy(h.R_start, h.cR[c], 72);
                h.posed = true, h.cnt = P[b].cnt2, h.side ^= 1, ++h.done;
            } else {
                h.active = false;
                if (j == 0) h.st = MLPL_E_FAILED;
            }
        }
    }
    // ---- the masks: 0/1 of the last accepted list; without a step, of the mask itself ----
    for (int b = 0; b < B; ++b) {
        P[b].act = H[b].st == MLPL_OK ? (steps > 0 ? 2 : 3) : 0;
        P[b].cnt = H[b].cnt, P[b].side = H[b].side;
    }
    if ((rc = round(true, false, false))) return finish(), rc;
    finish();
    for (int b = 0; b < B; ++b) {
        Host &h = H[b];
        if (steps == 0) {
            h.cnt = P[b].cnt;
            if (h.cnt < kLinRefineMinInliers) h.st = MLPL_E_FAILED;
        }
        const bool ok = h.st == MLPL_OK;
        status[b] = h.st;
        n_inliers[b] = ok ? h.cnt : 0;
        if (steps_done) steps_done[b] = ok ? h.done : 0;
        if (attempts_used) attempts_used[b] = h.attempts;
        if (!ok) continue;  // the reference returns false: nothing is touched (rt_valid included)
        std::memcpy(E + (size_t)b * 9, h.E, 72);
        // pose_linear_refinement.cpp:272-293: R_inout a rotation and t_out not zero; both are set by accepted steps only
        if (h.posed) {
            std::memcpy(R + (size_t)b * 9, h.R_acc, 72);
            std::memcpy(t + (size_t)b * 3, h.t_acc, 24);
            rt_valid[b] = 1;
        } else {
            rt_valid[b] = 0;
        }
    }
    return MLPL_OK;
}
