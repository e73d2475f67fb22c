// mlpl_internal.h -- shared by the HIP translation units of libmlpl_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "mlpl_c.h"
#include "mlpl_debug.h"

namespace mlpl {

void set_error(const char *fmt, ...);

// The guard of the C boundary.  Every entry is a function-try-block,
//     int mlpl_x(...) try { body } MLPL_ENTRY_END("mlpl_x")
// and entry_failed, called from its handler, rethrows the exception in flight and turns it into an error: std::bad_alloc ->
// MLPL_E_NOMEM, anything else -> MLPL_E_INTERNAL, the text names the entry.  Nothing leaves it.
int entry_failed(const char *who) noexcept;
#define MLPL_ENTRY_END(who) catch (...) { return ::mlpl::entry_failed(who); }

// counts[b] in [lo, stride] for every problem of a batch entry; otherwise the error is set and the answer is false
bool counts_in_range(const char *who, int n_problems, const int32_t *counts, int lo, int stride);

#define MLPL_HIP_TRY(expr)                                                                                  \
    do {                                                                                                    \
        hipError_t e__ = (expr);                                                                            \
        if (e__ != hipSuccess) {                                                                            \
            ::mlpl::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__));        \
            return MLPL_E_HIP;                                                                              \
        }                                                                                                   \
    } while (0)

// Workspace slots: each grows monotonically and is reused across calls (no hipMalloc on the steady path).
enum WsSlot {
    WS_PACK_Q = 0,
    WS_PACK_T,
    WS_PARTIAL,
    WS_IDX,
    WS_DIST,
    WS_MATCH,
    WS_COUNT,
    WS_AUX0,
    WS_AUX1,
    WS_AUX2,
    WS_AUX3,
    WS_AUX4,
    WS_AUX5,
    WS_AUX6,
    WS_AUX7,
    WS_SCALARS,   // small host-readable outputs of the host-pointer entry points (match counts)
    WS_L2_FLAG,   // device gate flag of the L2 auto path
    WS_FRAG_Q,    // fp4 MFMA fragments of the query / train descriptors (knn_hamming_mfma.hip)
    WS_FRAG_T,
    WS_PIPE,      // per-pair pipeline block (mlpl_pair_pose_dev)
    WS_DEBUG,     // diagnostics (per-wave clock stamps)
    WS_COUNTERS,  // chunk counters of the dynamic-split Hamming kernel
    WS_SPLIT_TAB, // age-aware split table of the static LDS-ring Hamming kernel
    WS_ARR_E,     // ARRSAC: models of every sample solved in a call
    WS_ARR_F,     // ARRSAC: their inlier bit rows
    WS_F16_Q,     // fp16 L2 path (knn_l2_f16.hip): hi / lo fragments of the queries, of the train rows, row constants, partial U pairs, candidates
    WS_F16_T,
    WS_F16_CST,
    WS_F16_PART,
    WS_F16_CAND,
    WS_BATCH_SMP, // mlpl_pair_pose_batch_dev: sample tables of a pass (drawn on the device), stream positions
    WS_RAND_RAW,  // raw rand() stream of the last RANSAC seed on the device + the control block of the device-side sampling
    WS_BATCH_RUNS, // device blocks of the runs of a batched sequential estimator (USAC / ARRSAC), one slice per run
    WS_CLOCK,     // clock ring of the Hamming kernel (option hamming_stamps = 2): kClockRing records of 4 x u64
    WS_SCAN,      // pass counts of the merge workgroups when the merge kernel emits the matches itself (knn_hamming.hip MergeEmit)
    WS_TICKETS,   // ticket counters of the fused Hamming epilogue (zero between launches; knn_hamming_mfma.hip)
    WS_VFC,       // VFC match filter (vfc.hip): per-point state, per-problem results, the raw rand() values of the control-point draws
    WS_GMS,       // GMS match filter (gms.hip): per-match cell codes, buckets and flags, per-problem results
    WS_SUBPIX,    // sub-pixel refinement (subpix.hip): per-match records and positions, per-keypoint winners, per-list results and tickets
    WS_SUBPIX_SEP,      // cornerSubPix refinement (subpix_separate.hip): per-match records and positions, per-keypoint winners, per-list results and tickets
    WS_SUBPIX_SEP_MASK, // ... its eight mask profiles (uploaded when the context is created)
    WS_BA,              // bundle adjustment (bundle_adjust.hip): per-point state of every problem, then the compacted row lists
    WS_BA_MULTICAM,     // multi-camera bundle adjustment (bundle_adjust_multicam.hip): per-point state of every problem
    WS_BA_MULTICAM_IO,  // ... its per-problem input and result blocks
    WS_HOMOG,           // homography ARRSAC (homography_impl.h): packed correspondences, the models of every sample solved in a call, the compacted inliers
    WS_HOMOG_PLANES,    // estimateMultHomographys: the two point buffers the rounds alternate between, the round's mask, the planes' masks
    WS_HOMOG_ALIGN,     // homography alignment (homography_align_impl.h): the result block and the correspondences sorted by plane
    WS_RECTIFY,         // stereo rectification (rectify.hip): the per-image map parameters of the fused, batched entry
    WS_NUM_SLOTS
};

int launch_gather_match_points(const mlpl_dmatch *d_matches, int n, const float *d_kp1, const float *d_kp2, const double K0[4],
                               const double K1[4], double *d_p1, double *d_p2, hipStream_t s);

// Device gate of the L2 auto path: *flag == gen <=> the descriptors of call `gen` are not integer-valued in [0,255] (knn_l2_mfma.hip).
// flag == nullptr: no gate.
struct L2Gate {
    const int *flag;
    int gen;
};

bool knn_l2_f16_applicable(int dim, int nt, int k);

}  // namespace mlpl

struct mlpl_ctx {
    int device;
    hipStream_t stream;
    hipStream_t aux_stream[2];     // helper streams of the RANSAC driver: the root kernels of the slices run beside the elimination kernels and each other
    hipEvent_t aux_ev[8];          // fork/join events for them (timing disabled)
    void *ws[mlpl::WS_NUM_SLOTS];
    size_t ws_bytes[mlpl::WS_NUM_SLOTS];
    void *pinned;  // small pinned host scratch for async result readback
    size_t pinned_bytes;
    void *pinned_batch;  // pinned, device-mapped block of the batched sequential estimators (one slice per run; csrc/usac_batch.h)
    size_t pinned_batch_bytes;
    void *hub_streams;   // what the launch hubs keep between calls (HubStreams, csrc/batch_hub.h: streams, events, item tables, run threads; created on first use)
    int l2_mode;
    int opt_l2_mfma_waves;          // waves per workgroup of the L2 matrix-core kernel: 4, 8 or 0 = automatic
    int opt_l2_mfma_blocks_per_cu;  // its grid sizing target (0 = automatic)
    int l2_gen;         // call counter of the L2 auto path (see L2Gate)
    int opt_l2_float_mfma;  // non-integer float descriptors: 0 = exact fp32 kernel, 1 (default) = fp16 matrix-core candidates + exact re-rank once the
                            // previous call's data were seen to be non-integer (hint, no host hop), 2 = always enqueue that path
    int *l2_hint_host;      // pinned + device-mapped: 2 * generation + (not integer-valued) of the last auto call that has finished on the device
    int *l2_hint_dev;
    int opt_l2_fold_counts; // 1 (default) = mlpl_match_l2_dev's split fold evaluates the ratio predicate and writes the pass counts (knn_l2_fold_ratio_kernel);
                            // 0 = knn_l2_merge_kernel + ratio_count_kernel (A/B, tests)
    int dbg_l2_match[4];    // mlpl_debug_last_l2_match: {path, train splits, counts by the fold, launches} of the last float knn / match call
    void *l2_flag_ptr;  // the flag buffer l2_gen counts for
    int kneip_times_on;     // mlpl_kneip_refine_times: measure the next PR_KNEIP refinements
    double kneip_times[4];  // {sums kernel, host solves, eval kernel, hops} of the last one, seconds
    int num_cus;
    // tuning knobs (mlpl_set_option)
    int opt_hamming_variant;        // 3 = fp4 matrix-core kernel (default), 0 = LDS-tiled VALU, 1 = scalar-operand VALU, 2 = one wave per block
    int opt_hamming_qpl;            // queries per lane for variant 1 (1 or 2)
    int opt_hamming_blocks_per_cu;  // grid sizing target
    int opt_hamming_mfma_blocks_per_cu;  // grid sizing target of the matrix-core kernel (4-wave blocks)
    int opt_hamming_mfma_qt;             // query tiles per wave (0 = automatic, else 1, 2 or 4)
    int opt_hamming_mfma_lds;       // 32-byte descriptors: 1 (default) = LDS-ring kernel with static train splits, 2 = LDS ring with dynamic splits, 0 = register-prefetch kernel
    int opt_hamming_mfma_waves;     // waves per workgroup of the static LDS-ring kernel: 0 (default) = automatic (8 with four query tiles per wave, else 4), 4, 8, 16 (four query tiles per wave only)
    int opt_hamming_split_rows;     // cap on the train rows of one split: 0 (default) = 8192, the exactness bound of the row fraction; 4096 = the cap up to round 4
    int opt_hamming_mfma_prefetch;  // prefetch distance of the ring in tiles with 8-wave workgroups: 0 / 2 (default), 4, 6
    int opt_hamming_mfma_prio;      // 1 = the LDS-ring kernel rotates wave priorities on a clock slice (equal finish times per SIMD; measured: no faster); 3 = the wave-uniform top-2 skip (<4, 3, 8> only; measured: no faster). Default 0
    int opt_hamming_mfma_weighted;  // 1 (default) = age-aware split sizes in the static LDS-ring kernel (4 workgroups per CU)
    long long split_tab_key;        // shape key of the split table currently in WS_COUNTERS
    void *split_tab_ptr;
    int opt_hamming_fused_merge;    // 1 (default) = the static LDS-ring kernel merges its splits / evaluates the ratio predicate itself (no merge launch)
    void *hamming_tickets_ptr;      // zeroed ticket counters of that merge (WS_TICKETS) ...
    size_t hamming_tickets_bytes;   // ... and how many bytes of them are known to be zero
    int opt_hamming_expand_fine;    // 1 (default) = small launches expand the train set with one thread per (tile, K-step, lane)
    int opt_hamming_stamps;         // diagnostics: 1 = the matrix-core kernel records per-wave clock stamps (mlpl_debug_hamming_stamps); 2 = one clock record per launch into a ring (mlpl_debug_hamming_clock)
    long long hamming_clock_launches;   // launches recorded into the clock ring so far
    int opt_hamming_merge_emit;     // 1 = one image pair per call: the merge kernel writes the DMatch rows itself (no ratio_write launch); default 0: measured, no faster
    void *hamming_scan_ptr;         // the WS_SCAN block the generation below counts for
    size_t hamming_scan_bytes;      // ... and its size when it was zeroed (a regrown block may return at the same address, never at the same size)
    uint32_t hamming_scan_gen;
    int opt_hamming_train01;        // 1 = {0, +1} train fragments in the static LDS-ring kernel (accumulator = pop(query) - distance), 0 = +-1
    int opt_vfc_store_u;            // 1 = the VFC kernel keeps the m x n kernel matrix U in the workspace; 0 (default, unmeasured: DESIGN section 8) = it recomputes U in both passes of an iteration
    int opt_hamming_expand_inkernel;   // 1 = the static LDS-ring kernel's throughput instance expands the raw train tiles itself (no expansion launch, no WS_FRAG_T)
    int opt_hamming_block_top2;        // 0 = the ring kernel folds every candidate into its running top-2; 4 = the in-kernel-expansion instances fold the maxima of blocks of four candidates and re-score the best row's block in the epilogue (same results)
    int opt_hamming_mfma_shape;        // 32 = v_mfma_f32_32x32x64_f8f6f4 everywhere; 16 = the throughput instance of the static ring kernel (eight waves, in-kernel expansion, block update, no stamps trace) runs on 16x16x128 (same results)
    int dbg_hamming_shape;             // MFMA shape the last Hamming launch really used (mlpl_debug_last_hamming_shape; 0 = a VALU kernel)
    int dbg_hamming_top2;              // block size the last Hamming launch really used (mlpl_debug_last_hamming_top2)
    int dbg_hamming_block_rows;        // train rows per block of the instance that ran: 0, 4, or 8 in the 16x16x128 form (mlpl_debug_last_hamming_block_rows)
    void *subpix_sep_mask_ptr;      // the WS_SUBPIX_SEP_MASK block that holds the mask profiles of subpix_separate.hip
    int dbg_stamp_items;
    // diagnostics (mlpl_debug_last_kernels): what the last launches chose -- {count instance code, its point splits} of the last
    // inlier-count pass, and the Hamming instance of the last knn_hamming call (layout: include/mlpl_debug.h)
    int dbg_count_kernel[2];
    int dbg_hamming_kernel[11];
    int opt_ransac_chunk;           // hypotheses per device pass (0 = 32768)
    int opt_ransac_event_cap;       // tests: capacity of the record-event list of candidate / replay kernels (0 = 1024); forces their serial fallback
    int opt_ransac_count_mpl;       // models per lane of the packed-fp32 counting kernel: 2 (default) or 1
    int opt_ransac_count_threads;   // threads per workgroup of the counting kernel: 256 (default since round 6: 4 waves, 96 VGPRs, five workgroups per CU) or 512 (rounds 2-5: 8 waves, two per CU)
    int opt_ransac_count_wpe;       // waves per SIMD the 256-thread counting kernel's registers are cut for: 5 (96 VGPRs) or 6 (80 VGPRs, a few spills outside the loop)
    int opt_ransac_count_tiles;     // 512-correspondence tiles one workgroup of the counting pass walks: 2 (rounds 3-5) or 1 (more, shorter workgroups: less idle tail)
    int opt_ransac_count_defer;     // 1 (default) = the packed-fp32 counting kernel queues its undecided evaluations in LDS and decides them workgroup-wide (same counts)
    int opt_ransac_f32_filter;      // 1 (default) = the count-only scoring kernels pre-filter in packed fp32 inside a rigorous error band (same counts)
    int opt_ransac_overlap;         // 1 (default) = large passes run their root kernels on the helper stream
    int opt_ransac_dev_split;      // device-drawn passes above 8192 hypotheses: per mille of the pass in the first of two solver slices (0 = one slice)
    int opt_ransac_lazy_sums;       // 1 (default) = division-free inlier counts + error sums only for models that can still win
    int opt_solver_polish;          // 1 (default) = every 5-point solution is finished by <= 4 Gauss-Newton steps on the cubic constraints (repairs the samples on which the DEVICE's elimination is ill conditioned); 0 = plain root path (A/B)
    int opt_solver_wave3;           // 1 (default) = solve5pt3_kernel (three hypotheses per wave, matrices in registers); 0 = one per wave
    int opt_ransac_host_table;      // 1 = always build the niters table on the host (default: evaluate on the device, verify)
    // cached table T[g] = cvRANSACUpdateNumIters1(conf, (n-g)/n, 5, inf) for the last (n, conf) (host libm values)
    int opt_rand_cache_max;         // tests: values of the rand() stream kept per context (0 = 4 Mi); beyond it a call generates privately
    void *rand_cache;               // raw rand() stream of the last RANSAC / LMedS seed (ransac_5pt.hip: RandCache)
    int32_t *ransac_T_host;
    int ransac_T_n;
    double ransac_T_conf;
    int ransac_force_table;        // 1 = build the host niters table (fallback / tests)
    int ransac_force_host_draw;    // 1 = draw the sample table on the host (fallback of the device-side sampling)
    int opt_ransac_device_draw;    // 1 (default) = passes of >= 4096 hypotheses draw their samples on the device from the cached raw stream
    void *rand_dev_ptr;            // the WS_RAND_RAW block the fields below describe
    unsigned rand_dev_seed;
    size_t rand_dev_len;           // values of srand(rand_dev_seed) / rand() present on the device
    long long ransac_draw_fallbacks;
    int last_ransac_dev_draw;      // the last mlpl_ransac_essential* call drew its samples on the device
    long long ransac_table_fallbacks;  // calls redone on the host table because a device-evaluated bound differed
    long long last_ransac_models, last_ransac_iters;  // statistics of the last mlpl_ransac_essential* call
    int32_t *arrsac_trace;                             // diagnostics: host buffer for the turn records of ARRSAC's first stage
    int arrsac_trace_cap, arrsac_trace_len;
    long long last_arrsac_stats[12];                   // ... of the last mlpl_arrsac_essential* call (mlpl_arrsac_last_stats)
    double *usac_trace;                                // diagnostics: host buffer for the decision records of USAC (16 doubles each)
    int usac_trace_cap, usac_trace_len;
    long long last_usac_stats[8];
    double last_usac_degen[16];                        // {tests on, inliers of the rotation, of "no motion", degeneracy type, R[9]}
    uint8_t *last_usac_flags;                          // malloc'ed, 2 * last_usac_flags_n bytes: inlier masks of the rotation / of "no motion"
    int last_usac_flags_n;
    unsigned *usac_prosac_tab;                         // calloc'ed, 1001 entries: PROSAC's non-randomness table of the last (beta, confidence) (usac_impl.h init_prosac)
    unsigned usac_prosac_tab_top;
    double usac_prosac_tab_beta, usac_prosac_tab_conf;
    float hop_us[48];                                  // diagnostics: microseconds since entry of the last mlpl_pair_pose_batch_dev call at its host hops ...
    int hop_code[48], hop_n;                           // ... 1 launches enqueued, 2 match counts back, 3 / 4 a pass enqueued / its states back, 5 / 6 pose enqueued / back
    long long ws_grows;                                // workspace / pinned blocks (re)allocated so far (a hipMalloc inside a call shows up here)
    long long last_batch_stats[8];                     // mlpl_pair_pose_batch_dev: {RANSAC passes, pair slots over all passes, pairs redone on a host table, 0}
    int opt_pair_batch;                                // pairs per internal batch of mlpl_pair_pose_batch_dev (0 = 256)
    int opt_pair_batch_feed;                           // 1 (default): the USAC / ARRSAC pair entries match cohort c + 1 while the estimators of cohort c run (pair_batch_usac.h)
    int opt_pair_batch_seq;                            // ... of mlpl_pair_pose_batch_usac_dev / _arrsac_dev (0 = 512)
    int opt_hub_lanes;                                 // cohorts in flight (0 = the estimator's own choice: six for USAC with REF_WEIGHTS, four otherwise; at most 8)
    int opt_eig_inverse_iteration;                     // 1 (default): the smallest eigenvector of the re-weighted 9 x 9 fits (USAC REF_WEIGHTS, robustEssentialRefine) by inverse iteration, Jacobi as the fallback
    int opt_hub_blocking_sync;                         // 1: a lane's thread sleeps on an event at the end of a round instead of spinning in hipStreamSynchronize
    int opt_hub_workers;                               // worker threads per cohort (0 = 16): the runs of a cohort are fibers on them
    int opt_hub_cohort;                                // runs of a batched USAC / ARRSAC call that advance together (0 = 128; two such cohorts are in flight)
    int opt_pair_batch_raw_cap;                        // tests: rand() values kept per pair for the device-side sampling (0 = 6.25 per iteration + 1024)
    int opt_arrsac_flag_points;                        // tests: correspondences every ARRSAC model is tested on up front (0 = 1024)
    int opt_arrsac_refine_warm_start;                  // 1 (default): robustEssentialRefine's rounds start their Jacobi iteration from the previous round's eigenvectors
    int opt_usac_first_batch;                          // samples in the first speculative batch of a USAC run (0 = as every batch: up to 128; measured, no robust gain from smaller ones)
    int opt_usac_lo5_fused_fit;                        // 1 (default): a fit of a usac5_* chain (solve -> roots -> choose) is one launch; 0 = three
    int opt_usac_lo_warm_start;                        // 1 (default): a refit of a local-optimisation chain starts its Jacobi iteration from the previous fit's eigenvectors
    int opt_usac_sprt_fast;         // 1 (default) = a sequential test that survives its first 128 steps is finished word by word on bounds (usac_impl.h sprt_walk)
    int opt_usac_lo_stepwise;                          // tests: every step of a local-optimisation chain goes through the resume path
    // optional per-kernel hipEvent bracketing (mlpl_profile_*)
    int prof_on;
    hipEvent_t *prof_ev[MLPL_PROF_NUM];  // pairs: [2*i] start, [2*i+1] stop
    int prof_n[MLPL_PROF_NUM];
    int prof_calls[MLPL_PROF_NUM];  // launches seen since the last reset (sampling: every prof_on-th is bracketed)
    int prof_take[MLPL_PROF_NUM];
};

namespace mlpl {

// Returns a device buffer of at least `bytes` for `slot`, growing it if needed (grow = sync + realloc).  A slot must not
// be requested twice with different sizes inside one entry point while the first pointer is still in use: every purpose
// that can coexist in a call has its own slot (see the WsSlot comments and the call sites).
int ws_get(mlpl_ctx *ctx, WsSlot slot, size_t bytes, void **out);
int pinned_get(mlpl_ctx *ctx, size_t bytes, void **out);
int pinned_batch_get(mlpl_ctx *ctx, size_t bytes, void **out);
void hub_streams_free(void *p);

// The correspondences of a host-pointer entry on the device: p1 -> WS_AUX0, p2 -> WS_AUX1 (n x 2 doubles each, sized for max(n, 1)), copied
// on ctx->stream when n > 0.  match_bytes > 0: *d_match = WS_MATCH with that many bytes (the entry's mask or labels; the entry fills it).
int upload_points(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const double **d_p1, const double **d_p2, size_t match_bytes = 0,
                  void **d_match = nullptr);
// ... and a mask of n bytes back to the host once the entry's work on the stream is done (a blocking copy)
int download_mask(uint8_t *mask, const void *d_mask, int n);

constexpr int kProfMaxLaunches = 2048;
constexpr int kClockRing = 256;  // launches the Hamming clock ring keeps
// Records the start (phase 0) / stop (phase 1) event of one launch of kernel `id` on stream s when profiling is on.
void prof_mark(mlpl_ctx *ctx, int id, int phase, hipStream_t s);

// `stream` of the *_dev entry points is a hipStream_t; NULL is HIP's null (legacy default) stream, as everywhere
// in HIP.  The context's private stream is only used by the host-pointer entry points.
inline hipStream_t pick_stream(mlpl_ctx *, void *stream) { return reinterpret_cast<hipStream_t>(stream); }

// ---- kernel launchers (defined in the .hip files) ----
// emit_out (optional): the caller wants the DMatch rows (out [batch][nq], n_out [batch]); *emitted = 1 when the Hamming path wrote them
// itself (the merge kernel of the latency shape) and launch_ratio_compact is not needed.
struct HammingEmitOut {
    mlpl_dmatch *out;
    int32_t *n_out;
    int emitted;
};
int launch_knn_hamming(mlpl_ctx *ctx, const uint8_t *d_q, int nq, size_t q_stride, size_t q_bstride,
                       const uint8_t *d_t, int nt, size_t t_stride, size_t t_bstride, int nbytes, int k, int batch,
                       int32_t *d_idx, int32_t *d_dist, hipStream_t s, float ratio = 0.75f,
                       int32_t *d_group_counts = nullptr, HammingEmitOut *emit_out = nullptr);
int launch_knn_l2(mlpl_ctx *ctx, const float *d_q, int nq, size_t q_stride, size_t q_bstride, const float *d_t,
                  int nt, size_t t_stride, size_t t_bstride, int dim, int k, int batch, int32_t *d_idx,
                  float *d_dist, hipStream_t s, int nms_order = 0, float ratio = 0.f, int32_t *d_group_counts = nullptr,
                  int *counts_done = nullptr);
// (d_group_counts: the caller wants the pass counts of the ratio predicate at `ratio` in the layout ratio_write_kernel reads, as
// launch_knn_hamming's; *counts_done = 1 when the path taken wrote them -- every path that ends in the split fold --, 0 when the caller
// still has to run ratio_count_kernel: the fp16 candidate path, which ends in its own re-rank kernel)
// group_counts_ready: d_group_counts (one int per kCountGroup queries per batch item, in the context workspace slot
// WS_COUNT) was already filled by knn_hamming_merge_kernel; otherwise a counting pass runs first.
constexpr int kRatioGroup = 256;  // queries per ratio_write block
constexpr int kCountGroup = 64;   // queries per entry of the pass-count table
int launch_ratio_compact(mlpl_ctx *ctx, const int32_t *d_idx, const void *d_dist, int dist_is_float, int nq, int k,
                         int batch, float ratio, mlpl_dmatch *d_out, int32_t *d_n_out, hipStream_t s,
                         int32_t *d_group_counts_ready = nullptr, int nms_emit = 0);

int launch_gather_match_points(const mlpl_dmatch *d_matches, int n, const float *d_kp1, const float *d_kp2, const double K0[4],
                               const double K1[4], double *d_p1, double *d_p2, hipStream_t s);
void free_rand_cache(void *p);

// The descriptors of a batch of image pairs, dense: q [pairs][nq][cols], t [pairs][nt][cols] elements of `type` -- 0 = CV_8U (bytes,
// Hamming), 5 = CV_32F (floats, squared L2), as mlpl_get_matches_linear's desc_type.  q == nullptr: no descriptors (correspondence mode).
struct DescView {
    const void *q, *t;
    int cols, type;
    size_t elem() const { return type == 5 ? sizeof(float) : 1; }
    DescView pair(size_t b, int nq, int nt) const {
        return DescView{(const char *)q + b * nq * cols * elem(), (const char *)t + b * nt * cols * elem(), cols, type};
    }
};
// The matching step of the pair entries: mlpl_match_hamming_dev / mlpl_match_l2_dev (ratio test at 0.75f) on `batch` pairs of the view,
// q_bstride / t_bstride in elements.  The idx / dist slots are 4 bytes per element either way.
int match_dev(mlpl_ctx *ctx, const DescView &v, int nq, size_t q_bstride, int nt, size_t t_bstride, int batch, int32_t *d_idx, void *d_dist,
              mlpl_dmatch *d_out, int32_t *d_n_out, hipStream_t s);
// mlpl_pair_pose_dev / mlpl_pair_pose_f32_dev on the first pair of the view
int pair_pose_one(mlpl_ctx *ctx, const DescView &v, int nq, int nt, const float *d_kp1, const float *d_kp2, const double K0[4], const double K1[4],
                  double thresh, int max_iters, double confidence, int refit, uint32_t seed, double dist, mlpl_pair_result *out, void *stream);

// cheirality for a batch of pairs (recover_pose.hip): decomposition, four triangulations, the reference's candidate choice and the mask
// of the chosen candidate, all on the device; d_out[pair] = {valid 3-D points, candidate (-1 none), R, t}
struct PairPoseDev {
    int32_t n_good, pick;
    double R[9], t[3];
};
int launch_recover_pose_batch(const char *d_E_base, size_t E_stride, const double *d_p1, const double *d_p2, const int32_t *d_counts,
                              const int32_t *d_active, int B, int pair_stride, double dist, uint8_t *d_mask, double *d_P,
                              uint8_t *d_cand_masks, int32_t *d_cand_counts, PairPoseDev *d_out, hipStream_t s);
int launch_gather_match_points_batch(const mlpl_dmatch *d_matches, const int32_t *d_counts, int B, int pair_stride, const float *d_kp1,
                                     size_t kp1_stride, const float *d_kp2, size_t kp2_stride, const double K0[4], const double K1[4],
                                     double *d_p1, double *d_p2, hipStream_t s);


// VFC match filter (vfc.hip).  Points either through a match list and keypoints (d_matches [batch][match_stride], d_n_matches [batch],
// d_kp1 [batch][nq][2], d_kp2 [batch][nt][2]) or directly (d_matches == nullptr, batch = 1: d_x1 / d_x2 [n_direct][2]); seeds: host,
// [batch] or nullptr (= 1).  One launch and one small upload on s, no synchronisation.  *work (optional) receives the workspace views of the
// launch: keep [batch][stride] bytes, P [batch][stride], res [batch][8] = {status, kept, control points, iterations, normalisation
// refused, singular solves, n_out, 0}.
struct VfcWork {
    const uint8_t *keep;
    const double *P;
    const int32_t *res;
    size_t stride;
};
int launch_vfc(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches, const float *d_kp1, int nq,
               const float *d_kp2, int nt, const float *d_x1, const float *d_x2, int n_direct, const uint32_t *seeds, int rule, mlpl_dmatch *d_out,
               int32_t *d_n_out, int32_t *d_status, VfcWork *work, hipStream_t s);

// GMS match filter (gms.hip) on match lists and keypoints (d_matches [batch][match_stride], d_n_matches [batch] or nullptr = n_direct for
// every problem, d_kp1 [batch][nq][2], d_kp2 [batch][nt][2]).  One launch on s, no upload, no synchronisation.  *work (optional) receives the
// workspace views of the launch: keep [batch][stride] bytes, res [batch][8] = {count, winning scale level or -1, winning rotation type or
// -1, matches dropped by the out-of-bounds rule in the winning run, n_out, 0, 0, 0}.
struct GmsWork {
    const uint8_t *keep;
    const int32_t *res;
    size_t stride;
};
int launch_gms(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches, int n_direct,
               const float *d_kp1, int nq, const float *d_kp2, int nt, int width1, int height1, int width2, int height2, int use_scale,
               int use_rotation, int rule, mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_n_inliers, GmsWork *work, hipStream_t s);

// Sub-pixel refinement (subpix.hip) of match lists (d_matches [batch][match_stride], nullptr = match i joins keypoint i of both lists;
// d_n_matches [batch] or nullptr = n_direct for every list; d_kp1 [batch][nq][2], d_kp2 [batch][nt][2]; d_size1 / d_size2 [batch][nq] /
// [batch][nt] or nullptr; 8-bit images as [batch] planes with a row step and a batch stride in bytes).  max_side: the largest template side
// LDS is provisioned for (0 = 255).  One kernel launch on s, no upload, no synchronisation.  *work (optional) receives the workspace view
// res [batch][8] = {refined, status, dropped by the border / side / coordinate rule, largest side used, n_out, inliers}.
struct SubpixWork {
    const int32_t *res;
};
int launch_subpix(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches, int n_direct,
                  const float *d_kp1, int nq, const float *d_kp2, int nt, const float *d_size1, const float *d_size2, const uint8_t *d_img1,
                  int width1, int height1, size_t step1, size_t bstride1, const uint8_t *d_img2, int width2, int height2, size_t step2,
                  size_t bstride2, int max_side, int rule, mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_status, float *d_kp2_out,
                  uint8_t *d_inlier, SubpixWork *work, hipStream_t s);

// cornerSubPix refinement of each image on its own (subpix_separate.hip): the arguments of launch_subpix without max_side, plus d_kp1_out
// ([batch][nq][2] or nullptr) and d_iters ([batch][match_stride][2] loop passes per match and image, or nullptr).  Two kernel launches on s
// (the per-list windows, the refinement), no upload (subpix_separate_init, called by mlpl_ctx_create, puts the eight mask profiles into
// WS_SUBPIX_SEP_MASK), no synchronisation.  *work (optional)
// receives res [batch][8] = {refined, status, w1, w2, points dropped by the coordinate rule, points reset by the "too far" rule, n_out, inliers}.
int subpix_separate_init(mlpl_ctx *ctx);
int launch_subpix_separate(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches, int n_direct,
                           const float *d_kp1, int nq, const float *d_kp2, int nt, const float *d_size1, const float *d_size2,
                           const uint8_t *d_img1, int width1, int height1, size_t step1, size_t bstride1, const uint8_t *d_img2, int width2,
                           int height2, size_t step2, size_t bstride2, int rule, mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_status,
                           float *d_kp1_out, float *d_kp2_out, uint8_t *d_inlier, int32_t *d_iters, SubpixWork *work, hipStream_t s);

// glibc srand()/rand() (TYPE_3 additive feedback generator: r[k+3] += r[k] over a ring of 31 words, output r >> 1, the first 310
// outputs discarded), produced 31 values at a time: one unrolled pass over the ring has no index wrap-around and three independent
// dependency chains.  After seeding the generator is block-aligned (310 = 10 * 31), so block k holds outputs 31 k .. 31 k + 30.
struct GlibcRand {
    uint32_t r[31];
    int32_t out[31];
    int pos;
    void refill() {
#pragma unroll
        for (int k = 0; k < 28; ++k) {
            r[k + 3] += r[k];
            out[k] = (int32_t)(r[k + 3] >> 1);
        }
        for (int k = 28; k < 31; ++k) {
            r[k - 28] += r[k];
            out[k] = (int32_t)(r[k - 28] >> 1);
        }
        pos = 0;
    }
    void seed(unsigned s) {
        if (s == 0) s = 1;
        int32_t t[31];
        t[0] = (int32_t)s;
        for (int i = 1; i < 31; ++i) {
            const long hi = t[i - 1] / 127773, lo = t[i - 1] % 127773;
            long w = 16807 * lo - 2836 * hi;
            if (w < 0) w += 2147483647;
            t[i] = (int32_t)w;
        }
        for (int i = 0; i < 31; ++i) r[i] = (uint32_t)t[i];
        for (int i = 0; i < 10; ++i) refill();
        pos = 31;
    }
    int next() {
        if (pos == 31) refill();
        return out[pos++];
    }
};

}  // namespace mlpl
