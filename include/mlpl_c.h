/*
 * mlpl_c.h -- C ABI of the MI355X-native (gfx950) descriptor-matching + robust-pose hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  The reference
 * (josefmaierfl/matchinglib_poselib) has no FFI of its own for this path -- the path sits behind exported
 * C++ functions -- so each entry point below names the reference code it replaces.  Paths are relative to
 * /root/reference/matchinglib_poselib/source/ (M/ = matchinglib/, P/ = poselib/).
 *
 * Conventions
 *   - return value: 0 = ok, negative = error.  Codes -1..-4 keep the meaning of the reference's getMatches
 *     (M/source/matchers.cpp:109-114); MLPL_E_* below are this library's own.
 *   - no exceptions, no exit(), no stdout.  mlpl_last_error() returns a thread-local message.
 *   - the caller owns every buffer; outputs are caller-allocated.
 *   - `*_dev` entry points take DEVICE pointers plus a hipStream_t (as void*; NULL = HIP's null stream, use
 *     mlpl_ctx_stream() for the context's own), enqueue work and return without synchronising; the plain
 *     entry points take HOST pointers, copy in/out on the context's stream and synchronise.
 *   - a context (mlpl_ctx) owns the device workspace and a private stream; use one per host thread.
 *   - there is NO CPU fallback: every compute entry point fails with MLPL_E_NO_DEVICE when no gfx950
 *     device is usable.
 */
#ifndef MLPL_C_H
#define MLPL_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLPL_OK 0
#define MLPL_E_BAD_INPUT (-1)     /* getMatches: "Wrong input data"        (matchers.cpp:110) */
#define MLPL_E_UNSUPPORTED (-2)   /* getMatches: "Matcher not supported"   (matchers.cpp:111) */
#define MLPL_E_FAILED (-3)        /* getMatches: "Matching algorithm failed" / < 2 matches (matchers.cpp:112,709-713) */
#define MLPL_E_FEW_KEYPOINTS (-4) /* getMatches: "Too less keypoits"       (matchers.cpp:113,123-127) */
#define MLPL_E_NO_DEVICE (-100)
#define MLPL_E_HIP (-101)
#define MLPL_E_NOMEM (-102)
#define MLPL_E_INTERNAL (-103)    /* an internal capacity limit was hit: NOT an estimator outcome (in/out states are left untouched) */

/* cv::DMatch layout {int queryIdx; int trainIdx; int imgIdx; float distance;} -- 16 bytes. */
typedef struct mlpl_dmatch {
    int32_t queryIdx;
    int32_t trainIdx;
    int32_t imgIdx;
    float distance;
} mlpl_dmatch;

typedef struct mlpl_ctx mlpl_ctx;

/* ---- context ------------------------------------------------------------------------------------------ */
int mlpl_ctx_create(int device_ordinal, mlpl_ctx **out);
void mlpl_ctx_destroy(mlpl_ctx *ctx);
const char *mlpl_last_error(void);
const char *mlpl_version(void);
/* Number of visible HIP devices (0 when none); does not create a context. */
int mlpl_device_count(void);
/* The context's private stream (hipStream_t) and device ordinal. */
void *mlpl_ctx_stream(mlpl_ctx *ctx);
int mlpl_ctx_device(mlpl_ctx *ctx);
int mlpl_ctx_synchronize(mlpl_ctx *ctx);

/* Tuning knobs (performance only; "solver_polish", below, is the one numerical option):
 *   Hamming: "hamming_variant" 3 = fp4 matrix-core kernels (default; descriptors above 64 bytes fall back to 0), 0 = LDS-tiled VALU
 *     kernel, 1 = scalar-operand VALU kernel, 2 = one-wave-per-block VALU kernel; "hamming_mfma_lds" 1 (default) = LDS-ring kernel for
 *     32-byte descriptors, 0 = register-prefetch kernel, 2 = dynamic train splits; "hamming_mfma_weighted" (default 1) = age-aware split
 *     sizes; "hamming_mfma_prio" 0 | 1 (rotating wave priorities, diagnostics) | 3 (wave-uniform skip of the running top-2 update, 8-wave
 *     workgroups only: measured slower, round 6); "hamming_mfma_blocks_per_cu" and "hamming_mfma_qt" (query tiles per wave,
 *     0 = automatic) size the matrix-core grid; "hamming_qpl" queries per lane 1|2 and "hamming_blocks_per_cu" size the VALU grids;
 *     "hamming_stamps" 1 = per-wave / per-workgroup clock stamps (mlpl_debug_hamming_stamps), 2 = one clock record per launch
 *       (mlpl_debug_hamming_clock).  "hamming_train01" 1 = {0, +1} instead of +-1 train fragments in the matrix-core Hamming kernel
 *       (same results; see knn_hamming_mfma.hip; measured no faster, default 0).  "hamming_merge_emit" 1 = with one image pair per call the
 *       merge kernel writes the DMatch rows itself (no ratio_write launch; measured no faster, default 0; TEST-ONLY: its chained look-back
 *       assumes that the whole merge grid is resident, which other streams on the same device can break).
 *       "hamming_split_rows" 0 (default) | 8192 | 4096 = cap on the train rows one workgroup scans (4096 = rounds 1-4: every 8192-row train
 *       set was cut in two even with the chip full); "hamming_mfma_waves" 0 (automatic) | 4 | 8 | 16 waves per workgroup and
 *       "hamming_mfma_prefetch" 0 | 2 | 4 | 6 tiles of prefetch distance in the LDS-ring kernel.  They do not combine: waves 16 beats a
 *       prefetch of 4 or 6, which beats "hamming_mfma_prio"; prefetch and prio 3 exist with 8-wave workgroups only and are ignored elsewhere.
 *       "hamming_expand_fine" (default 1) = small launches expand the train set with one thread per (tile, K-step, lane).
 *       "hamming_expand_inkernel" 1 = the eight-wave LDS-ring kernel reads the raw 32-byte train rows and expands each tile in its own
 *       workgroup (no expansion launch, no expanded copy of the train set in the workspace); 0 = the separate expansion kernel.
 *       "hamming_block_top2" 4 (default) | 0 = block size of the running top-2 update of that in-kernel-expansion kernel: 0 folds every
 *       candidate into a lane's running pair, 4 folds only the maxima of aligned groups of four train rows and re-scores the rows of the one
 *       group that holds a query's best row from the raw descriptors in the epilogue (same results bit for bit, measured faster; ignored by
 *       every other kernel, mlpl_debug_last_hamming_top2 reports what ran).
 *       "hamming_mfma_shape" 32 | 16 = matrix-core instruction of that kernel with the block update of four (and without the stamps trace of
 *       "hamming_stamps" 1): v_mfma_f32_32x32x64_f8f6f4, or v_mfma_f32_16x16x128_f8f6f4 with two chains of two per 16 queries and one
 *       re-base of the running pairs per two tiles (same results bit for bit; ignored by every other kernel,
 *       mlpl_debug_last_hamming_shape reports what ran).
 *   L2: "l2_mfma_waves" 0|4|8 and "l2_mfma_blocks_per_cu" shape the int8 matrix-core kernel of the forced mode (see mlpl_set_l2_path);
 *     "l2_float_mfma" 0|1|2 decides when the fp16 candidate path serves non-integer float descriptors (mlpl_set_l2_path, mode 0);
 *     "l2_fold_counts" (default 1) = mlpl_match_l2_dev's fold over the train splits evaluates the ratio predicate and writes the pass
 *     counts itself (four launches), 0 = separate merge and counting launches (five; A/B and tests; same results).
 *   VFC: "vfc_store_u" 1 = the filter's kernel keeps the m x n kernel matrix U (128 bytes per match) in the workspace, 0 (default) = it
 *     recomputes U in both passes of an EM iteration.  Same bits either way; the default is not backed by a measurement yet.
 *   RANSAC: "ransac_device_draw" (default 1) = large passes draw their samples on the device (mlpl_debug_ransac_draw); "ransac_chunk" hypotheses per device pass (0 = 32768 = the maximum; the sequential best/niters rule is replayed across
 *     passes); "ransac_lazy_sums" (default 1) = the passes count inliers without the division and compute error sums only for the
 *     models that can still win, 0 = sums for every model; "ransac_f32_filter" (default 1) = the counting kernels decide in packed single
 *     precision outside a rigorous error band and in fp64 inside it (same counts), 0 = fp64 only; "ransac_overlap" (default 1) = the
 *     root kernels of a large pass run on helper streams beside the elimination kernels; "ransac_host_table" 1 = build the
 *     iteration-bound table T[g] on the host for every call (default 0: the device evaluates the few bounds it needs and the host
 *     verifies exactly those against its libm, falling back to the table when one differs); "ransac_event_cap" (tests) = capacity of
 *     the record-event list of the replay kernels.
 *   Sequential estimators (round 4): "eig_inverse_iteration" (default 1) = the one eigenvector the re-weighted 9 x 9 fits need (USAC
 *     REF_WEIGHTS, robustEssentialRefine) by inverse iteration, the Jacobi decomposition as fallback, 0 = Jacobi always;
 *     "usac_lo_warm_start" / "arrsac_refine_warm_start" (default 1) = a chain's eigen-iterations start from its previous fit;
 *     "usac_sprt_fast", "usac_lo_stepwise" (tests).  Batches of them: "hub_lanes" (cohorts of runs in flight, 1..8; 0 = the estimator's own choice: six for USAC with REF_WEIGHTS, four otherwise),
 *     "usac_lo5_fused_fit" (default 1: a fit of the 5-point refinements' chains -- solve, roots, choice -- is one launch, 0 = three),
 *     "usac_first_batch" (samples in a run's first speculative batch, 1..128; 0 = default = as later batches: up to 128),
 *     "hub_cohort" (runs per cohort, 0 = 128), "hub_workers" (worker threads per cohort, 0 = 16: the runs are fibers on them),
 *     "hub_blocking_sync" (default 1: a cohort's thread sleeps at the end of a round instead of spinning), "pair_batch" /
 *     "pair_batch_seq" (image pairs per internal batch of mlpl_pair_pose_batch_dev, 0 = 256 / of its USAC and ARRSAC forms, 0 = 512).
 *     Hamming: "hamming_fused_merge" (default 1) = the LDS-ring kernel folds its train splits, evaluates the ratio predicate and counts
 *     itself, 0 = separate merge launch; RANSAC: "ransac_count_mpl" 1|2 models per lane of the counting kernel (A/B, default 2);
 *     "ransac_count_threads" 256 (default since round 6: 4-wave workgroups at 96 VGPRs, five per CU) | 512; "ransac_count_tiles" 2 (default) | 1
 *     tiles of 512 correspondences per counting workgroup; "ransac_count_wpe" 5 (default) | 6 waves per SIMD the 256-thread counting
 *     kernel's registers are cut for; "ransac_count_defer" (default 1) = the counting kernel decides its undecided evaluations in a
 *     workgroup-wide queue after its loop, 0 = on the spot (same counts).
 *   "solver_polish" (default 1) = every 5-point solution is finished by <= 4 Gauss-Newton steps on the ten cubic constraints (a step is
 *     kept only while the residual falls).  It is the accuracy safeguard of THIS solver, not a departure from the reference: the device's
 *     elimination (like the CPU code's, five-point.cpp:366-471, but on other samples) is ill conditioned on ~0.4 % of minimal samples and its
 *     plain result is then off by up to 4e-3.  Measured against the CPU path on 43 760 models (tools/polish_default_ab.py, round 6): with the
 *     safeguard 158 models differ by more than 1e-8 -- every one a sample on which the CPU path's OWN model violates the essential-matrix
 *     constraints; without it 318 differ, half of them because the device's model is the inaccurate one, and ten parity tests against the
 *     oracle fail (USAC decisions part).  RANSAC runs: identical to the CPU path on 126 of 126 seeds either way.  0 = the plain elimination +
 *     root path, kept for A/B (mlpl_set_option(ctx, "solver_polish", 0) or MLPL_OPTIONS=solver_polish=0). */
int mlpl_set_option(mlpl_ctx *ctx, const char *name, int value);
/* The current value of a tuning knob: every name mlpl_set_option takes.  Returns 0, MLPL_E_BAD_INPUT for a name it does not know. */
int mlpl_get_option(mlpl_ctx *ctx, const char *name, int *value);
/* The option table without a context (and without a device): the name and the default of option `index`, 0 <= index < the number of
 * options, in the table's order.  Returns 0, MLPL_E_BAD_INPUT past either end or for a NULL output; walk it from 0 until it refuses. */
int mlpl_option_info(int index, const char **name, int *default_value);
/* 1 if mlpl_set_option would take `value` for `name`, 0 if it would refuse it (the same check); MLPL_E_BAD_INPUT for an unknown or
 * NULL name. */
int mlpl_option_accepts(const char *name, int value);

/* ---- in-library kernel timing (for roofline accounting) ------------------------------------------------------
 * When enabled, the launches of the dominant kernel of each path are bracketed with hipEvents on the stream
 * they run on.  mlpl_profile_read() synchronises those events and returns the summed duration and the
 * launch count since the last reset.  kernel_id: 0 = Hamming partial top-2 (matrix-core or VALU kernel), 1 = knn_l2 (exact or
 * MFMA), 2 = 5-point solver, 3 = Sampson scoring, 4 = recover_pose, 6 = bundle adjustment, 7 = multi-camera bundle adjustment.  mlpl_profile_enable(ctx, N): 0 = off, 1 = every launch,
 * N > 1 = every Nth launch (sampling: the two event records cost ~10 us of stream time per bracketed launch). */
#define MLPL_PROF_KNN_HAMMING 0
#define MLPL_PROF_KNN_L2 1
#define MLPL_PROF_SOLVE_5PT 2
#define MLPL_PROF_SCORE 3
#define MLPL_PROF_RECOVER_POSE 4
#define MLPL_PROF_COUNT 5         /* the inlier-counting kernel of a RANSAC pass alone (MLPL_PROF_SCORE brackets the whole scoring pass: it, the candidate selection and the candidates' error sums) */
#define MLPL_PROF_BUNDLE_ADJUST 6 /* the bundle-adjustment kernel (mlpl_refine_stereo_ba*): one launch per call */
#define MLPL_PROF_BA_MULTICAM 7  /* the multi-camera bundle-adjustment kernel (mlpl_refine_multicam_ba*): one launch per call */
#define MLPL_PROF_NUM 8
int mlpl_profile_enable(mlpl_ctx *ctx, int on);
int mlpl_profile_reset(mlpl_ctx *ctx);
int mlpl_profile_read(mlpl_ctx *ctx, int kernel_id, double *total_ms, int *launches);

/* ---- brute-force k-NN (k = 1 or 2) ---------------------------------------------------------------------
 * Replaces cvflann::Index<HammingLUT>(dataset, LinearIndexParams()).knnSearch(query, indices, dists, nn, ...)
 * at M/source/matchers.cpp:567-588 (CV_8U) and cvflann::Index<L2<float>> at :634-664 (CV_32F).
 * q = descriptors1 (query, nq rows), t = descriptors2 (train, nt rows).  Strides are in BYTES for the
 * Hamming entry and in ELEMENTS for the float entry.  idx/dist are nq*k row-major.
 * Result = the k lexicographically smallest (distance, trainIdx) pairs, ascending (cvflann
 * KNNUniqueResultSet semantics).  Hamming distances are exact integers; L2 is SQUARED, summed in fp32 in
 * the reference's order (4 differences per step), so both are bit-exact against the CPU path.
 * Requires nt >= k, nbytes in [1,256] / dim in [1,1024].
 */
int mlpl_knn2_hamming(mlpl_ctx *ctx, const uint8_t *q, int nq, size_t q_stride, const uint8_t *t, int nt,
                      size_t t_stride, int nbytes, int k, int32_t *idx, int32_t *dist);
int mlpl_knn2_l2sq_f32(mlpl_ctx *ctx, const float *q, int nq, size_t q_stride, const float *t, int nt,
                       size_t t_stride, int dim, int k, int32_t *idx, float *dist);

/* Device-pointer, batched forms.  `batch` independent problems of identical shape; problem b reads
 * q + b*q_batch_stride (bytes for Hamming / elements for float), writes idx + b*nq*k etc. */
int mlpl_knn2_hamming_dev(mlpl_ctx *ctx, const uint8_t *d_q, int nq, size_t q_stride, size_t q_batch_stride,
                          const uint8_t *d_t, int nt, size_t t_stride, size_t t_batch_stride, int nbytes, int k,
                          int batch, int32_t *d_idx, int32_t *d_dist, void *stream);
int mlpl_knn2_l2sq_f32_dev(mlpl_ctx *ctx, const float *d_q, int nq, size_t q_stride, size_t q_batch_stride,
                           const float *d_t, int nt, size_t t_stride, size_t t_batch_stride, int dim, int k,
                           int batch, int32_t *d_idx, float *d_dist, void *stream);
/* L2 path selector for the *_dev/host float entries (results are identical on every path):
 *   0 = auto: int8 matrix-core distance-GEMM when every element is an integer in [0,255] (OpenCV SIFT layout); otherwise fp16
 *       matrix-core candidate passes + exact fp32 re-rank (dim <= 128; option "l2_float_mfma": 1 (default) = once the previous call of
 *       this context saw non-integer data -- the first such call runs the exact kernel --, 2 = enqueued on every call, 0 = never), or the
 *       exact fp32 VALU kernel in cvflann's summation order;
 *   1 = force the exact fp32 VALU kernel;
 *   2 = force the int8 matrix-core path (MLPL_E_BAD_INPUT if the data are not integer-valued 0..255);
 *   3 = force the fp16 candidate path + exact re-rank (MLPL_E_BAD_INPUT if dim > 128 or a row is outside its range: non-finite,
 *       |x| > 1e15, or largest element below 1e-12). */
int mlpl_set_l2_path(mlpl_ctx *ctx, int mode);

/* ---- ratio test + DMatch emission ----------------------------------------------------------------------
 * Replaces the loops at M/source/matchers.cpp:601-625 (int distances) and :677-701 (float distances):
 * k==2: keep q iff (float)d0 < ratio*(float)d1 (reference ratio = 0.75f); k==1: keep every q.
 * Matches are emitted in ascending queryIdx, imgIdx = -1, distance = (float)d0.
 * out must hold nq entries (per batch item); *n_out receives the count.
 */
int mlpl_ratio_compact_i32(mlpl_ctx *ctx, const int32_t *idx, const int32_t *dist, int nq, int k, float ratio,
                           mlpl_dmatch *out, int *n_out);
int mlpl_ratio_compact_f32(mlpl_ctx *ctx, const int32_t *idx, const float *dist, int nq, int k, float ratio,
                           mlpl_dmatch *out, int *n_out);
int mlpl_ratio_compact_i32_dev(mlpl_ctx *ctx, const int32_t *d_idx, const int32_t *d_dist, int nq, int k,
                               int batch, float ratio, mlpl_dmatch *d_out, int32_t *d_n_out, void *stream);
int mlpl_ratio_compact_f32_dev(mlpl_ctx *ctx, const int32_t *d_idx, const float *d_dist, int nq, int k,
                               int batch, float ratio, mlpl_dmatch *d_out, int32_t *d_n_out, void *stream);

/* ---- getMatches(..., "LINEAR", ...) in one call ---------------------------------------------------------
 * Replaces the whole LINEAR branch, M/source/matchers.cpp:115-135 + 525-714.  desc_type: 0 = CV_8U
 * (cols bytes per row), 5 = CV_32F (cols floats per row); step1/step2 = cv::Mat::step in bytes.
 * Returns the reference's codes (0, -1, -3, -4).  out must hold rows1 entries.
 */
int mlpl_get_matches_linear(mlpl_ctx *ctx, int n_keypoints1, int n_keypoints2, const void *desc1, int rows1,
                            size_t step1, const void *desc2, int rows2, size_t step2, int cols, int desc_type,
                            int ratio_test, mlpl_dmatch *out, int *n_out);
/* getMatches(..., "BRUTEFORCENMS", ...): M/source/matchers.cpp:476-519 -> nmslibMatching<dist_t>(..., "seq_search",
 * "bit_hamming" | "l2") (M/include/nmslib/nmslib_matchers.h:159-424) on the vendored NMSLIB, including its quirks:
 * CV_8U rows are compared WITHOUT their last two bytes (one for odd widths; the wrapper omits the length word that
 * SpaceBitHamming::HiddenDistance strips), CV_32F uses the TRUE L2 distance sqrt(sum) summed in NMSLIB's 4-lane order and
 * the ratio test runs on those, K = 2 always, without ratio test ties emit the larger train id, and there is no
 * minimum-match check.  desc_type 0 = CV_8U, 5 = CV_32F (CV_64F: MLPL_E_UNSUPPORTED). */
int mlpl_get_matches_bruteforce_nms(mlpl_ctx *ctx, int n_keypoints1, int n_keypoints2, const void *desc1, int rows1,
                                    size_t step1, const void *desc2, int rows2, size_t step2, int cols, int desc_type,
                                    int ratio_test, mlpl_dmatch *out, int *n_out);
/* Device-resident, batched: knn + ratio + compaction, nothing leaves the device. */
int mlpl_match_hamming_dev(mlpl_ctx *ctx, const uint8_t *d_q, int nq, size_t q_stride, size_t q_batch_stride,
                           const uint8_t *d_t, int nt, size_t t_stride, size_t t_batch_stride, int nbytes,
                           int ratio_test, float ratio, int batch, int32_t *d_idx, int32_t *d_dist,
                           mlpl_dmatch *d_out, int32_t *d_n_out, void *stream);

/* The same for CV_32F descriptors: the float half of the LINEAR branch, M/source/matchers.cpp:632-707 -- cvflann::Index<L2<float>>
 * knnSearch (:634-664: squared L2 in cvflann's summation order) and the ratio loop (:677-701: keep q iff d0 < 0.75f * d1; rows in
 * ascending queryIdx, imgIdx = -1, distance = d0).  Strides in ELEMENTS and argument limits as mlpl_knn2_l2sq_f32_dev (dim in [1,1024],
 * nt >= k, batch <= 65535); follows mlpl_set_l2_path and option "l2_float_mfma" exactly as that entry does.  Every output -- d_idx,
 * d_dist, d_out[0..n), d_n_out -- is bit-identical to mlpl_knn2_l2sq_f32_dev followed by mlpl_ratio_compact_f32_dev on every L2 path;
 * wherever the path ends in a fold over train splits (exact, int8, auto) that fold evaluates the predicate and counts the passes
 * itself (option "l2_fold_counts"), so the call is four launches instead of five.  nq == 0: OK, d_n_out[b] = 0. */
int mlpl_match_l2_dev(mlpl_ctx *ctx, const float *d_q, int nq, size_t q_stride, size_t q_batch_stride,
                      const float *d_t, int nt, size_t t_stride, size_t t_batch_stride, int dim,
                      int ratio_test, float ratio, int batch, int32_t *d_idx, float *d_dist,
                      mlpl_dmatch *d_out, int32_t *d_n_out, void *stream);

/* ---- VFC match filter: getMatches' VFCrefine ----------------------------------------------------------------
 * matchinglib::filterWithVFC (M/source/vfcMatches.cpp:63-100) with VFC's default method, SparseVFC (M/source/vfc.cpp; the other two
 * methods are unreachable in the reference and not built), on the matched points x1[i] -> x2[i] (n x 2 floats, pixels, host).
 * normalize() is reproduced bit for bit; the control points are drawn from the first 48 values of glibc's srand(seed) / rand() (the
 * reference draws from wherever the process-wide stream stands; an unseeded process starts at seed 1); everything from the kernel matrices on
 * -- posteriors, the m x m system (LU, partial pivoting; a pivot below 100 DBL_EPSILON gives C = 0, cv::solve's rule for doubles), exp and
 * log -- is float64 with the reference's float constants widened, because the system is numerically singular (condition 1e15 - 1e16) and
 * the reference's own float rounding decides nothing reproducible.  The contract is the KEPT SET: equal to the reference's on separable
 * data, equal to the float64 restatement (tests/vfc_oracle.py) otherwise.  One workgroup, all (at most 50) EM iterations in one launch.
 * keep: n bytes (1 = kept), *n_keep their number; P: NULL or n doubles, the inlier posteriors of the last iteration (diagnostic);
 * info (optional) = {control points, iterations run, 1 if normalize() refused (a scale below 0.1: everything is kept), solves that hit the
 * singular rule}.  Returns filterWithVFC's value: 0; -1 (n < 5: nothing ran, keep all 1 and *n_keep = n); -2 (fewer than 10 % kept; keep
 * and *n_keep are still written).  Errors: MLPL_E_INTERNAL and below (never -1 / -2).  n <= 65535. */
int mlpl_vfc_filter(mlpl_ctx *ctx, const float *x1, const float *x2, int n, uint32_t seed, uint8_t *keep, int *n_keep, double *P /* NULL or n */,
                    int info[4]);
/* The same for a batch of match lists, device-resident and non-synchronising (one launch and a 192-byte-per-problem upload on `stream`):
 * problem b filters d_matches + b * match_stride (d_n_matches[b] <= match_stride entries: the output of mlpl_match_hamming_dev /
 * mlpl_match_l2_dev) on x1 = d_kp1[b][queryIdx], x2 = d_kp2[b][trainIdx] ([batch][nq][2] / [batch][nt][2] floats, as
 * mlpl_gather_match_points_dev reads them; indices outside are clamped).  seeds: HOST, one per problem, or NULL (all 1).  The kept matches
 * are compacted in order into d_out + b * match_stride (the layout of the pair entries' d_matches_out; d_out must not be d_matches),
 * d_n_out[b] their number, d_status[b] = 0 / -1 / -2 as above.  status -1 (0 <= n < 5) passes the list through.  getmatches_rule != 0
 * applies M/source/matchers.cpp:726-731: the list is passed through unchanged unless status is 0 and (kept > 8 or n < 24).
 * Every problem's list, count and status are bit-identical to what mlpl_vfc_filter yields for it with the same seed (the same kernel,
 * every sum in an order that depends on the problem alone).  Option "vfc_store_u": see mlpl_set_option. */
int mlpl_vfc_filter_matches_dev(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches,
                                const float *d_kp1, int nq, const float *d_kp2, int nt, const uint32_t *seeds /* host */, int getmatches_rule,
                                mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_status, void *stream);

/* ---- GMS match filter: matchinglib::filterMatchesGMS --------------------------------------------------------
 * Grid-based motion statistics (M/source/gms.cpp over M/thirdparty/gms-1.0/src/MatchGMS.cpp), the filter getCorrespondences runs behind
 * getMatches (M/source/correspondences.cpp:378-397).  Integer voting on a 20 x 20 left grid and a right grid of 20, 10, 14, 28 or 40 cells a
 * side (scale levels 0-4; only level 0 without use_scale), four half-cell-shifted grid types per run, eight rotation types of the 3 x 3
 * neighbourhood with use_rotation (only type 0 without); the first run with the most inliers wins (scale level outer, rotation type inner,
 * strict >).  Reproduced bit for bit, the reference's quirks included: coordinates are normalised with a float reciprocal and one float
 * multiply, the cell is floorf of a separately rounded multiply (and + 0.5f); a negative left x is not checked and may alias into the
 * row before; the right cell is computed at grid type 1 only and not bounds-checked (x = Wr aliases into the next row); a match whose left
 * or right index is negative at a grid type is dropped for the REST of the run (it keeps an inlier flag it earned before); the cell test
 * score < 6 sqrt(thresh / numPair) is evaluated in double.
 * Deviations: where the reference reads or writes out of bounds or converts an unrepresentable float to int, the match is dropped like a
 * negative index and counted: a right index at or above Wr * Hr, a coordinate that is not finite or whose floor does not fit an int.  Cell
 * indices are formed in 64 bits (the reference's int sum can overflow).  A non-positive image size is MLPL_E_BAD_INPUT.
 * kp1 / kp2: n1 / n2 rows of (x, y) floats; matches: n DMatch rows; all HOST pointers.  keep: n bytes of 0 / 1, *n_keep the best run's count
 * (0 = "nothing assigned": keep is all 0).  info (optional) = {winning scale level or -1, winning rotation type or -1, matches dropped by
 * the out-of-bounds rule in the winning run, 0}.  Returns 0, or MLPL_E_BAD_INPUT (n > 65535, a non-positive size, a queryIdx / trainIdx
 * outside the keypoint arrays) or another MLPL_E_* code.  n = 0 returns 0 with *n_keep = 0. */
int mlpl_gms_filter(mlpl_ctx *ctx, const float *kp1, int n1, int width1, int height1, const float *kp2, int n2, int width2, int height2,
                    const mlpl_dmatch *matches, int n, int use_scale, int use_rotation, uint8_t *keep, int *n_keep, int info[4]);
/* The same for a batch of match lists, device-resident and non-synchronising (one launch on `stream`, no upload): the layouts of
 * mlpl_vfc_filter_matches_dev -- problem b filters d_matches + b * match_stride (d_n_matches[b] <= match_stride entries: the output of
 * mlpl_match_hamming_dev / mlpl_match_l2_dev) on d_kp1[b][queryIdx], d_kp2[b][trainIdx] ([batch][nq][2] / [batch][nt][2] floats; indices
 * outside are clamped).  The kept matches are compacted in order into d_out + b * match_stride (d_out must not be d_matches), d_n_out[b]
 * their number, d_n_inliers[b] the filter's count.  min_final_rule != 0 applies correspondences.cpp:388-397: the list passes through
 * unchanged unless the count is at least MIN_FINAL_MATCHES (2).  Every list, count and flag is bit-identical to mlpl_gms_filter on the same
 * problem (the same kernel).  batch, match_stride in [1, 65535]. */
int mlpl_gms_filter_matches_dev(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches,
                                const float *d_kp1, int nq, const float *d_kp2, int nt, int width1, int height1, int width2, int height2,
                                int use_scale, int use_rotation, int min_final_rule, mlpl_dmatch *d_out, int32_t *d_n_out,
                                int32_t *d_n_inliers, void *stream);

/* ---- sub-pixel refinement: matchinglib::getSubPixMatches ------------------------------------------------------
 * Template matching around matched keypoints (M/source/matchers.cpp:1085-1297), the step getCorrespondences runs with subPixRefine == 1
 * behind getMatches and the filters (M/source/correspondences.cpp:444-494).  Keypoint lists 1 and 2 are matched index by index.  Match i:
 *  1. side fs = (int)(size1 > size2 ? size1 : size2) + 6, at least 18 (a NaN or negative size ends here), minus 1 when even; d1 = (fs - 1) / 2.
 *  2. template: fs x fs pixels of image 1 at (cvRound(x1) - d1, cvRound(y1) - d1); window: (fs + 10)^2 pixels of image 2 at
 *     (cvRound(x2) - d1 - 5, cvRound(y2) - d1 - 5); cvRound rounds half to even; pixels outside an image read as 0.
 *  3. R[v][u], u, v in 0..10 = sum over the template of (window[v + r][u + c] - template[r][c])^2 as an EXACT integer, then rounded to float32.
 *  4. (mx, my) = the first minimum of the float32 table in row-major order.
 *  5. inlier iff (mx - 5)^2 + (my - 5)^2 <= 16.
 *  6. an inlier's parabola fit in float32, every operation rounded on its own: nx = 2 (2 c - xn - xp), ny likewise; if both are non-zero,
 *     keypoint 2 = ((float)(window x + mx + d1) + (xp - xn) / nx, (float)(window y + my + d1) + (yp - yn) / ny) and the match counts as refined.
 *     Keypoint 1 and an outlier's keypoint 2 never change.
 *  7. *status = -1 if refined < n / 3 or refined < 2 (MIN_FINAL_MATCHES), else 0; mask and keypoints are written in both cases.
 * Deviations:
 *  - The reference's table comes from cv::matchTemplate, which forms the cross term in float32 (OpenCV is not in this tree; its exact
 *    arithmetic is not reproduced).  The table here is the exact integer, bit for bit the restatement tests/subpix_oracle.py.  Against the
 *    reference a near-tie may pick a neighbouring placement and offsets may differ by about 1e-3 px; the difference is unmeasured.
 *  - Dropped matches (mask 0, keypoint unchanged, counted in info under the first rule that applies, in this order): a coordinate that is
 *    not finite or whose rounded value does not fit an int; a side above 255 (it bounds the LDS footprint and keeps the sum in 32 bits);
 *    a template or window that leaves the 100-pixel border the reference pads the images with (it asserts in cv::Mat::operator() there).
 *  - Images are 8-bit single channel; anything else is MLPL_E_BAD_INPUT at this level.
 * img1 / img2: HOST pointers, `step` bytes from row to row (>= width).  kp1 [n][2], kp2 [n][2] (in / out), size1 / size2 [n] or NULL (all 0:
 * side 17), inlier [n] bytes of 0 / 1.  info (optional) = {dropped by the border rule, by the side rule, by the coordinate rule, largest
 * side used (0 when every match was dropped)}.  Returns MLPL_OK, MLPL_E_BAD_INPUT (n > 65535, a non-positive size, step < width) or
 * another MLPL_E_* code; the reference's 0 / -1 goes to *status.  n = 0 returns MLPL_OK with *status = -1. */
int mlpl_subpix_matches(mlpl_ctx *ctx, const uint8_t *img1, int width1, int height1, size_t step1, const uint8_t *img2, int width2, int height2,
                        size_t step2, const float *kp1, float *kp2, const float *size1, const float *size2, int n, uint8_t *inlier,
                        int *n_refined, int *status, int info[4]);
/* Step 1 on the host: the template side for a pair of keypoint sizes, 17 ... 255, or 0 when the side rule drops the match. */
int mlpl_subpix_template_side(float size1, float size2);
/* The same for a batch of match lists, device-resident and non-synchronising (one kernel launch on `stream`, no upload): the layouts of
 * mlpl_gms_filter_matches_dev -- problem b refines d_matches + b * match_stride (d_n_matches[b] <= match_stride entries) on
 * d_kp1[b][queryIdx], d_kp2[b][trainIdx] ([batch][nq][2] / [batch][nt][2] floats; indices outside are clamped), sizes d_size1[b][queryIdx],
 * d_size2[b][trainIdx] (or NULL), images d_img1 + b * batch_stride1 and d_img2 + b * batch_stride2 (bytes; row steps step1 / step2).
 * max_side: the largest template side LDS is provisioned for, 0 = 255; a match with a larger side is dropped by the side rule (pass the
 * largest mlpl_subpix_template_side of the data, or 17 with NULL sizes, for more workgroups per compute unit; with 0 every per-match
 * result is bit-identical to mlpl_subpix_matches on the same data: the same kernel).
 * d_kp2_out [batch][nt][2] (may be d_kp2) starts as a copy of d_kp2; then, as correspondences.cpp:480-483, every match writes its refined or
 * unchanged position to its train keypoint, and of several matches with one trainIdx the LAST in list order wins.  d_status[b] = step 7.
 * correspondences_rule == 0: the inliers are compacted in list order into d_out + b * match_stride (d_out must not be d_matches),
 * d_n_out[b] their number.  correspondences_rule != 0 applies correspondences.cpp:474-494: on status -1 the list and the keypoints pass
 * through unchanged; on status 0 the inliers are emitted in REVERSE list order (the reference's loop runs from the end).
 * d_inlier (optional) [batch][match_stride] bytes: the mask of step 5.  batch, match_stride in [1, 65535]. */
int mlpl_subpix_matches_dev(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches,
                            const float *d_kp1, int nq, const float *d_kp2, int nt, const float *d_size1, const float *d_size2,
                            const uint8_t *d_img1, int width1, int height1, size_t step1, size_t batch_stride1, const uint8_t *d_img2,
                            int width2, int height2, size_t step2, size_t batch_stride2, int max_side, int correspondences_rule,
                            mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_status, float *d_kp2_out, uint8_t *d_inlier, void *stream);

/* ---- sub-pixel refinement, each image on its own: matchinglib::getSubPixMatches_seperate_Imgs ------------------
 * cv::cornerSubPix on the matched keypoints of image 1 and of image 2 independently (M/source/matchers.cpp:1318-1391), the step
 * getCorrespondences runs with subPixRefine == 2 (M/source/correspondences.cpp:444-494): the variant for pairs with large rotation or scale
 * change, where a template of image 1 is not found in image 2.  OpenCV is not in this tree: the arithmetic of cv::cornerSubPix and
 * cv::getRectSubPix is RESTATED here from OpenCV 4.2's cornersubpix.cpp / samplers.cpp as remembered, and this text is the definition.  The
 * device result equals the restatement tests/subpix_separate_oracle.py bit for bit; the distance to a real OpenCV build is unmeasured.
 * Keypoint lists 1 and 2 are matched index by index.  Per call (one match list):
 *  1. window half-size per image, w1 and w2: m = the smallest keypoint size of that list that is > 0 (a NaN or non-positive size never
 *     compares true and is ignored; FLT_MAX when there is none or the size array is NULL), clamped to at most 20, then to at least 6;
 *     w = (int)ceilf(m / 2.f), so w is 3 ... 10, and every point of that image uses it.
 *  2. mask: g[i] = (float)exp(-(double)(y * y)) with float y = (float)(i - w) / w, i = 0 ... 2w; mask[i][j] = g[i] * g[j], a float32 product.
 *     The eight profiles are evaluated on the host in double by libm's exp, rounded to float and uploaded when the context is created.
 *  3. refinement of one point cT (float32 x, y) in an image of cols x rows: cI = cT, iter = 0, then repeat
 *     a. sampling: cx = cI.x - (float)(w + 1), ix = floor(cx), a = cx - (float)ix, the same in y for iy and b, all float32; the weights, every
 *        operation rounded to float32, a11 = (1-a)*(1-b), a12 = a*(1-b), a21 = (1-a)*b, a22 = a*b; for r, c in 0 ... 2w+2
 *        S[r][c] = ((P(iy+r, ix+c)*a11 + P(iy+r, ix+c+1)*a12) + P(iy+r+1, ix+c)*a21) + P(iy+r+1, ix+c+1)*a22 in float32, each product and
 *        each sum rounded on its own; P is the 8-bit image with row and column indices clamped to the image (edge replication).
 *     b. terms: for window element k = i*(2w+1) + j, i, j in 0 ... 2w, all in double: tgx = S[i+1][j+2] - S[i+1][j],
 *        tgy = S[i+2][j+1] - S[i][j+1], m = mask[i][j], gxx = (tgx*tgx)*m, gxy = (tgx*tgy)*m, gyy = (tgy*tgy)*m, px = j - w, py = i - w;
 *        the five terms are gxx, gxy, gyy, gxx*px + gxy*py, gxy*px + gyy*py.
 *     c. summation order (part of the contract: double addition is not associative): lane l = k mod 64 adds its terms in increasing k,
 *        starting from its first term; a lane without terms holds +0.0; the 64 lane sums are folded by v[l] = v[l] + v[l + s] for
 *        s = 32, 16, 8, 4, 2, 1 and the result is v[0] -- the halving tree of one wave.  Results: a, b, c, bb1, bb2.
 *     d. det = a*c - b*b; if fabs(det) <= DBL_EPSILON*DBL_EPSILON the loop ends and cI stays.
 *     e. scale = 1.0/det; nx = (float)(((double)cI.x + (c*scale)*bb1) - (b*scale)*bb2), ny = (float)(((double)cI.y - (b*scale)*bb1) +
 *        (a*scale)*bb2); err = (nx-cI.x)*(nx-cI.x) + (ny-cI.y)*(ny-cI.y) in float32, widened to double; cI = (nx, ny).
 *     f. if cI.x < 0 || cI.x >= cols || cI.y < 0 || cI.y >= rows the loop ends.
 *     g. the loop continues while ++iter < 40 && err > 1e-6 (TermCriteria(EPS + COUNT, 40, 0.001), squared).
 *     After the loop: if fabsf(cI.x - cT.x) > w || fabsf(cI.y - cT.y) > w the result is cT ("too far"), else cI.
 *  4. match i: d1 = the squared float32 distance between the old and the refined point 1 (dx*dx + dy*dy, each operation rounded), d2
 *     likewise for point 2.  d1 > 12 || d2 > 12: mask 0 and neither keypoint changes.  Otherwise mask 1, both keypoints take their refined
 *     positions and the match counts as refined.  A point that never moved is an inlier: a constant image refines nothing, every match is
 *     an inlier and the status is 0 (unlike mlpl_subpix_matches).
 *  5. *status = -1 if refined < n / 3 or refined < 2 (MIN_FINAL_MATCHES), else 0; mask and keypoints are written in both cases.
 * Deviations:
 *  - Sampling: OpenCV's in-image fast path factors the expression of 3a differently; the out-of-image path is the one restated.  Mask:
 *    OpenCV calls std::exp on a float; the double route rounded to float equals a correctly rounded expf, the reference's libm may not.
 *    Neither difference is measured.
 *  - A point with a coordinate that is not finite or does not fit an int is dropped: its match has mask 0, stays unchanged and the point
 *    is counted in info (the reference's behaviour there is undefined); the other point of the match is still iterated.
 *  - A non-finite nx or ny ends the loop and the result is cT.
 *  - Images are 8-bit single channel.  An image with cols < 2w + 5 or rows < 2w + 5 is MLPL_E_BAD_INPUT (OpenCV asserts there).
 * img1 / img2: HOST pointers, `step` bytes from row to row (>= width).  kp1, kp2 [n][2] (both in / out), size1 / size2 [n] or NULL, inlier [n]
 * bytes of 0 / 1, iters NULL or [n][2]: the value of step 3's `iter` when the loop of point 1 / point 2 of the match ended (the passes that
 * reached 3g; 0 for a dropped point) -- the sensitive witness that two implementations walk the same trajectory.  info (optional) = {w1, w2,
 * points dropped by the coordinate rule, points reset by the "too far" rule}.  Returns MLPL_OK, MLPL_E_BAD_INPUT (n > 65535, a non-positive
 * size, step < width, an image too small) or another MLPL_E_* code; the reference's 0 / -1 goes to *status.  n = 0 returns MLPL_OK with
 * *status = -1. */
int mlpl_subpix_separate(mlpl_ctx *ctx, const uint8_t *img1, int width1, int height1, size_t step1, const uint8_t *img2, int width2, int height2,
                         size_t step2, float *kp1, float *kp2, const float *size1, const float *size2, int n, uint8_t *inlier, int32_t *iters,
                         int *n_refined, int *status, int info[4]);
/* Step 1's clamp and ceil on the host: the window half-size, 3 ... 10, for the smallest positive keypoint size of a list (FLT_MAX or a
 * NaN: none, 10). */
int mlpl_subpix_separate_window(float min_size);
/* The same for a batch of match lists, device-resident and non-synchronising (two kernel launches on `stream`: the windows of every list,
 * then the refinement; no upload: the mask profiles are in the context): the layouts and the argument order of
 * mlpl_subpix_matches_dev without max_side and with d_kp1_out.  The windows of list b are step 1 over the sizes of that list's matched
 * keypoints, d_size1[b][queryIdx] and d_size2[b][trainIdx] (indices outside are clamped); the windows are only known on the device, so
 * images smaller than 25 x 25 are MLPL_E_BAD_INPUT whatever the sizes.  Every per-match result is bit-identical to mlpl_subpix_separate on
 * the gathered keypoints (the same kernel).
 * d_kp2_out [batch][nt][2] (may be d_kp2) starts as a copy of d_kp2; then, as correspondences.cpp:480-483, every match writes its refined or
 * unchanged position to its train keypoint, and of several matches with one trainIdx the LAST in list order wins.  d_kp1_out (NULL or
 * [batch][nq][2], may be d_kp1) likewise by queryIdx when correspondences_rule == 0; under the rule it is a plain copy of d_kp1: the
 * reference's caller discards the refined keypoints 1.  d_status[b] = step 5.
 * correspondences_rule == 0: the inliers are compacted in list order into d_out + b * match_stride (d_out must not be d_matches),
 * d_n_out[b] their number.  correspondences_rule != 0 applies correspondences.cpp:474-494: on status -1 the list and the keypoints pass
 * through unchanged; on status 0 the inliers are emitted in REVERSE list order.  d_inlier (optional) [batch][match_stride] bytes: the mask
 * of step 4.  batch, match_stride in [1, 65535]. */
int mlpl_subpix_separate_dev(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches,
                             const float *d_kp1, int nq, const float *d_kp2, int nt, const float *d_size1, const float *d_size2,
                             const uint8_t *d_img1, int width1, int height1, size_t step1, size_t batch_stride1, const uint8_t *d_img2,
                             int width2, int height2, size_t step2, size_t batch_stride2, int correspondences_rule, mlpl_dmatch *d_out,
                             int32_t *d_n_out, int32_t *d_status, float *d_kp1_out, float *d_kp2_out, uint8_t *d_inlier, void *stream);

/* ---- stereo rectification: poselib::getRectificationParameters, cv::initUndistortRectifyMap, poselib::GetRectifiedImages ----------
 * The end of the reference harness' per-pair loop (T/poselib-test/main.cpp:2051-2070).  OpenCV is not in this tree: the arithmetic of
 * cv::initUndistortRectifyMap and of cv::remap's fixed-point bilinear path is RESTATED from OpenCV 4.x as remembered, and the operation
 * order of every entry is written down once, in tests/rectify_oracle.py, which the code follows line by line; that file is the definition.
 * The maps and the images of the device equal it bit for bit / byte for byte.
 *
 * mlpl_rectify_parameters: getRectificationParameters with globRectFunct = true, i.e. rectifyFusiello (P/source/pose_helper.cpp:1366-1422,
 * :1459-1857) with cvUndistortPoints2 (:2290-2412) and icvGetRectanglesV0 (:2429-2503).  Host arithmetic, no device, no context.
 *   In: R[9], t[3] (divided by its norm when that is further than 1e-4 from 1, :1394-1397), K1[9], K2[9] (row major), dist1 / dist2 with
 *   n_dist1 / n_dist2 in {0, 4, 5, 8} coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]), the image size, alpha, the new image size
 *   ((0, 0), or any size with a zero side: the image size).  Out: Rect1[9], Rect2[9], Knew[9] (K1new = K2new); optional roi[4] = {x, y,
 *   width, height}, the intersection at :1819-1823 (the reference never writes its roi2 on this branch); optional P1[12], P2[12]; optional info[8] = {fc_new
 *   before scaling, s0, s1 (both 0 when alpha < 0), s, and the number of 0.01 reduction steps each of the four undistortion loops took:
 *   corners of camera 1, of camera 2, the 9 x 9 grid of camera 1, of camera 2}.
 *   Kept from the reference: the float32 roundings of the Point2f corner and grid points (and the float32 arithmetic that forms the grid),
 *   of cvUndistortPoints2's outputs, of the Rect_<float> rectangles (inner.x + inner.width is a float32 sum) and of the proofdist test
 *   against 0.25 (float32 products, sum and root; a NaN passes); the in-place re-undistortion inside the corner loop (a valid corner returns
 *   to its saved pixel position, an invalid one moves inwards by floor()); the coefficient-free pass once the reduction reaches 0.25; the
 *   clamp of s to 1 outside [0.5, 2]; the focal length branch on dk1 < 0 and idx = |t.x| > |t.y| ? 0 : 1.
 *   Deviations:
 *   - The three 3 x 3 inverses (K1; K2 R; Knew) are adjugate over determinant in a fixed order; matrix products add their three terms
 *     left to right.  OpenCV's own inverse and gemm may order differently (last bits).
 *   - cv::projectPoints is handed the 3 x 3 Rect as its rotation; OpenCV passes it through Rodrigues and back, which moves an orthonormal
 *     matrix at 1e-16.  The matrix is used directly.  cv::mean is the sum in order over 4.
 *   - icvGetRectanglesV0 copies its grid into a std::vector and then undistorts the UNINITIALISED matrix the copy was made from, so what
 *     the reference computes there depends on uninitialised memory.  Here the grid itself is undistorted, as in OpenCV's icvGetRectangles,
 *     of which the function is a copy.
 *   - n_dist = 0 is eight zeros (the reference asserts on an empty coefficient matrix).  The (int) casts of the roi saturate, NaN -> 0.
 *   MLPL_E_BAD_INPUT: a NULL input or output matrix, a value that is not finite, t = 0, a size < 1, a negative new size, another n_dist.
 *   The stereoRectify2 branch (globRectFunct = false) is not built.
 *
 * mlpl_rectify_maps / _dev: cv::initUndistortRectifyMap(K, dist, Rect, Knew, size, CV_32FC1, mapx, mapy).  All arithmetic in double, per
 *   pixel (u = column, v = row), one lane for 4 adjacent pixels: ir = (Knew Rect)^-1 on the host as above; _x = u ir0 + (v ir1 + ir2), _y and
 *   _w likewise; x = _x / _w, y = _y / _w; r2 = x x + y y; kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2);
 *   xd = (x kr + p1 ((2 x) y)) + p2 (r2 + 2 x x), yd = (y kr + p1 (r2 + 2 y y)) + p2 ((2 x) y); mapx = (float)(fx xd + cx),
 *   mapy = (float)(fy yd + cy) with fx, fy, cx, cy of K.  Deviation, unmeasured: OpenCV's scalar path accumulates _x += ir0 along a row;
 *   the direct product can differ from it in the last float bit.  Host form: mapx, mapy [height][width] dense.  Device form: row stride
 *   map_stride in floats (>= width), one launch on `stream`, no synchronisation.  Sides in [1, 16384].
 *
 * mlpl_remap_bilinear / _dev: cv::remap(img, out, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT (0)) on an 8-bit single-channel image,
 *   OpenCV's fixed-point path: a = mapx * 32 in float32; sx = round-half-even(a), ix = sx >> 5 saturated to int16, fx = sx & 31, y likewise;
 *   weights (32-fx)(32-fy) 32, fx (32-fy) 32, (32-fx) fy 32, fx fy 32 (sum 2^15) on the taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1);
 *   value = (sum + 16384) >> 15; a tap outside the image adds 0.  (OpenCV stores the weight 32768 as 32767: immaterial, (32767 p + 16384)
 *   >> 15 = p for every byte p.)  Safety: a map value that is NaN or whose product with 32 does not fit an int32 makes the pixel 0; image
 *   sides above 16384 are MLPL_E_BAD_INPUT, so a saturated index is always outside; no source address is formed before its tap has passed
 *   the inside test.  The maps are [out_height][out_width]; step / out_step in bytes (>= width).
 *
 * mlpl_rectify_images_dev: the fused hot path for `batch` pairs in one launch; the image index is a grid dimension.  d_img1 / d_img2:
 *   [batch] planes of width x height bytes, `step` bytes from row to row and batch_stride bytes from pair to pair; d_out1 / d_out2 likewise
 *   with out_width, out_height, out_step, out_batch_stride.  params: a HOST array [batch][2] of blocks {K[9], dist[8], Rect[9], Knew[9]}
 *   (35 doubles; image 1 then image 2 of a pair), read before the call returns.  Each lane computes the map values of 4 adjacent pixels in
 *   registers, rounds them to float32 exactly as mlpl_rectify_maps does, samples as mlpl_remap_bilinear does and stores the 4 bytes with one
 *   store (row tails and unaligned outputs: byte stores); no map reaches memory.  The result is byte for byte mlpl_rectify_maps_dev followed
 *   by mlpl_remap_bilinear_dev.  One small upload and one launch on `stream`, no synchronisation.  batch in [1, 32767].
 * mlpl_rectify_images: the same for one pair of HOST images (params [2][35]). */
int mlpl_rectify_parameters(const double R[9], const double t[3], const double K1[9], const double K2[9], const double *dist1, int n_dist1,
                            const double *dist2, int n_dist2, int width, int height, double alpha, int new_width, int new_height,
                            double Rect1[9], double Rect2[9], double Knew[9], int roi[4], double P1[12], double P2[12], double info[8]);
int mlpl_rectify_maps(mlpl_ctx *ctx, const double K[9], const double *dist, int n_dist, const double Rect[9], const double Knew[9], int width,
                      int height, float *mapx, float *mapy);
int mlpl_rectify_maps_dev(mlpl_ctx *ctx, const double K[9], const double *dist, int n_dist, const double Rect[9], const double Knew[9],
                          int width, int height, float *d_mapx, float *d_mapy, size_t map_stride, void *stream);
int mlpl_remap_bilinear(mlpl_ctx *ctx, const uint8_t *img, int width, int height, size_t step, const float *mapx, const float *mapy, int out_width,
                        int out_height, uint8_t *out, size_t out_step);
int mlpl_remap_bilinear_dev(mlpl_ctx *ctx, const uint8_t *d_img, int width, int height, size_t step, const float *d_mapx, const float *d_mapy,
                            size_t map_stride, int out_width, int out_height, uint8_t *d_out, size_t out_step, void *stream);
int mlpl_rectify_images(mlpl_ctx *ctx, const uint8_t *img1, const uint8_t *img2, int width, int height, size_t step, const double *params,
                        int out_width, int out_height, uint8_t *out1, uint8_t *out2, size_t out_step);
int mlpl_rectify_images_dev(mlpl_ctx *ctx, int batch, const uint8_t *d_img1, const uint8_t *d_img2, int width, int height, size_t step,
                            size_t batch_stride, const double *params, int out_width, int out_height, uint8_t *d_out1, uint8_t *d_out2,
                            size_t out_step, size_t out_batch_stride, void *stream);

/* ---- correspondence gather (pre-step of the pose path) -------------------------------------------------------
 * Replaces the gather + ImgToCamCoordTrans of StereoRefine::addNewCorrespondences (P/source/stereo_pose_refinement.cpp:
 * 428-455, P/source/pose_helper.cpp:1100-1109): p1[i] = ((double)kp1[m.queryIdx] - c0) / f0 rounded to float and widened
 * to double, p2 likewise with kp2[m.trainIdx].  kp1/kp2: device arrays of (x,y) float pairs; K = {fx, fy, cx, cy}.
 * All pointers are device pointers; n = number of matches (known to the host). */
int mlpl_gather_match_points_dev(mlpl_ctx *ctx, const mlpl_dmatch *d_matches, int n, const float *d_kp1, const float *d_kp2,
                                 const double K0[4], const double K1[4], double *d_p1, double *d_p2, void *stream);

/* ---- pre/post steps of the pose path (host-pointer forms) ----------------------------------------------------------
 * mlpl_img_to_cam: ImgToCamCoordTrans (P/source/pose_helper.cpp:1100-1109), pts = n x (x,y) floats rewritten in place,
 *   K = {fx, fy, cx, cy}.
 * mlpl_remove_lens_dist: Remove_LensDist + LensDist_Oulu (pose_helper.cpp:1169-1279): 10 fixed-point iterations per
 *   point and view, correspondences failing the 0.25 proof gate are dropped (order kept), points rewritten in place,
 *   *n_out = remaining count.  No-op when both coefficient sums are within 1e-3 of zero.  MLPL_E_FAILED (-3) = the
 *   reference's `false` (fewer than 16 correspondences left).
 * mlpl_get_inliers_strict: computeReprojError2 + getInlierMask (pose_helper.cpp:639-664, 3030-3045) as used by
 *   StereoRefine::getInliers (stereo_pose_refinement.cpp:2085-2090): err[i] = fp64 Sampson error (kept double),
 *   mask[i] = err[i] < th2 (STRICT, unlike RANSAC's <=).  Returns the inlier count (>= 0) or a negative error. */
int mlpl_img_to_cam(mlpl_ctx *ctx, float *pts, int n, const double K[4]);
int mlpl_remove_lens_dist(mlpl_ctx *ctx, float *points1, float *points2, int n, const double dist1[8], const double dist2[8],
                          int *n_out);
int mlpl_get_inliers_strict(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const double E[9], double th2, double *err,
                            uint8_t *mask);

/* ---- robust essential matrix ----------------------------------------------------------------------------
 * Replaces poselib::estimateEssentialMat(E,p1,p2,"RANSAC",th,refine,mask) (P/source/pose_estim.cpp:857-890)
 * = findEssentialMat (P/source/five-point-nister/five-point.cpp:69-148) = CvModelEstimator3::runRANSAC
 * (modelest.cpp:343-474) with the Nister solver CvEMEstimator::run5Point (five-point.cpp:366-471) and
 * Sampson scoring computeReprojError3 (five-point.cpp:476-503).
 * p1,p2: n x 2 doubles (camera-normalised).  The reference hard-codes max_iters=1000, confidence=0.999
 * and seeds std::srand(time) (modelest.cpp:58); here they are parameters, and `seed` reproduces the glibc
 * srand(seed)/rand() sample stream so that a fixed seed gives the CPU path's hypotheses.
 * refit != 0 = the reference's `lesqu` least-squares step on all inliers (modelest.cpp:420-464).
 * mask: n bytes, 1 = inlier.  Returns 0 on success, MLPL_E_FAILED when no model was found
 * (reference returns false), -1 on bad input.
 */
int mlpl_ransac_essential(mlpl_ctx *ctx, const double *p1, const double *p2, int n, double thresh,
                          double confidence, int max_iters, int refit, uint32_t seed, double E[9],
                          uint8_t *mask, int *n_inliers, int *iters_used);
/* Device-resident points; E/mask/n_inliers/iters_used are HOST outputs (the replay of the sequential
 * best/niters logic needs one device->host hop).  d_p1/d_p2: n x 2 doubles on the device. */
int mlpl_ransac_essential_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, double thresh,
                              double confidence, int max_iters, int refit, uint32_t seed, double E[9],
                              uint8_t *d_mask, int *n_inliers, int *iters_used, void *stream);

/*
 * CvModelEstimator3::runLMeDS (modelest.cpp:483-564) as findEssentialMat drives it for method LMEDS (five-point.cpp:125-129;
 * estimateEssentialMat passes prob = 0.999, pose_estim.cpp:874-877, findEssentialMat maxIters = 2000):
 * niters = clamp(round(log(1-confidence)/log(1-0.55^5)), 3, max_iters) samples from the same glibc stream as RANSAC, the 5-point
 * solver on each, the MEDIAN of the float Sampson errors per model (exact radix select over the bit patterns, the order the
 * reference's int sort gives), the first model with the smallest median, sigma = max(2.5*1.4826*(1+5/(n-5))*sqrt(median), 0.001),
 * mask = err <= sigma^2.  Returns 0, MLPL_E_FAILED when no model was found or fewer than 5 correspondences pass (the mask and
 * *n_inliers are still written in the latter case), -1 on bad input (n must exceed 5).  *min_median may be NULL.
 */
int mlpl_lmeds_essential(mlpl_ctx *ctx, const double *p1, const double *p2, int n, double confidence, int max_iters,
                         uint32_t seed, double E[9], uint8_t *mask, int *n_inliers, double *min_median);
int mlpl_lmeds_essential_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, double confidence, int max_iters,
                             uint32_t seed, double E[9], uint8_t *d_mask, int *n_inliers, double *min_median, void *stream);

/*
 * CvModelEstimator3::runARRSAC (modelest.cpp:197-341) as findEssentialMat drives it for method ARRSAC, the DEFAULT method of
 * poselib::estimateEssentialMat (pose_estim.h:204-210, pose_estim.cpp:866-869; five-point.cpp:120-124): theia::Arrsac(5, thresh^2, 500
 * hypotheses, blocks of 100, inner RANSAC on 14 / at least 8 points) (include/arrsac/arrsac.h:236-547) over the 5-point solver with
 * CvEMEstimator::ValidModel (five-point.cpp:534-601), PROSAC and uniform sampling from two cv::RNG streams, Wald's sequential test per
 * hypothesis, then the preemptive breadth-first stage; the mask is findInliers of the winner; `refine` != 0 runs
 * robustEssentialRefine (pose_estim.cpp:337-792) on its inliers (>= 50 needed) and returns the refined matrix with the unrefined
 * model's mask, as the reference does (modelest.cpp:280-318).  Solver, validity test, all error evaluations and the refinement run on
 * the device in speculative batches; the sequential decisions are taken on the host.
 * rng_state: in/out, the states of the reference's two function-local `static cv::RNG rng;` (prosac_sampler.h:115, random_sampler.h:65),
 * which live as long as the PROCESS there: both are 0xffffffff before the first ARRSAC call of a program and carry over from call to
 * call -- the caller keeps them (the C++ facade keeps one pair per process).  Returns 0, MLPL_E_FAILED when no hypothesis passed or the
 * winner has < 15 inliers (< 50 when n > 200) (modelest.cpp:275-278; the mask and *n_inliers are still written then), -1 on bad input
 * (n must exceed 5; with exactly 5 correspondences findEssentialMat never reaches runARRSAC, use mlpl_solve_5pt).
 */
int mlpl_arrsac_essential(mlpl_ctx *ctx, const double *p1, const double *p2, int n, double thresh, int refine, uint64_t rng_state[2],
                          double E[9], uint8_t *mask, int *n_inliers);
int mlpl_arrsac_essential_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, double thresh, int refine,
                              uint64_t rng_state[2], double E[9], uint8_t *d_mask, int *n_inliers, void *stream);
/* A batch of ARRSAC problems in one call (estimateEssentialMat's default method, pose_estim.h:207): problem b = correspondences d_p1 / d_p2 +
 * b * stride * 2 doubles (device), counts[b] in [6, stride] of them (host), its own pair of cv::RNG states rng_states[2 b], [2 b + 1] (host,
 * in / out -- the reference's samplers draw from process-wide streams; here every problem owns a pair, so problems do not depend on each
 * other).  Every problem runs the sequential program of mlpl_arrsac_essential_dev on its own stack (a fiber on a worker thread) and the launches of all runs that
 * stand at the same point of their control flow are merged into one launch per kernel (csrc/batch_hub.h), 128 problems at a time.
 * Outputs per problem: status[b] (0; MLPL_E_FAILED; other < 0 end the call), E + 9 b, n_inliers[b] (optional), its inlier mask at d_masks +
 * b * stride (device) -- what mlpl_arrsac_essential_dev returns for the problem alone with the same stream states. */
int mlpl_arrsac_essential_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, double thresh,
                                    int refine, uint64_t *rng_states, double *E, uint8_t *d_masks, int32_t *n_inliers, int32_t *status, void *stream);
/*
 * poselib::robustEssentialRefine(points1, points2, E_init, E_refined, th, 0, true, ..., mask, 0) (pose_estim.h:225-228,
 * pose_estim.cpp:337-792) for the essential-matrix model without normalisation: iteratively re-weighted (pseudo-Huber on the Sampson
 * distance, threshold th) 9 x 9 eigenproblem over the correspondences with mask != 0 (mask == NULL: all), the closest essential matrix
 * after every round, the reference's stopping tests; one workgroup on the device.  Fewer than 50 correspondences or a rank-deficient
 * system return E_init.  info (may be NULL) = {the reference's loop counter at the end (index of the round a stopping
 * test fired in -- one less than the rounds executed -- or 50), status: 0 converged or exhausted, 1 stopped on an invalid matrix (last
 * valid one returned), 2 rejected: fewer than 50 correspondences, 3 rejected: rank-deficient system (E_init returned by both)}.  StereoRefine's refineRTold step (stereo_pose_refinement.cpp:1460-1474) and ARRSAC's
 * `refine` are this.
 */
int mlpl_robust_essential_refine(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const uint8_t *mask, const double E_init[9],
                                 double th, double E_refined[9], int info[2]);

/* ARRSAC's model estimators on ONE sample (EssentialMatEstimatorTheia::EstimateModel / EstimateModelNonminimal, modelest.cpp:111-178), a
 * building block exposed for parity tests: idx = m indices into p1/p2; kind 0 = the 5-point solver on 5..7 correspondences (the reference
 * runs run5Point on them: cv::SVD of an m x 9 system, its four last right singular vectors), kind 1 = cv::findFundamentalMat(FM_8POINT)
 * on 8..14.  E_out: 10 x 9 doubles, the first *n_models are models (solver order, library sign convention); valid[i] = ValidModel
 * (five-point.cpp:534-601) on the sample's correspondences.  thresh only sizes internal buffers' inlier rows. */
int mlpl_arrsac_sample_models(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const int32_t *idx, int m, int kind, double thresh,
                              double *E_out, int32_t *n_models, uint8_t *valid);

/* Statistics of the last mlpl_arrsac_essential[_dev] call: {k of the initial hypothesis set, hypotheses after it, PROSAC samples,
 * inner-RANSAC samples, inner-RANSAC restarts, samples of the preemptive stage, correspondence index where that stage ended,
 * hypotheses left there, device batches, samples solved on the device, samples the control flow consumed, refinement status
 * (-1 not run, 0 converged, 1 stopped on an invalid matrix, 2 / 3 rejected: too few points / rank-deficient system)}. */
int mlpl_arrsac_last_stats(mlpl_ctx *ctx, long long stats[12]);

/*
 * poselib::computeHomographyArrsac (pose_homography.h, pose_homography.cpp:478-555): a robust plane-induced homography p2 ~ H p1.
 * n < 4 fails; n == 4 is one call of the normalised DLT kernel (runHomogrophyKernel, :674-744; mask all ones); n > 4 runs
 * theia::Arrsac(4, th^2, 500 hypotheses, blocks of 100, inner RANSAC on at most 12 points) (:505) -- the template mlpl_arrsac_essential
 * runs for E, with the 4-point DLT as the minimal estimator, cv::findHomography(m1, m2, 0) (float32 points, DLT, 10 Levenberg-Marquardt
 * turns) as the non-minimal one and the one-way transfer error (:642-663, strict < th^2 inside ARRSAC) -- then findHomographyInliers
 * (:785-813, err <= th^2 over all n) and refineHomography on those inliers (:825-885, CvLevMarq, 10 iterations).  H is the refined matrix
 * (H(2,2) as the DLT scaled it: 1 to rounding), the mask is the one from before the refinement, as in the reference.  Estimators, error
 * evaluations, mask, compaction and refinement run on the device; the sequential decisions are taken on the host.
 * rng_state: in/out, the SAME two cv::RNG streams mlpl_arrsac_essential uses (function-local statics of the reference's samplers, shared
 * by every theia::Arrsac instantiation of a process); they advance whenever ARRSAC ran, also when it found nothing.
 * stats (may be NULL): [0..7] as mlpl_arrsac_last_stats -- {k of the initial hypothesis set, hypotheses after it, PROSAC samples,
 * inner-RANSAC samples, inner-RANSAC restarts, samples of the preemptive stage, correspondence index where that stage ended, hypotheses
 * left there} --, [8] device batches, [9] samples solved on the device, [10] samples the control flow consumed, [11] outliers.
 * Returns 0; MLPL_E_FAILED for the reference's `false` (n < 4, a degenerate quadruple, no hypothesis passed the sequential test: a
 * result, not an error -- H, mask and *n_inliers are not written); MLPL_E_BAD_INPUT for a malformed call (null pointers, n < 1, th not
 * positive and finite; nothing is launched); MLPL_E_INTERNAL if more than 8192 samples had to be solved in one call (rng_state untouched).
 * Every model is tested on the first 1024 correspondences up front; at inlier ratios above ~0.9 the preemptive stage keeps generating
 * hypotheses and runs past them (its first halving comes at correspondence 1100), and the survivors' bits over all n are then computed
 * on demand.  The _dev form takes device pointers and leaves the mask on the device.
 */
int mlpl_homography_arrsac(mlpl_ctx *ctx, const double *p1, const double *p2, int n, double th, uint64_t rng_state[2], double H[9], uint8_t *mask,
                           int *n_inliers, long long stats[12]);
int mlpl_homography_arrsac_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, double th, uint64_t rng_state[2], double H[9],
                               uint8_t *d_mask, int *n_inliers, long long stats[12], void *stream);
/* findHomographyInliers (pose_homography.cpp:785-813): mask[i] = 0 iff the transfer error of correspondence i under H exceeds th^2
 * (H(2,2) is taken as 1, as the reference's error does); *n_inliers (may be NULL) = the count. */
int mlpl_homography_inliers(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const double H[9], double th, uint8_t *mask, int *n_inliers);
int mlpl_homography_inliers_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const double H[9], double th, uint8_t *d_mask,
                                int *n_inliers, void *stream);
/*
 * poselib::estimateMultHomographys (pose_homography.cpp:291-463): plane after plane with mlpl_homography_arrsac at 1.5 th (with var_th:
 * times 1.5 per failed try while below 6 th), the outliers of a round are the next round's input in their original order, while more than
 * 3 correspondences remain, the last plane had at least min_pts_per_plane inliers and (max_planes == 0 or fewer than max_planes rounds
 * ran).  A plane is reported only with at least min_pts_per_plane inliers.  The correspondences stay on the device between rounds.
 * Outputs for plane k < *n_planes, in the reference's output order (by inlier count, descending, std::sort, when more than one plane was
 * found): H + 9 k, num_inl[k], strength[k] = 1.5 th num_inl / (th_used n), th_used[k] = the threshold of the successful try, masks + k n
 * (n bytes in the ORIGINAL indexing; masks may be NULL).  cap = planes the output arrays hold; finding more is MLPL_E_BAD_INPUT.
 * *n_planes = -1 is the reference's return value -1 (the first plane was not found); the call itself returns 0 then.  rng_state as above.
 */
int mlpl_mult_homographies(mlpl_ctx *ctx, const double *p1, const double *p2, int n, double th, int var_th, unsigned max_planes, unsigned min_pts_per_plane,
                           uint64_t rng_state[2], int cap, int *n_planes, double *H, int32_t *num_inl, double *strength, double *th_used, uint8_t *masks);
int mlpl_mult_homographies_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, double th, int var_th, unsigned max_planes,
                               unsigned min_pts_per_plane, uint64_t rng_state[2], int cap, int *n_planes, double *H, int32_t *num_inl, double *strength,
                               double *th_used, uint8_t *d_masks, void *stream);
/* The same with one LABEL per correspondence instead of -- or beside -- the masks: the planes' inlier sets are disjoint, so labels (n
 * int32: output plane index, -1 = none) hold what cap masks hold, and cap may be the worst case n / max(min_pts_per_plane, 1) + 1 at the
 * cost of a few words per plane.  found_at[k] (cap int32) = the round that found output plane k: ascending found_at is the order of
 * discovery, which the reference keeps when its caller does not ask for num_inl.  found_at, labels and masks may each be NULL; masks are
 * written for the planes found only.  Finding more than cap planes returns MLPL_E_BAD_INPUT with rng_state put back (both forms, and the
 * entries above), so the call can be repeated with larger arrays. */
int mlpl_mult_homographies_labels(mlpl_ctx *ctx, const double *p1, const double *p2, int n, double th, int var_th, unsigned max_planes,
                                  unsigned min_pts_per_plane, uint64_t rng_state[2], int cap, int *n_planes, double *H, int32_t *num_inl, double *strength,
                                  double *th_used, int32_t *found_at, int32_t *labels, uint8_t *masks);
int mlpl_mult_homographies_labels_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, double th, int var_th, unsigned max_planes,
                                      unsigned min_pts_per_plane, uint64_t rng_state[2], int cap, int *n_planes, double *H, int32_t *num_inl,
                                      double *strength, double *th_used, int32_t *found_at, int32_t *d_labels, uint8_t *d_masks, void *stream);
/* Batches of the two plane estimators in one call, laid out as mlpl_arrsac_essential_batch_dev: problem b = correspondences d_p1 / d_p2 +
 * b * stride * 2 doubles (device), counts[b] in [0, stride] of them (host), its own pair of cv::RNG states rng_states[2 b], [2 b + 1] (host,
 * in / out).  Every problem runs the sequential program of the single entry on its own stack (a fiber on a worker thread) and the launches
 * of all runs that stand at the same point of their control flow are merged into one launch per kernel (csrc/batch_hub.h), 128 problems
 * at a time; the options hub_cohort, hub_lanes, hub_workers and hub_blocking_sync apply.  Every problem's outputs are byte for byte what
 * mlpl_homography_arrsac_dev / mlpl_mult_homographies_labels_dev returns for it alone with the same stream states.
 * mlpl_homography_arrsac_batch_dev: per problem status[b] (0; MLPL_E_FAILED = the reference's `false`, counts[b] < 4 included, with the
 * stream states as the single entry leaves them), H + 9 b, n_inliers[b], its mask at d_masks + b * stride (device), stats + 12 b (stats may
 * be NULL).
 * mlpl_mult_homographies_batch_dev: per problem n_planes[b] (-1 = the reference's -1, with status[b] = 0; counts[b] < 4: -1 with status[b]
 * = MLPL_E_FAILED and the stream states untouched) and cap planes each of H [b][cap][9], num_inl, strength, th_used, found_at [b][cap]
 * (found_at may be NULL), labels at d_labels + b * stride (device, may be NULL), plane indices in the reference's output order.
 * Any other negative status[b] ends the call, which returns the first such code with its message (the message names the problem): finding
 * more than cap planes in a problem is MLPL_E_BAD_INPUT with that problem's stream states put back.  A malformed call (null required
 * pointers, n_problems < 0, stride < 1, a counts[b] outside [0, stride], th not positive and finite, cap < 1) is MLPL_E_BAD_INPUT with
 * nothing launched; n_problems == 0 returns 0.  After a batch mlpl_arrsac_last_stats [8] / [9] hold the hub's rounds / merged launches. */
int mlpl_homography_arrsac_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, double th,
                                     uint64_t *rng_states, double *H, uint8_t *d_masks, int32_t *n_inliers, int32_t *status, long long *stats,
                                     void *stream);
int mlpl_mult_homographies_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, double th,
                                     int var_th, unsigned max_planes, unsigned min_pts_per_plane, uint64_t *rng_states, int cap, int32_t *n_planes,
                                     double *H, int32_t *num_inl, double *strength, double *th_used, int32_t *found_at, int32_t *d_labels, int32_t *status,
                                     void *stream);
/*
 * Pose from planes: the second half of poselib::estimatePoseHomographies (pose_homography.h, pose_homography.cpp:127-269).
 *
 * mlpl_homography_alignment[_dev]: Homographys_Alignment (HomographyAlignment.cpp:197-360) and its caller's part (ComputeHomographyMotion
 * :82-171, pose_homography.cpp:195-213), the building block without any plane search: n correspondences in camera coordinates with one
 * label each (the plane, or -1 = none: what mlpl_mult_homographies_labels writes), n_planes planes with num_inl[k] correspondences
 * (plane 0 the dominant one), H0 = plane 0's homography, tol = the inlier threshold.  One workgroup runs the whole problem in one
 * launch (csrc/homography_align_impl.h).  Outputs: R (the rotation from camera 1 to camera 2), t (minus the position of camera 2 in
 * camera 1's frame, unit length), E = [t]x R as the reference forms it, norms [n_planes][3] (plane k: norms_k . P1 = 1 up to the scale
 * of t), Hs_out [n_planes][9] the planes' homographies R (I - t' n_k^T) / h22 under the common motion, and
 * info[24]: [0] the code -- 0, or -3 "Homography alignment failed" --, [1] the chosen candidate q, [2..5] / [6..9] the rounds run in each
 * of the 4 outer turns for q = 0 / 1 (0 = turn not run), [10] [11] the last mean transfer error per q, [12..15] the motion errors (the
 * two initial candidates, the two results), [16] the sign-candidate choices (bit 4 q + turn), [17] the reason of a -3: 1 a
 * Longuet-Higgins decomposition refused the matrix, 2 fewer than two of its sign candidates have plane(2) > 0, 3 no ray pair counted in
 * Check_motion_error, 4 a result is not finite (a pure rotation ends here), 5 fewer than two planes (the reference's defined answer),
 * 6 a plane without correspondences; 1-4 and 6 are cases in which the reference reads unset memory or divides by zero.
 * The calls return 0 for the code -3 too, and then write nothing but info.  MLPL_E_BAD_INPUT (nothing launched): null pointers, n < 1,
 * n_planes outside [0, 64], tol not positive and finite, a label >= n_planes, num_inl not matching the labels.
 * The _dev form takes d_p1, d_p2, d_labels on the device (the labels are read back once to check them); everything else is host memory.
 */
int mlpl_homography_alignment(mlpl_ctx *ctx, const double *p1, const double *p2, const int32_t *labels, int n, int n_planes, const int32_t *num_inl,
                              const double H0[9], double tol, double R[9], double t[3], double E[9], double *norms, double *Hs_out, double info[24]);
int mlpl_homography_alignment_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, const int32_t *d_labels, int n, int n_planes,
                                  const int32_t *num_inl, const double H0[9], double tol, double R[9], double t[3], double E[9], double *norms,
                                  double *Hs_out, double info[24], void *stream);
/*
 * mlpl_pose_homographies[_dev]: the whole of estimatePoseHomographies -- the rows the optional input mask keeps (mask_in may be NULL;
 * order kept), mlpl_mult_homographies_labels on them with (th, var_th, MAX_PLANES_PER_PAIR = 50, MIN_PTS_PLANE = 15), with
 * check_plane_strength the gate "the strengths above 0.1 sum to more than 0.5", the alignment above with tol = th, and the mask
 * computeReprojError2 < th^2 (strict) over ALL n rows.  *result = the reference's return value: 0, -1 (no plane found), -2 (the planes
 * are too weak), -3 (alignment failed; fewer than 4 kept rows end here or at -2, because the reference's plane loop then reports no
 * plane); the call itself returns 0 for all four.  R, t, E, *n_inliers and mask_out (n bytes) are written only with *result == 0.
 * Optional, all NULL or all set with cap >= 1: *n_planes, H [cap][9], num_inl [cap], strength [cap] -- the planes in the reference's
 * order, written whenever the plane search ran (finding more than cap planes is MLPL_E_BAD_INPUT with rng_state put back).  labels (may be
 * NULL; n int32): the plane of every KEPT row, in the kept rows' order.  info (may be NULL): the alignment's 24 doubles.  rng_state as in
 * mlpl_homography_arrsac.  The _dev form takes d_p1, d_p2, d_mask_in, d_mask_out and d_labels on the device.
 */
int mlpl_pose_homographies(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const uint8_t *mask_in, double th, int check_plane_strength, int var_th,
                           uint64_t rng_state[2], int *result, double R[9], double t[3], double E[9], int *n_inliers, uint8_t *mask_out, int cap,
                           int *n_planes, double *H, int32_t *num_inl, double *strength, int32_t *labels, double *info);
int mlpl_pose_homographies_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const uint8_t *d_mask_in, double th, int check_plane_strength,
                               int var_th, uint64_t rng_state[2], int *result, double R[9], double t[3], double E[9], int *n_inliers, uint8_t *d_mask_out,
                               int cap, int *n_planes, double *H, int32_t *num_inl, double *strength, int32_t *d_labels, double *info, void *stream);
/* A batch of estimatePoseHomographies problems in one call, laid out as mlpl_mult_homographies_batch_dev (no input masks): problem b =
 * d_p1 / d_p2 + b * stride * 2 doubles (device), counts[b] in [0, stride] rows (host), the stream pair rng_states[2 b], [2 b + 1] (host,
 * in / out).  Every problem runs the single entry's sequential program as a fiber (csrc/batch_hub.h); the launches of the runs that
 * stand at the same point are merged -- the alignment, the final mask and the copies of their results are ONE launch each per cohort.
 * Per problem: results[b] (0 / -1 / -2 / -3), R + 9 b, t + 3 b, E + 9 b, n_inliers[b] and the mask at d_masks + b * stride (device) --
 * these five written only with results[b] == 0 --, n_planes[b] and cap planes each of H [b][cap][9], num_inl, strength [b][cap], the
 * labels at d_labels + b * stride (device, may be NULL), info + 24 b (may be NULL), status[b] (0, or the error that ended the call).
 * Every problem's outputs and stream states are byte for byte what mlpl_pose_homographies_dev returns for it alone.  Malformed calls
 * (null required pointers, n_problems < 0, stride < 1, a counts[b] outside [0, stride], th not positive and finite, cap < 1) are
 * MLPL_E_BAD_INPUT with nothing launched; more than cap planes in a problem is MLPL_E_BAD_INPUT with that problem's streams put back. */
int mlpl_pose_homographies_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, double th,
                                     int check_plane_strength, int var_th, uint64_t *rng_states, int32_t *results, double *R, double *t, double *E,
                                     int32_t *n_inliers, uint8_t *d_masks, int cap, int32_t *n_planes, double *H, int32_t *num_inl, double *strength,
                                     int32_t *d_labels, double *info, int32_t *status, void *stream);
/* The homography estimators on `count` samples of m indices each (idx [count][m], 4 <= m <= 12), a building block exposed for parity
 * tests (the twin of mlpl_arrsac_sample_models): m == 4 the minimal DLT, m > 4 findHomography(., ., 0) with the reference's rejection.
 * H [count][9], ok [count] (0 = the normalisation refused the sample or the model was rejected). */
int mlpl_debug_homography_models(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const int32_t *idx, int m, int count, double *H, int32_t *ok);

/*
 * USAC essential-matrix estimation with the Nister minimal solver -- poselib::estimateEssentialOrPoseUSAC (pose_estim.h:212-223,
 * pose_estim.cpp:1737-2244) -> estimateEssentialMatUsac (source/usac/usac_estimations.cpp:283-735) -> USAC<EssentialMatEstimator>::solve
 * (include/usac/estimators/USAC.h:335-620, EssentialMatEstimator.h): PROSAC or uniform sampling, sample pre-validation, the oriented
 * epipolar constraint on every model, Wald's sequential test over a shuffled evaluation order with re-estimated delta / epsilon,
 * local optimisation (5 inner repetitions of a 14-point fit + 4 re-weighted refits; `refine` below) on every new best model, and the
 * SPRT-aware stopping criterion.  The harness default estimator (tests/poselib-test/main.cpp:734).  Minimal solves, validity tests and
 * every error evaluation run on the device in speculative batches, the refits as one launch (REF_WEIGHTS) or one chain of launches
 * (5-point refinements) per local optimisation; the sequential
 * decisions are taken on the host.  params->check_degeneracy switches the degeneracy handling of
 * UsacChkDegenType::DEGEN_USAC_INTERNAL on: EssentialMatEstimator::testSolutionDegeneracyRot / NoMot and upgradeDegenerateModel
 * (EssentialMatEstimator.h:1334-1362, 1511-1663, 1838-1911, 2098-2361); results through mlpl_usac_last_degeneracy.  Not built: the
 * homography test the reference adds with the 8-point refinements (:1368-1505; its upgrade branch :1958-2015 writes past a vector and
 * reads a translation nothing has set), DEGEN_QDEGSAC.
 * The reference seeds srand(time(nullptr)) and shuffles its evaluation order on the process-wide stream; `seed` is that seed.
 * estimator: PoseEstimator value, 0 = POSE_NISTER, 2 = POSE_STEWENIUS (both are exact 5-point solvers with the same real solution set;
 * the device solver serves both, solutions ordered by the library's convention); refine: RefineAlg value of the local optimisation's
 * fits (EssentialMatEstimator::generateRefinedModel :526-850, findWeights :2366-2428): 0 = REF_WEIGHTS (8-point fit with Torr weights),
 * 4 = REF_STEWENIUS, 5 = REF_STEWENIUS_WEIGHTS (ConfigUSAC's default, pose_estim.h:99-100), 6 = REF_NISTER, 7 = REF_NISTER_WEIGHTS -- the
 * five-point solver on all points of the fit set (unit bearing vectors; the _WEIGHTS forms scale the rows of a re-weighted step by the
 * pseudo-Huber weights of P/source/usac/utils/weightingEssential.cpp:190-206), of its solutions the one with the smallest Sampson-error
 * sum over the inliers of the best model so far.  Other values (REF_8PT_PSEUDOHUBER, REF_EIG_KNEIP(_WEIGHTS), POSE_EIG_KNEIP):
 * MLPL_E_UNSUPPORTED.  check_degeneracy = 3 goes with refine = 0 only (usac_estimations.cpp:368-375).
 * results[12] = {1, hypotheses, models, samples rejected by pre-validation, models rejected by the oriented constraint, inliers of the
 * best model, correspondences verified, local optimisations, SPRT delta and epsilon the reference reports back (newest history entry,
 * usac_estimations.cpp:459-468 halves epsilon itself), delta and epsilon at the end}.  mask: n bytes, 1 = inlier of the returned model.
 * Returns 0; MLPL_E_FAILED when solve() refuses (fewer than 5 correspondences, or fewer than 20 with PROSAC).
 */
typedef struct {
    double th;             /* inlier threshold in camera coordinates (not squared) */
    double conf;           /* 0.99 */
    int32_t max_hyp;       /* 50000 */
    int32_t estimator;     /* poselib::PoseEstimator */
    int32_t refine;        /* poselib::RefineAlg */
    uint32_t seed;
    double prosac_beta;    /* 0.09, or the SPRT delta when the automatic PROSAC parameter is on */
    double sprt_delta;     /* 0.05 */
    double sprt_epsilon;   /* 0.15 */
    double sprt_mS;        /* 8.5 for Nister on the first call of a process, then models / hypotheses so far */
    double sprt_tM;        /* 2314 (Nister), 2736 (Stewenius) */
    const uint32_t *sorted_idx; /* HOST pointer: NULL = uniform sampling; else n indices, best match first = PROSAC */
    int32_t check_degeneracy; /* 0 = DEGEN_NO_CHECK; 1 = the rotation-only / no-motion tests after every new best model and the
                                 upgrade R -> R + t, no motion -> t (DEGEN_USAC_INTERNAL); 3 = also after every local optimisation
                                 (what estimateEssentialMatUsac switches on with the 8-point refinements, usac_estimations.cpp:368-371) */
    int32_t reserved;
    double th_pixels;      /* ConfigUSAC::th_pixels (0.8): with focal_length the angular threshold of the degeneracy tests */
    double focal_length;   /* ConfigUSAC::focalLength (800) */
} mlpl_usac_params;
void mlpl_usac_default_params(mlpl_usac_params *p, double th);
int mlpl_usac_essential(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const mlpl_usac_params *params, double E[9],
                        uint8_t *mask, double results[12]);
int mlpl_usac_essential_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const mlpl_usac_params *params, double E[9],
                            uint8_t *d_mask, double results[12], void *stream);
/*
 * A batch of USAC problems in one call -- the harness runs estimateEssentialOrPoseUSAC once per image pair (T/poselib-test/main.cpp:
 * 1440-2072, RobMethod "USAC" is its default, :734); a rank's share of a batch of pairs is many such problems.  Problem b: correspondences
 * d_p1 / d_p2 + b * stride * 2 doubles (device, camera coordinates), counts[b] <= stride of them (host), parameters params[b] (host; its own
 * seed, thresholds, PROSAC order).  Every problem runs the sequential program of mlpl_usac_essential_dev on its own stack (a fiber on a worker thread), and the
 * launches of all runs that stand at the same point of their control flow are merged into ONE launch per kernel (problem = grid
 * dimension; csrc/batch_hub.h), 128 problems at a time.  Outputs per problem: status[b] (0; MLPL_E_FAILED = solve() refused; < 0 other
 * errors, which also end the call), E + 9 b, results + 12 b, its inlier mask at d_masks + b * stride (device, optional), degen + 16 b
 * (optional: what mlpl_usac_last_degeneracy's info[] returns), its decision trace at trace + b * trace_cap * 16 with trace_lens[b]
 * records (optional, diagnostics).  Every output equals what mlpl_usac_essential_dev returns for that problem alone
 * (tests/test_gpu_usac_batch.py: records and event traces of 64 problems).
 */
int mlpl_usac_essential_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts,
                                  const mlpl_usac_params *params, double *E, uint8_t *d_masks, double *results, int32_t *status, double *degen,
                                  double *trace, int trace_cap, int32_t *trace_lens, void *stream);
/* Statistics of the last mlpl_usac_essential[_dev] call: {device batches, samples solved on the device, samples the control flow
 * consumed, local-optimisation launches / chain runs, of which chain resumes, rechecks of the solution choices after a repetition
 * stored a new best model (5-point refinements), chains re-run because a choice changed, Jacobi sweeps (REF_WEIGHTS)}.
 * After a BATCHED call (mlpl_usac_essential_batch_dev, mlpl_pair_pose_batch_usac_dev): {hub rounds, merged launches, microseconds the hub
 * waited for host work (summed over the lanes), microseconds of device work (summed), microseconds spent starting the runs, microseconds
 * of the whole call, lanes (cohorts served side by side) the call used, cohorts}. */
int mlpl_usac_last_stats(mlpl_ctx *ctx, long long stats[8]);
/* What the degeneracy tests of the last mlpl_usac_essential[_dev] call found -- the quantities estimateEssentialMatUsac hands to
 * estimateEssentialOrPoseUSAC (usac_estimations.cpp:564-636, 689-726; pose_estim.cpp:2044-2133 takes the decision "degenerate" from
 * them): info[16] = {1 if the tests ran, inliers of the best rotation-only model (degen_inlier_count_rot), inliers of "no motion"
 * (degen_inlier_count_noMot), degeneracy type of the last test (EssentialMatEstimator.h:168-175 bit set), R_degenerate[9] row-major,
 * 0...}; flags_rot / flags_nomot (n bytes each, may be NULL): the inlier masks of the two degenerate models.  Returns 0, or
 * MLPL_E_BAD_INPUT when n differs from the last call's correspondence count (masks requested) or no call has been made. */
int mlpl_usac_last_degeneracy(mlpl_ctx *ctx, double info[16], uint8_t *flags_rot, uint8_t *flags_nomot, int n);

/*
 * One image pair through the whole hot path, device-resident (the per-pair body of the reference harness loop,
 * tests/poselib-test/main.cpp:1440-2072, and of StereoRefine's first call): Hamming 2-NN + 0.75 ratio test -> gather of the matched
 * keypoints with ImgToCamCoordTrans -> RANSAC essential matrix -> cheirality.  d_q/d_t: dense nq/nt x nbytes descriptors,
 * d_kp1/d_kp2: (x, y) float pixel coordinates per keypoint, K = {fx, fy, cx, cy}, thresh in camera units.  Two host hops.
 * status: 0 = pose found, -1 = fewer than 16 matches, -2 = RANSAC found no model.
 */
typedef struct {
    int32_t n_matches, n_inliers, n_good, status, iters, pad;
    double E[9], R[9], t[3];
} mlpl_pair_result;
int mlpl_pair_pose_dev(mlpl_ctx *ctx, const uint8_t *d_q, int nq, const uint8_t *d_t, int nt, int nbytes, const float *d_kp1,
                       const float *d_kp2, const double K0[4], const double K1[4], double thresh, int max_iters, double confidence,
                       int refit, uint32_t seed, double dist, mlpl_pair_result *out, void *stream);
/* The same pair with CV_32F descriptors (SIFT, RootSIFT, KAZE ...: the float half of getMatches "LINEAR", M/source/matchers.cpp:632-707):
 * squared-L2 2-NN + 0.75 ratio test (mlpl_match_l2_dev) in place of the Hamming step, everything behind it unchanged.  d_q / d_t: dense
 * nq / nt x dim floats, dim in [1,1024].  Record fields, status codes and host hops as mlpl_pair_pose_dev. */
int mlpl_pair_pose_f32_dev(mlpl_ctx *ctx, const float *d_q, int nq, const float *d_t, int nt, int dim, const float *d_kp1,
                           const float *d_kp2, const double K0[4], const double K1[4], double thresh, int max_iters, double confidence,
                           int refit, uint32_t seed, double dist, mlpl_pair_result *out, void *stream);

/*
 * A BATCH of image pairs through the same pipeline with the pair as a grid dimension of every launch (the reference harness loop over
 * image pairs, tests/poselib-test/main.cpp:1440-2072; BASELINE config 5): d_q / d_t / d_kp1 / d_kp2 hold n_pairs contiguous items
 * ([n_pairs][nq][nbytes], [n_pairs][nt][nbytes], [n_pairs][nq][2], [n_pairs][nt][2]), seeds[n_pairs] and out[n_pairs] are HOST arrays.
 * Every pair's record equals what mlpl_pair_pose_dev returns for it with the same seed.  Host hops per internal batch of 256 pairs
 * (option "pair_batch"): the match counts, one per RANSAC pass (the first 324 iterations of every pair, then the rest for the pairs
 * the adaptive bound has not stopped), the results.  refit != 0 runs the pairs one by one through mlpl_pair_pose_dev.
 */
int mlpl_pair_pose_batch_dev(mlpl_ctx *ctx, int n_pairs, const uint8_t *d_q, int nq, const uint8_t *d_t, int nt, int nbytes, const float *d_kp1,
                             const float *d_kp2, const double K0[4], const double K1[4], double thresh, int max_iters, double confidence,
                             int refit, const uint32_t *seeds, double dist, mlpl_pair_result *out, mlpl_dmatch *d_matches_out, void *stream);
/* mlpl_pair_pose_batch_dev on CV_32F descriptors (M/source/matchers.cpp:632-707 as the matching step): d_q / d_t are
 * [n_pairs][nq][dim] / [n_pairs][nt][dim] floats, `dim` stands where `nbytes` stood; everything else -- record fields and status codes
 * (-1 fewer than 16 matches, -2 estimator failure), host hops, d_matches_out, mlpl_pair_batch_last_stats, refit != 0 falling back to the
 * single-pair entry (mlpl_pair_pose_f32_dev) -- as above.  Every pair's record equals what mlpl_pair_pose_f32_dev returns for it. */
int mlpl_pair_pose_batch_f32_dev(mlpl_ctx *ctx, int n_pairs, const float *d_q, int nq, const float *d_t, int nt, int dim, const float *d_kp1,
                                 const float *d_kp2, const double K0[4], const double K1[4], double thresh, int max_iters, double confidence,
                                 int refit, const uint32_t *seeds, double dist, mlpl_pair_result *out, mlpl_dmatch *d_matches_out, void *stream);
/* mlpl_pair_pose_batch_dev (refit = 0) with `lanes` calls in flight on one GPU: lane l = (ctxs[l], streams[l]: a context and a stream of
 * its own, same device) runs the l-th contiguous share of the batch on its own host thread inside this call, which returns when every
 * lane has finished AND its stream is idle.  Inputs must be complete before the call (they were produced on another stream).
 * lane_span_ms: NULL or 2 * lanes doubles {start, end} of each lane's call in milliseconds since entry (diagnostics). */
int mlpl_pair_pose_batch_lanes_dev(mlpl_ctx *const *ctxs, void *const *streams, int lanes, int n_pairs, const uint8_t *d_q, int nq, const uint8_t *d_t, int nt,
                                   int nbytes, const float *d_kp1, const float *d_kp2, const double K0[4], const double K1[4], double thresh, int max_iters,
                                   double confidence, const uint32_t *seeds, double dist, mlpl_pair_result *out, mlpl_dmatch *d_matches_out,
                                   double *lane_span_ms);
/*
 * The same batch with USAC -- the reference harness' default RobMethod (T/poselib-test/main.cpp:734) -- as the robust estimator:
 * matching, match counts, gather + ImgToCamCoordTrans as above, then mlpl_usac_essential_batch_dev on the pairs' correspondences (every
 * pair's sequential program on its own stack, every launch merged over the pairs), then the batched cheirality step.  *usac:
 * the parameters every pair runs with (th, conf, max_hyp, estimator, refine, SPRT start values, degeneracy tests; its seed and sorted_idx
 * are ignored); seeds[n_pairs]: the pairs' seeds; prosac != 0: PROSAC sampling in the order of the matching costs -- poselib::
 * getSortedMatchIdx' std::sort of the pair's matches (pose_helper.cpp:2896-2923) -- else uniform sampling.  Record per pair:
 * status 0, -1 (fewer than 16 matches) or -2 (USAC failed); iters = hypotheses, n_inliers = inliers of the USAC model, n_good, E, R, t --
 * what mlpl_match_hamming_dev + mlpl_gather_match_points_dev -> mlpl_usac_essential_dev -> mlpl_recover_pose_dev return for the pair.
 */
int mlpl_pair_pose_batch_usac_dev(mlpl_ctx *ctx, int n_pairs, const uint8_t *d_q, int nq, const uint8_t *d_t, int nt, int nbytes, const float *d_kp1,
                                  const float *d_kp2, const double K0[4], const double K1[4], const mlpl_usac_params *usac, int prosac,
                                  const uint32_t *seeds, double dist, mlpl_pair_result *out, mlpl_dmatch *d_matches_out, void *stream);
/* The USAC batch on CV_32F descriptors (matching step: M/source/matchers.cpp:632-707; [n_pairs][nq][dim] / [n_pairs][nt][dim] floats): the
 * record per pair is what mlpl_match_l2_dev + mlpl_gather_match_points_dev -> mlpl_usac_essential_dev -> mlpl_recover_pose_dev return
 * for it; the PROSAC order is the same std::sort of the (float) matching costs; the cohorts are fed as above -- the later cohorts are
 * matched beside the earlier cohorts' estimators, through the one context: the float matcher's per-context blocks are sized by the
 * first (largest) cohort, and its data-kind hint word may be stale across cohorts, which can cost speed and never results. */
int mlpl_pair_pose_batch_usac_f32_dev(mlpl_ctx *ctx, int n_pairs, const float *d_q, int nq, const float *d_t, int nt, int dim, const float *d_kp1,
                                      const float *d_kp2, const double K0[4], const double K1[4], const mlpl_usac_params *usac, int prosac,
                                      const uint32_t *seeds, double dist, mlpl_pair_result *out, mlpl_dmatch *d_matches_out, void *stream);
/* ... and with ARRSAC, estimateEssentialMat's default method (pose_estim.h:207; `refine` = robustEssentialRefine on the winner's inliers):
 * mlpl_arrsac_essential_batch_dev on the pairs' correspondences.  rng_states[2 * n_pairs]: a pair of cv::RNG states per image pair (in / out).
 * Record per pair: status 0 / -1 / -2 (ARRSAC failed), iters = 0, n_inliers = inliers of the unrefined winner, n_good, E, R, t. */
int mlpl_pair_pose_batch_arrsac_dev(mlpl_ctx *ctx, int n_pairs, const uint8_t *d_q, int nq, const uint8_t *d_t, int nt, int nbytes, const float *d_kp1,
                                    const float *d_kp2, const double K0[4], const double K1[4], double thresh, int refine, uint64_t *rng_states, double dist,
                                    mlpl_pair_result *out, mlpl_dmatch *d_matches_out, void *stream);
/* The ARRSAC batch on CV_32F descriptors (matching step: M/source/matchers.cpp:632-707), otherwise as mlpl_pair_pose_batch_arrsac_dev. */
int mlpl_pair_pose_batch_arrsac_f32_dev(mlpl_ctx *ctx, int n_pairs, const float *d_q, int nq, const float *d_t, int nt, int dim, const float *d_kp1,
                                        const float *d_kp2, const double K0[4], const double K1[4], double thresh, int refine, uint64_t *rng_states,
                                        double dist, mlpl_pair_result *out, mlpl_dmatch *d_matches_out, void *stream);
/* poselib::getSortedMatchIdx (P/source/pose_helper.cpp:2896-2923) on a HOST match list: the indices of the matches in the order
 * std::sort leaves them when comparing the distances -- the PROSAC order estimateEssentialOrPoseUSAC and the batch entry above use. */
int mlpl_sorted_match_idx(const mlpl_dmatch *matches, int n, uint32_t *sorted_idx);
/* The same batch behind the matching -- the batched form of mlpl_ransac_essential_dev (refit = 0) followed, with recover_pose != 0, by
 * mlpl_recover_pose_dev on the RANSAC inliers: problem b's correspondences are d_p1 / d_p2 + b * stride * 2 (camera coordinates, n x 2
 * doubles, device), counts[b] <= stride of them (host array), seeds[b] its srand() seed.  Records as above with n_matches = counts[b];
 * status -1 for fewer than 6 correspondences, -2 when RANSAC finds no model; R, t, n_good stay zero without recover_pose.  d_masks: NULL or
 * a device block [n_problems][stride] that receives the inlier masks (after cheirality when recover_pose is set, as mlpl_recover_pose_dev
 * leaves them).  Every record equals what the single-problem entries return for that problem (tests/test_gpu_batch.py). */
int mlpl_ransac_essential_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts, double thresh,
                                    int max_iters, double confidence, const uint32_t *seeds, int recover_pose, double dist, mlpl_pair_result *out,
                                    uint8_t *d_masks, void *stream);
/*
 * poselib::refineEssentialLinear(p1, p2, E, mask, refineMethod, nr_inliers, R, t, th, num_iterative_steps, threshold_multiplier,
 * pseudoHuberThreshold_multiplier, maxRelativeInlierCntLoss) (P/include/poselib/pose_linear_refinement.h, P/source/pose_linear_refinement.cpp:85-635):
 * the iteratively re-weighted linear refit of E on its inliers.  method = solver | weights as poselib::RefinePostAlg: solver 0x1 PR_8PT,
 * 0x2 PR_NISTER, 0x3 PR_STEWENIUS (one exact five-point solver serves both, as in USAC), weights 0x10 PR_TORR_WEIGHTS, 0x20
 * PR_PSEUDOHUBER_WEIGHTS (threshold th * ph_mult), 0x30 PR_NO_WEIGHTS.  Per step j < steps: weights of the current inliers, refit on them
 * (of several five-point solutions the one with the smallest Sampson-error sum over the inlier list, early exit tested every 4th list
 * position), every point's Sampson L2 error on bearing vectors against th_mult th^2 - (j + 1) (th_mult th^2 - th^2) / steps; the step is
 * kept when its count is at least (1 - max_loss) times the current one.  One workgroup per problem, all steps in one launch.
 * p1, p2: n x 2 doubles (camera coordinates, host); E[9] in / out; mask: n bytes in / out (nonzero = inlier; out: 0 / 1).
 * Returns 0 (reference: true) with E, mask, *n_inliers and *steps_done (accepted steps; both outputs may be NULL) written;
 * MLPL_E_FAILED (reference: false: fewer than 6 starting inliers, or the first step lost too many) with E and mask untouched.
 * As the reference: a solver nibble of 0 or above 4 ("not supported") and steps = 0 return 0 with E unchanged and the mask made 0 / 1;
 * with PR_NISTER / PR_STEWENIUS, weight bits other than 0x10 / 0x20 run the unweighted solver.
 * Deliberate deviations: PR_KNEIP (0x4) returns MLPL_E_UNSUPPORTED from this entry and its batch form, which carry no R / t (the solver
 * is built: mlpl_refine_essential_linear_rt below); PR_8PT with weight bits other
 * than 0x10 / 0x20 / 0x30 returns MLPL_E_BAD_INPUT (the reference reads uninitialised weights there); a PR_8PT fit on fewer than 8
 * points counts as a failed refit (the reference's assert(n > 7) is compiled out and its null space is not unique).  The method is
 * checked before anything else.  R / t of the reference are the caller's business: with every solver built here a passed R is cleared.
 */
int mlpl_refine_essential_linear(mlpl_ctx *ctx, const double *p1, const double *p2, int n, int method, double th, int steps, double th_mult,
                                 double ph_mult, double max_loss, double E[9], uint8_t *mask, int *n_inliers, int *steps_done);
/* The same for a batch in one launch, in the layout mlpl_ransac / usac / arrsac_essential_batch_dev write: problem b = d_p1 / d_p2 + b * stride * 2
 * doubles (device), counts[b] <= stride of them (host), th[b] (host), E + 9 b (host, in / out), mask at d_masks + b * stride (device, in / out).
 * Outputs per problem (host): status[b] (0 or MLPL_E_FAILED; a failed problem keeps E and mask), n_inliers[b], steps_done[b] (optional).
 * Every problem's result is bit-identical to what mlpl_refine_essential_linear returns for it (the same kernel).  Returns 0 or the
 * call's error (MLPL_E_UNSUPPORTED / MLPL_E_BAD_INPUT as above). */
int mlpl_refine_essential_linear_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts,
                                           const double *th, int method, int steps, double th_mult, double ph_mult, double max_loss, double *E,
                                           uint8_t *d_masks, int32_t *n_inliers, int32_t *status, int32_t *steps_done, void *stream);
/*
 * refineEssentialLinear with R and t: the two entries above plus PR_KNEIP (0x4), OpenGV's eigensolver (Kneip & Lynen) on the current
 * inliers in list order -- the only solver that returns the pose itself (csrc/kneip_refine_impl.h).  Added arguments: R[9] in / out (row
 * major), t[3] out (unit length), *rt_valid in: R holds a start rotation (0 = the reference's empty R) / out: R and t were written -- the
 * reference's rule (pose_linear_refinement.cpp:272-293): at least one step was accepted; otherwise the reference clears R, here R and t
 * stay and *rt_valid is 0.  Without a usable start (rt_valid 0, or R not a rotation by isMatRoationMat) step 0 makes up to 12 attempts from
 * the identity perturbed in Cayley space by (rand() / RAND_MAX - 0.5) * 0.2 per component, rand() being glibc's stream after srand(seed),
 * attempt a using raw values 3 a .. 3 a + 2; an attempt is taken when its count at th^2 is at least (1 - max_loss) times the inliers.
 * *attempts_used (may be NULL): attempts made, 0 when R was the start.  When all 12 fail the reference returns true with E unchanged, the
 * mask made 0 / 1 and R cleared, and so does this (0, steps_done 0, rt_valid 0); the same when the solver rejects step 0 from a given R.
 * Per step: kneip_sums_kernel (the 36 distinct summation terms, bit-identical to the host's dgm::eig_sums), the Levenberg-Marquardt solve
 * on the host (csrc/usac_degen_math.h), kneip_eval_kernel (all candidates of the step in one launch).  The weight bits are accepted and
 * change nothing (OpenGV's useWeights stays false in the reference).  Deviation: with weight bits other than 0x10 / 0x20 the reference sums
 * its zero-padded inlier vector until the first accepted step (n - count copies of correspondence 0); here always the list itself.
 * Solver nibbles other than 0x4 run the kernel of the entries above and clear *rt_valid.  Returns as mlpl_refine_essential_linear;
 * MLPL_E_FAILED leaves every in / out argument untouched.
 */
int mlpl_refine_essential_linear_rt(mlpl_ctx *ctx, const double *p1, const double *p2, int n, int method, double th, int steps, double th_mult,
                                    double ph_mult, double max_loss, double E[9], uint8_t *mask, int *n_inliers, int *steps_done, double R[9], double t[3],
                                    int *rt_valid, uint32_t seed, int *attempts_used);
/* The batch form, in the layout of mlpl_refine_essential_linear_batch_dev: R + 9 b, t + 3 b, rt_valid[b] (host, as above), seeds[b] (host;
 * NULL = 1 for every problem), attempts_used[b] (host, may be NULL).  The batch moves in lockstep over the steps (two launches and two
 * host hops per step); its problems are solved by a few host threads.  Every problem's result is bit-identical to the single entry's. */
int mlpl_refine_essential_linear_rt_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts,
                                              const double *th, int method, int steps, double th_mult, double ph_mult, double max_loss, double *E,
                                              uint8_t *d_masks, int32_t *n_inliers, int32_t *status, int32_t *steps_done, double *R, double *t,
                                              int32_t *rt_valid, const uint32_t *seeds, int32_t *attempts_used, void *stream);
/* Where the last mlpl_refine_essential_linear_rt(_batch_dev) call with solver 0x4 spent its time, seconds: {kneip_sums_kernel,
 * host solves, kneip_eval_kernel, uploads + downloads + synchronisation}.  Measured only while enabled (enable: 1 / 0 / -1 = leave). */
int mlpl_kneip_refine_times(mlpl_ctx *ctx, int enable, double out[4]);
/* mlpl_recover_pose_dev for a batch in the same layout (the batched cheirality step of the pair entries): E + 9 b (host), d_masks NULL (all
 * points) or [n_problems][stride] on the device (in / out: the chosen candidate's mask), n_good[b], R + 9 b, t + 3 b (host).  Every problem's
 * result equals what mlpl_recover_pose_dev returns for it. */
int mlpl_recover_pose_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts,
                                const double *E, double dist, uint8_t *d_masks, int32_t *n_good, double *R, double *t, void *stream);
/* d_matches_out: NULL, or a device block [n_pairs][nq] that receives every pair's match list (out[i].n_matches valid entries each,
 * ascending queryIdx) -- what a caller gathers beside the pose records (needs refit = 0).
 * Statistics of the last mlpl_pair_pose_batch_dev call: {RANSAC passes, pair slots summed over the passes, pairs redone by the
 * single-pair pipeline (a device-evaluated iteration bound differed from the host's libm, or the pair's raw rand() stream ran out on the
 * device), host microseconds spent generating the raw rand() streams (the samples themselves are drawn on the device), essential matrices scored, Sampson evaluations (matrices x correspondences), RANSAC iterations executed, 0}. */
int mlpl_pair_batch_last_stats(mlpl_ctx *ctx, long long stats[8]);

/* Building blocks, exposed for parity tests and for callers that schedule the phases themselves. */
/* 5-point minimal solver, one wavefront per sample: samples = n_samples x 5 indices into p1/p2 (host).
 * E_out: n_samples x 10 x 9 doubles, n_models: n_samples ints (host). Replaces run5Point (five-point.cpp:366-471). */
int mlpl_solve_5pt(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const int32_t *samples, int n_samples,
                   double *E_out, int32_t *n_models);
/* Sampson scoring of n_models 3x3 matrices against n correspondences: count[i] = #{err <= thresh^2},
 * err_sum[i] = sum of the float-rounded errors (findInliers + cv::sum(err), modelest.cpp:69-83,407). */
int mlpl_score_models(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const double *E, int n_models,
                      double thresh, int32_t *count, double *err_sum);

/* Inlier counts only, by the division-free predicate the RANSAC passes use (exactly (double)(float)(N / D) <= thresh2, see
 * sampson_inlier in ransac_5pt.hip); thresh2 is the SQUARED threshold as the reference holds it (modelest.cpp:79).
 * shape: 0 = automatic, 1 = 4-lanes-per-model kernel, 2 = block-per-model kernel (for tests). */
int mlpl_count_models(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const double *E, int n_models, double thresh2, int shape,
                      int32_t *count);

/* Median of the float Sampson errors per model, as runLMeDS takes it (modelest.cpp:540-544: errors sorted as int bit patterns;
 * even n: float sum of the two middle values * 0.5).  median: n_models doubles (host). */
int mlpl_median_models(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const double *E, int n_models, double *median);

/* Statistics of the last mlpl_ransac_essential[_dev] call on this context: {iterations executed, essential matrices
 * scored}.  Used by bench.py to turn the scoring kernel's time into algorithmic FLOP/s. */
int mlpl_ransac_last_stats(mlpl_ctx *ctx, long long stats[2]);




/* ---- cheirality / pose recovery --------------------------------------------------------------------------
 * Replaces poselib::getPoseTriangPts (P/source/pose_estim.cpp:913-946) = recoverPose
 * (five-point.cpp:150-338) with t_only empty: decomposeEssentialMat (:340-352), four triangulations,
 * masks z*w>0, (P*Q)z*w>0, z<dist, AND with mask_inout (NULL = all ones), candidate choice by the
 * reference's if-chain.  R: 9, t: 3, Q: n x 3 doubles, mask_inout: n bytes (nonzero = keep; rewritten as
 * 0/255 like the reference's comparison masks).  Returns the number of good points (>=0) or a negative error.
 */
int mlpl_recover_pose(mlpl_ctx *ctx, const double E[9], const double *p1, const double *p2, int n, double dist,
                      double R[9], double t[3], double *Q, uint8_t *mask_inout);
/* The same with `t_only` given (getPoseTriangPts(..., translatE = true), five-point.cpp:178-193): R = I and only the two
 * candidates [I|t], [I|-t] compete.  t_only = getTfromTransEssential(E) (P/source/pose_helper.cpp:422-433). */
int mlpl_recover_pose_translation(mlpl_ctx *ctx, const double t_only[3], const double *p1, const double *p2, int n,
                                  double dist, double R[9], double t[3], double *Q, uint8_t *mask_inout);
/* mlpl_recover_pose on device-resident correspondences: d_p1, d_p2 n x 2 doubles, d_Q n x 3 doubles or NULL, d_mask_inout n bytes
 * (nonzero = use; rewritten with the chosen candidate's mask) or NULL -- all device pointers; E, R, t are host.  One host hop:
 * the four candidate counts (five-point.cpp:299-336) decide whose outputs are kept.  Returns the number of valid 3-D points. */
int mlpl_recover_pose_dev(mlpl_ctx *ctx, const double E[9], const double *d_p1, const double *d_p2, int n, double dist,
                          double R[9], double t[3], double *d_Q, uint8_t *d_mask_inout, void *stream);

/* Triangulation with a GIVEN pose: poselib::triangPts3D (P/source/pose_estim.cpp:964-1044), P0 = [I|0], P1 = [R|t].  Per correspondence
 * the DLT null vector X of mlpl_recover_pose (unit norm), then m = ((P1 X).z * X.w > 0) & mask, Q = X.xyz / X.w by division,
 * m &= (Q.z < dist) & (Q.z > 0): both comparisons on the quotient, so that X.w = 0 (inf / NaN) fails them, as in the reference.
 * R: 9, t: 3 (host); Q: n x 3 doubles or NULL, written for EVERY point, masked or not; mask_inout: n bytes or NULL (= all points), rewritten
 * as in & (m ? 255 : 0).  Returns the number of points that pass (>= 0) or a negative error.  With Q NULL a point outside the incoming mask
 * is not triangulated at all.  (The reference returns -1 without Q after it has updated the mask; that rule lives in the C++ drop-in.) */
int mlpl_triang_pts3d(mlpl_ctx *ctx, const double R[9], const double t[3], const double *p1, const double *p2, int n, double dist, double *Q,
                      uint8_t *mask_inout);
/* The same on device-resident correspondences (d_p1, d_p2: n x 2 doubles; d_Q: n x 3 doubles or NULL; d_mask_inout: n bytes or NULL);
 * only the count is read back. */
int mlpl_triang_pts3d_dev(mlpl_ctx *ctx, const double R[9], const double t[3], const double *d_p1, const double *d_p2, int n, double dist,
                          double *d_Q, uint8_t *d_mask_inout, void *stream);
/* A batch in the layout of mlpl_recover_pose_batch_dev (it chains behind mlpl_refine_essential_linear_rt_batch_dev): R + 9 b, t + 3 b
 * (host), d_masks NULL or [n_problems][stride] (in / out; bytes beyond counts[b] untouched), d_Q NULL or [n_problems][stride][3],
 * n_good[b] (host).  One launch for the whole batch; every problem's mask, count and points are bit-identical to mlpl_triang_pts3d's. */
int mlpl_triang_pts3d_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts,
                                const double *R, const double *t, double dist, uint8_t *d_masks, double *d_Q, int32_t *n_good, void *stream);

/* Bundle adjustment of one stereo pair: poselib::refineStereoBA with pointsInImgCoords == false (P/source/pose_estim.cpp:1083-1206, :1294-1348) --
 * motion and structure, calibrated cameras, the first camera fixed, the pseudo-Huber cost, no covariances; SBAdriver::perform_sba
 * (P/source/BA_driver.cpp:1878-2260) around sba_motstr_levmar_x (sba-1.6/sba_levmar.c:449-1400) restated in float64 (tests/ba_oracle.py is
 * the restatement; it is not pinned against an SBA build).  p1, p2: n x 2 in CAMERA coordinates; mask: NULL or n bytes (nonzero = use);
 * R[9], t[3]: in / out; Q: n x 3, in / out; th: the Huber threshold in CAMERA units, ALREADY converted
 * (4 th_px / (sqrt(2) (K1(1,1) + K1(2,2) + K2(1,1) + K2(2,2))), the reference's indices; the C++ drop-in converts); info: NULL or the
 * optimiser's info[0..9] (sba_levmar.c:1377-1400; all zero when the optimiser refuses the problem: fewer than 12 valid points, i.e. fewer
 * measurements than unknowns, or its "almost singular" return).  Returns 1 = accepted (R, t -- normalised when | |t| - 1 | > 1e-4 -- and the
 * valid rows of Q refined), 0 = rejected (|rotation change| > angle_thresh degrees, translation change > t_norm_thresh, stop reason > 5) or
 * failed: R, t and Q untouched; negative: an MLPL_E_* error.  One launch: the whole Levenberg-Marquardt iteration runs in one workgroup. */
int mlpl_refine_stereo_ba(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const uint8_t *mask, double R[9], double t[3], double *Q,
                          double th, double angle_thresh, double t_norm_thresh, double info[10]);
/* The same on device-resident d_p1, d_p2 (n x 2), d_Q (n x 3, in / out), d_mask (n bytes or NULL); only the pose and info are read back. */
int mlpl_refine_stereo_ba_dev(mlpl_ctx *ctx, const double *d_p1, const double *d_p2, int n, const uint8_t *d_mask, double R[9], double t[3],
                              double *d_Q, double th, double angle_thresh, double t_norm_thresh, double info[10], void *stream);
/* A batch in the layout of mlpl_triang_pts3d_batch_dev, behind which it chains: d_p1 / d_p2 + b stride 2, counts[b], d_masks NULL or
 * [n_problems][stride], d_Q [n_problems][stride][3] (in / out; rows outside the mask and beyond counts[b] untouched), host R + 9 b, t + 3 b
 * (in / out), th[b], accepted[b] (1 / 0 as above; a problem without a valid point gives 0), info + 10 b (or NULL).  One launch, one workgroup
 * per problem; every problem's result is bit-identical to mlpl_refine_stereo_ba's.  Returns 0 or a negative error. */
int mlpl_refine_stereo_ba_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p1, const double *d_p2, int stride, const int32_t *counts,
                                    const uint8_t *d_masks, double *d_Q, double *R, double *t, const double *th, double angle_thresh,
                                    double t_norm_thresh, int32_t *accepted, double *info, void *stream);

/* Bundle adjustment of m cameras over one shared structure: poselib::refineMultCamBA with pointsInImgCoords == false and optimMotionOnly ==
 * false (P/source/pose_estim.cpp:1384-1735) -- motion and structure, calibrated cameras, the FIRST camera fixed at the pose given, a
 * visibility map per camera, the pseudo-Huber cost; SBAdriver::perform_sba (nconstframes = 1) around sba_motstr_levmar_x (mcon = 1) restated
 * in float64 (tests/ba_multicam_oracle.py is the restatement; mlpl_refine_stereo_ba is its two-camera, full-visibility special case).  The
 * layout is DENSE, not the reference's compacted lists (the C++ drop-in expands them): p: m x n x 2 in CAMERA coordinates, read where vis is
 * nonzero; vis: m x n bytes; R: m x 9, t: m x 3, in / out; Q: n x 3, in / out; th: the Huber threshold in CAMERA units, ALREADY converted
 * (th_px / mean_j((K_j(1,1) + K_j(2,2)) / 2), the reference's indices; the C++ drop-in converts); info: NULL or the optimiser's info[0..9]
 * (all zero when the optimiser refuses the problem: fewer measurements than unknowns, 2 nvis < 6 m + 3 n, or its "almost singular" return).
 * 2 <= m <= MLPL_BA_MAX_CAMS; a larger m returns MLPL_E_UNSUPPORTED, m < 2 MLPL_E_BAD_INPUT, and nothing is written.  Returns 1 = accepted:
 * Q replaced whole (a point no camera sees keeps its coordinates), every R_j -- camera 0 included -- rewritten as quatToMatrix of its
 * normalised, sign-fixed quaternion, every t_j as the optimiser left it (NOT normalised); 0 = rejected (any camera's |rotation change| >
 * angle_thresh degrees or translation change, both translations normalised, > t_norm_thresh; stop reason > 5) or failed: R, t and Q
 * untouched; negative: an MLPL_E_* error.  vis is never written.  One launch: the whole Levenberg-Marquardt iteration runs in one workgroup. */
#define MLPL_BA_MAX_CAMS 16
int mlpl_refine_multicam_ba(mlpl_ctx *ctx, const double *p, const uint8_t *vis, int m, int n, double *R, double *t, double *Q, double th,
                            double angle_thresh, double t_norm_thresh, double info[10]);
/* The same on device-resident d_p (m x n x 2), d_vis (m x n bytes), d_Q (n x 3, in / out); the poses stay on the host; only they and info are
 * read back. */
int mlpl_refine_multicam_ba_dev(mlpl_ctx *ctx, const double *d_p, const uint8_t *d_vis, int m, int n, double *R, double *t, double *d_Q,
                                double th, double angle_thresh, double t_norm_thresh, double info[10], void *stream);
/* A batch: problem b has n_cams[b] <= cams_stride cameras and counts[b] <= stride points; d_p [n_problems][cams_stride][stride][2], d_vis
 * [n_problems][cams_stride][stride], d_Q [n_problems][stride][3] (in / out), host R [n_problems][cams_stride][9], t
 * [n_problems][cams_stride][3] (in / out), th[b], accepted[b] (1 / 0 as above), info + 10 b (or NULL).  Points beyond counts[b], cameras
 * beyond n_cams[b] and the visibility bytes are never written.  counts[b] == 0 or n_cams[b] < 2: not accepted, info zero, nothing touched;
 * an n_cams[b] > MLPL_BA_MAX_CAMS fails the call with MLPL_E_UNSUPPORTED before anything runs.  One launch, one workgroup per problem; every
 * problem's result is bit-identical to mlpl_refine_multicam_ba's.  Returns 0 or a negative error. */
int mlpl_refine_multicam_ba_batch_dev(mlpl_ctx *ctx, int n_problems, const double *d_p, const uint8_t *d_vis, int cams_stride, int stride,
                                      const int32_t *n_cams, const int32_t *counts, double *d_Q, double *R, double *t, const double *th,
                                      double angle_thresh, double t_norm_thresh, int32_t *accepted, double *info, void *stream);


/* The diagnostics entry points (mlpl_debug_*: traces, clock stamps, solver statistics, self-tests -- exported by the same library, used by
 * the tests and by bench.py, not part of the drop-in surface) are declared in mlpl_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* MLPL_C_H */
