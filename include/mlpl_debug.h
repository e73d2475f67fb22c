/*
 * mlpl_debug.h -- diagnostics entry points of libmlpl_hip.so (traces, clock stamps, solver statistics, self-tests).
 *
 * Exported by the same shared library as the C ABI in mlpl_c.h, but NOT part of the drop-in surface: nothing in the reference corresponds
 * to them and no integration needs them.  The parity tests (tests/), the tools under tools/ and bench.py's clock passes use them.
 * They may change between versions.
 */
#ifndef MLPL_DEBUG_H
#define MLPL_DEBUG_H
#include "mlpl_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostics: the following mlpl_arrsac_essential* calls record the turns of their first stage into buf (20 ints per turn: k, inner-RANSAC
 * turn?, sample size, its first five indices, valid models, per model 1000 * accepted + inliers seen by the sequential test, sixth + 100 * seventh index); returns the
 * number of ints written since the previous call of this function.  buf = NULL switches the recording off. */
int mlpl_debug_arrsac_trace(mlpl_ctx *ctx, int32_t *buf, int cap);

/* Diagnostics: the following mlpl_usac_essential* calls record their decisions into buf, 16 doubles per record: [0] type -- 1 sample
 * {hypothesis, 5 indices, solutions (-1 = rejected by pre-validation)}, 2 evaluation {hypothesis, model, start position in the evaluation
 * order, inliers seen, correspondences tested, accepted, delta, epsilon, decision threshold, squared inlier threshold, local
 * optimisations so far}, 3 refined model {hypothesis, points, weighted, 1, model[9]}, 4 model stored {hypothesis, model, inliers},
 * 5 minimal model {hypothesis, index, model[9]}, 6 model rejected by the oriented constraint {hypothesis, index}, 7 degeneracy test
 * {hypothesis, degenerate, upgrade, type, inliers of the rotation, of "no motion", of the best model}, 8 rotation evaluated on all
 * correspondences {hypothesis, pair of the sample, inliers of the two-point rotation, of its refit, stored}, 9 upgrade {hypothesis,
 * 1 = no motion -> t / 2 = R -> R + t, candidates tried, best inlier count}, 10 upgrade candidate {hypothesis, branch, number, t[3] or
 * E[9]}; evaluations of translation candidates are type 2 with model -1 and the angular threshold.  Returns the number of
 * records produced since the previous call of this function (may exceed cap: only cap are written).  buf = NULL switches it off. */
int mlpl_debug_usac_trace(mlpl_ctx *ctx, double *buf, int cap_records);

/* Diagnostics of the device-side sampling of large RANSAC passes (option "ransac_device_draw", default 1: passes of >= 4096 hypotheses on
 * >= 64 correspondences draw their samples on the device from the cached raw rand() stream): {calls redone with the host drawing the table
 * because a window / list / the stream ran out, 1 if the last call's samples were drawn on the device}. */
int mlpl_debug_ransac_draw(mlpl_ctx *ctx, long long out[2]);

/* The run scheduler of the batched sequential estimators by itself (csrc/batch_hub.h: fibers on worker threads, futex hand-over), no GPU
 * and no context needed: n fibers on `workers` threads pass `rounds` times through the hand-over against a stand-in hub on the calling
 * thread.  Returns n * rounds, or a negative value on bad arguments / a fiber that was not released exactly once per round. */
long long mlpl_debug_fiber_selftest(int n, int workers, int rounds);

/* The guard every entry carries against C++ exceptions by itself, no GPU and no context needed: a guarded body that returns 7 (kind 0),
 * throws std::bad_alloc (kind 1: MLPL_E_NOMEM comes back), a std::runtime_error (kind 2: MLPL_E_INTERNAL, mlpl_last_error() carries its
 * what()) or an int (kind 3: MLPL_E_INTERNAL). */
int mlpl_debug_entry_guard(int kind);

/* The two eigen-solvers of the re-weighted 9 x 9 fits on `count` symmetric matrices G[count][81] (tests): out12[count][12] = {steps of the
 * inverse iteration (0: it did not settle and the caller would take the Jacobi path), x^T G x, 0, x[9]}; jacobi10[count][10] = {smallest
 * eigenvalue, its eigenvector} of the full Jacobi decomposition; start[count][9] (may be NULL) = start vectors of the inverse iteration. */
int mlpl_debug_eig9(mlpl_ctx *ctx, const double *G, const double *start, int count, double *out12, double *jacobi10);

/* Diagnostics: root-iteration (Ehrlich-Aberth) sweep statistics of the solver since the last call: {sum, solves, max, (enabled), sample
 * index of the max, solves with <= 8, 12, 16, 24, 32, 64, 128, 256, < 400, = 400 sweeps, 0}; enable != 0 turns the (atomic) bookkeeping on.
 * Not for production use. */
int mlpl_debug_dk_stats(mlpl_ctx *ctx, int enable, int stats[16]);

/* Diagnostics: the four flag words of the float L2 paths after the calls enqueued so far have finished (synchronises the device):
 * {generation of the last call whose data were not integer-valued (int8 preparation), generation of the last fp16-path call with a row
 * outside that path's range, number of queries the fp16 path re-ranked against every train row since the flag block was created,
 * generation of the last fp16-path call whose data were not integer-valued}. */
int mlpl_debug_l2_flags(mlpl_ctx *ctx, int flags[4]);

/* Diagnostics: with option "hamming_stamps" = 1 every wave of the matrix-core Hamming kernel records {shader-clock cycles, 100 MHz
 * real-time ticks, 32x32 tiles processed, start tick}; this copies up to max_items records of 4 x u64 of the LAST launch to `out`
 * and returns their number.  In-kernel clock = cycles / ticks * 100 MHz.  Not for production use. */
int mlpl_debug_hamming_stamps(mlpl_ctx *ctx, unsigned long long *out, int max_items);

/* Diagnostics: with option "hamming_stamps" = 2 every launch of the static LDS-ring Hamming kernel leaves ONE record {shader-clock
 * cycles, 100 MHz ticks, start tick, launch number} of the lifetime of its first workgroup in a ring of 256 launches (one 32-byte store
 * per launch; nothing else changes).  Copies the records of the last min(max_items, 256, launches so far) launches, oldest first, and
 * returns their number (synchronises the device).  Shader clock of a launch = cycles / ticks * 100 MHz. */
int mlpl_debug_hamming_clock(mlpl_ctx *ctx, unsigned long long *out, int max_items);

/* Diagnostics: the host-hop timeline of the last mlpl_pair_pose_batch_dev / mlpl_ransac_essential_batch_dev call of this context:
 * us[i] = microseconds since the call's entry, codes[i] = 1 matching enqueued, 2 match counts back, 3 / 4 a RANSAC pass enqueued / its
 * states back, 5 / 6 pose step enqueued / back; *ws_grows = workspace blocks (re)allocated by this context so far.  Returns the number
 * of entries written (<= max_items). */
int mlpl_debug_hop_trace(mlpl_ctx *ctx, float *us, int *codes, int max_items, long long *ws_grows);

/* Diagnostics: the kernel instances the last launches chose (tests check that an option reached the instance it names).  Writes 13 ints
 * and returns 13:
 *   out[0]  instance of the last inlier-count pass (RANSAC pass, pair batch, mlpl_count_models, mlpl_debug_count_pass; 0 = none yet):
 *           1 score_models_block_kernel<count> (one workgroup per model), 2 score_models_kernel<fp64, 512 threads>,
 *           3 score_models_kernel<fp64, 128 threads, 256-point tiles> (passes of <= 24576 models), 4 count_models_f32_kernel<128, 256>
 *           (the same passes, packed-fp32 filter), 5 count_models_f32_kernel<512, 512> (one model per lane), 6 <512, 512, 2 models per
 *           lane>, 7 <512, 512, 2, deferred queue>, 8 <256, 512, 2, deferred, 96 VGPRs> (default), 9 <256, 512, 2, deferred, 80 VGPRs>
 *           (ransac_count_wpe 6), 10 / 11 the block / 4-lane kernels with error sums;
 *   out[1]  its workgroups per model group (point splits; 0 for the block kernel);
 *   out[2]  Hamming kernel of the last knn_hamming call: 0 / 1 / 2 VALU kernel of hamming_variant 0 / 1 / 2, 3 register-prefetch
 *           matrix-core kernel, 4 static LDS-ring kernel, 5 dynamic-split LDS-ring kernel;
 *   out[3]  query tiles per wave (matrix-core) or queries per lane (VALU);  out[4] PRIO of the static ring kernel (0, 1, 3);
 *   out[5]  waves per workgroup of the static ring kernel (4, 8, 16; 4 for the other matrix-core kernels, 0 VALU);
 *   out[6]  its prefetch distance in tiles (2, 4, 6; 0 otherwise);  out[7] 1 = the kernel merged its splits itself (no merge launch);
 *   out[8]  1 = the age-aware split table was used;  out[9] 1 = the train set was expanded one thread per (tile, K-step, lane);
 *   out[10] train splits;  out[11] 64-bit K-steps of the matrix-core kernels (0 VALU);
 *   out[12] 1 = the static ring kernel expanded the raw train tiles itself (option "hamming_expand_inkernel"; no expansion launch). */
int mlpl_debug_last_kernels(mlpl_ctx *ctx, int out[13]);

/* Diagnostics: the block size of the running top-2 update the last knn_hamming call really used (option "hamming_block_top2"): 4 = the
 * in-kernel-expansion instance of the static ring kernel folded the maxima of blocks of four and re-scored the best row's block in its epilogue,
 * 0 = the per-candidate update (every other kernel, and every call the option does not apply to). */
int mlpl_debug_last_hamming_top2(mlpl_ctx *ctx);

/* Diagnostics: the train rows per block of the instance the last knn_hamming call really ran: 8 = the 16x16x128 form of the throughput instance
 * (a block is a lane's eight accumulator registers of a tile: rows T + 16 h + 4 g + i, h < 2, i < 4), 4 = the 32x32x64 in-kernel-expansion
 * instances with "hamming_block_top2" = 4 (aligned groups of four rows), 0 = the per-candidate update.  The option and
 * mlpl_debug_last_hamming_top2 keep their values (0 | 4) and their meaning: block maxima in the loop. */
int mlpl_debug_last_hamming_block_rows(mlpl_ctx *ctx);

/* Diagnostics: the matrix-core shape the last knn_hamming call really used (option "hamming_mfma_shape"): 16 = the 16x16x128 form of the
 * throughput instance of the static ring kernel, 32 = every other matrix-core kernel (and every call the option does not apply to), 0 = a
 * VALU kernel. */
int mlpl_debug_last_hamming_shape(mlpl_ctx *ctx);

/* Diagnostics: what the last float knn / match call of this context (mlpl_knn2_l2sq_f32*, mlpl_match_l2_dev, the float pair entries)
 * chose.  Writes 4 ints and returns 4: out[0] path -- 1 exact fp32 kernel, 2 int8 matrix-core path (forced), 3 the auto path's fused
 * kernel (int8 or exact by the device flag), 4 fp16 candidate path, 0 nothing launched (nq = 0); out[1] train splits the fold reads
 * (auto: the larger of the two tables; 0 on the fp16 path); out[2] 1 = the fold kernel produced the pass counts of the ratio test
 * (mlpl_match_l2_dev with option "l2_fold_counts"); out[3] kernel launches of the call (memsets and copies not counted). */
int mlpl_debug_last_l2_match(mlpl_ctx *ctx, int out[4]);

/* Tests: the float knn with the fused fold alone (no ratio_write_kernel behind it), on the context's own stream: d_idx / d_dist as
 * mlpl_knn2_l2sq_f32_dev writes them, counts[batch][ceil(nq / 64)] (host) = the pass counts of the ratio predicate per group of 64
 * queries as knn_l2_fold_ratio_kernel stored them (-1: a group no workgroup wrote).  Returns the number of counts, 0 when the path taken
 * has no fold (the fp16 candidate path), or a negative error.  Arguments as mlpl_match_l2_dev; the inputs must be complete on the device. */
int mlpl_debug_l2_fold_counts(mlpl_ctx *ctx, const float *d_q, int nq, size_t q_stride, size_t q_batch_stride, const float *d_t, int nt,
                              size_t t_stride, size_t t_batch_stride, int dim, int ratio_test, float ratio, int batch, int32_t *d_idx, float *d_dist,
                              int32_t *counts);

/* Tests: one count-only scoring pass exactly as a RANSAC pass runs it.  The correspondences are packed as for RANSAC; E holds n_live
 * models (9 doubles each), padded on the device to n_bound rows with NaN models; the live count n_live is read on the device; the count
 * of live model m goes to table_inout[ids ? ids[m] : m] (table_len ints, uploaded as given and read back: slots no id names keep their
 * contents).  point_splits: -1 = what a RANSAC pass of n_bound models would take, 0 = one workgroup per model (stores), 1 = one workgroup
 * per model group (stores), > 1 = that many workgroups per model group, which ADD to the table.  The instance follows the context's
 * ransac_count_* / ransac_f32_filter options (mlpl_debug_last_kernels reports it). */
int mlpl_debug_count_pass(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const double *E, int n_live, int n_bound,
                          const int32_t *ids, int table_len, double thresh2, int point_splits, int32_t *table_inout);

/* Tests: the damping term mu at exit of every problem of the calling thread's last mlpl_refine_stereo_ba* call (0 for a problem the optimiser
 * refused).  Writes min(problems, max_items) doubles and returns that number. */
int mlpl_debug_ba_last_mu(double *mu, int max_items);
/* The same for the calling thread's last mlpl_refine_multicam_ba* call. */
int mlpl_debug_ba_multicam_last_mu(double *mu, int max_items);

#ifdef __cplusplus
}
#endif
#endif /* MLPL_DEBUG_H */
