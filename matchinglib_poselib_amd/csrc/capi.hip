// capi.hip -- context management and the host-pointer entry points of the C ABI (include/mlpl_c.h).
// Every compute path here ends in a HIP kernel launch; there is no CPU fallback.

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>

#include "mlpl_internal.h"

namespace mlpl {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int entry_failed(const char *who) noexcept {
    try {
        throw;
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory", who);
        return MLPL_E_NOMEM;
    } catch (const std::exception &e) {
        set_error("%s: C++ exception: %s", who, e.what());
    } catch (...) {
        set_error("%s: C++ exception of an unknown type", who);
    }
    return MLPL_E_INTERNAL;
}

bool counts_in_range(const char *who, int n_problems, const int32_t *counts, int lo, int stride) {
    for (int b = 0; b < n_problems; ++b)
        if (counts[b] < lo || counts[b] > stride) {
            set_error("%s: counts[%d] = %d outside [%d, stride = %d]", who, b, counts[b], lo, stride);
            return false;
        }
    return true;
}

int upload_points(mlpl_ctx *ctx, const double *p1, const double *p2, int n, const double **d_p1, const double **d_p2, size_t match_bytes,
                  void **d_match) {
    const size_t bytes = (size_t)std::max(n, 1) * 16;
    void *a, *b;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, bytes, &a))) return rc;
    if ((rc = ws_get(ctx, WS_AUX1, bytes, &b))) return rc;
    if (match_bytes && (rc = ws_get(ctx, WS_MATCH, match_bytes, d_match))) return rc;
    if (n > 0) {
        MLPL_HIP_TRY(hipMemcpyAsync(a, p1, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
        MLPL_HIP_TRY(hipMemcpyAsync(b, p2, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    }
    *d_p1 = (const double *)a, *d_p2 = (const double *)b;
    return MLPL_OK;
}

int download_mask(uint8_t *mask, const void *d_mask, int n) {
    if (n > 0) MLPL_HIP_TRY(hipMemcpy(mask, d_mask, (size_t)n, hipMemcpyDeviceToHost));
    return MLPL_OK;
}

int ws_get(mlpl_ctx *ctx, WsSlot slot, size_t bytes, void **out) {
    if (bytes < 4096) bytes = 4096;  // small requests share one minimum size, so they never trigger a regrow
    if (ctx->ws_bytes[slot] < bytes) {
        // growing: make sure nothing in flight still uses the old buffer
        MLPL_HIP_TRY(hipDeviceSynchronize());
        if (ctx->ws[slot]) MLPL_HIP_TRY(hipFree(ctx->ws[slot]));
        ctx->ws[slot] = nullptr;
        ctx->ws_bytes[slot] = 0;
        ctx->ws_grows++;
        size_t want = bytes + bytes / 4;
        want = (want + 255) & ~size_t(255);
        hipError_t e = hipMalloc(&ctx->ws[slot], want);
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
            return MLPL_E_NOMEM;
        }
        ctx->ws_bytes[slot] = want;
    }
    *out = ctx->ws[slot];
    return MLPL_OK;
}

int pinned_get(mlpl_ctx *ctx, size_t bytes, void **out) {
    if (ctx->pinned_bytes < bytes) {
        MLPL_HIP_TRY(hipDeviceSynchronize());
        if (ctx->pinned) MLPL_HIP_TRY(hipHostFree(ctx->pinned));
        ctx->pinned = nullptr;
        ctx->pinned_bytes = 0;
        ctx->ws_grows++;
        size_t want = std::max<size_t>(bytes * 2, 4096);
        hipError_t e = hipHostMalloc(&ctx->pinned, want, hipHostMallocMapped);
        if (e != hipSuccess) {
            set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
            return MLPL_E_NOMEM;
        }
        ctx->pinned_bytes = want;
    }
    *out = ctx->pinned;
    return MLPL_OK;
}

int pinned_batch_get(mlpl_ctx *ctx, size_t bytes, void **out) {
    if (ctx->pinned_batch_bytes < bytes) {
        MLPL_HIP_TRY(hipDeviceSynchronize());
        if (ctx->pinned_batch) MLPL_HIP_TRY(hipHostFree(ctx->pinned_batch));
        ctx->pinned_batch = nullptr;
        ctx->pinned_batch_bytes = 0;
        const size_t want = bytes + bytes / 8 + 4096;
        hipError_t e = hipHostMalloc(&ctx->pinned_batch, want, hipHostMallocMapped);
        if (e != hipSuccess) {
            set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
            return MLPL_E_NOMEM;
        }
        ctx->pinned_batch_bytes = want;
    }
    *out = ctx->pinned_batch;
    return MLPL_OK;
}

void prof_mark(mlpl_ctx *ctx, int id, int phase, hipStream_t s) {
    if (!ctx->prof_on) return;
    if (!ctx->prof_ev[id]) return;  // pools are created by mlpl_profile_enable, outside any timed region
    if (ctx->prof_n[id] >= kProfMaxLaunches) return;
    // prof_on = N > 1: bracket every Nth launch only (two event records cost ~10 us of stream time per launch)
    if (phase == 0) ctx->prof_take[id] = (ctx->prof_calls[id]++ % ctx->prof_on) == 0;
    if (!ctx->prof_take[id]) return;
    (void)hipEventRecord(ctx->prof_ev[id][2 * ctx->prof_n[id] + phase], s);
    if (phase == 1) ctx->prof_n[id]++;
}

}  // namespace mlpl

using namespace mlpl;

// The tuning options: one row per opt_* field of mlpl_ctx, and nothing else to keep in step.  mlpl_ctx_create sets the defaults from
// it, mlpl_set_option / mlpl_get_option / mlpl_option_info / mlpl_option_accepts look a name up in it, tests/option_guard.py takes its
// names from it.  A value is accepted if lo <= value <= hi and `ok`, where a row has one, holds (the value sets that are no range).
namespace {

struct Option {
    const char *name;
    int mlpl_ctx::*field;
    int def, lo, hi;
    bool (*ok)(int) = nullptr;
};
const int kAnyCount = 0x7fffffff;   // hi of an option that takes every non-negative int
const Option kOptions[] = {
    {"l2_fold_counts", &mlpl_ctx::opt_l2_fold_counts, 1, 0, 1},
    {"hamming_expand_inkernel", &mlpl_ctx::opt_hamming_expand_inkernel, 1, 0, 1},   // measured (tools/hamming_opt_ab.py, profiles/README.md): the step loses the expansion pass, the ring kernel gains less
    {"hamming_block_top2", &mlpl_ctx::opt_hamming_block_top2, 4, 0, 4, [](int v) { return v % 4 == 0; }},   // 0 or 4.  Measured (tools/hamming_opt_ab.py, profiles/README.md): the step of 64 C2 pairs loses 15-27 us of 366-380
    {"hamming_mfma_shape", &mlpl_ctx::opt_hamming_mfma_shape, 16, 16, 32, [](int v) { return v % 16 == 0; }},   // 16 or 32 (16 = the 16x16x128 form of the throughput instance: DESIGN 4.1 for the measurement behind the default)
    {"vfc_store_u", &mlpl_ctx::opt_vfc_store_u, 0, 0, 1},   // not measured yet (tools/vfc_timing.py measures both settings)
    {"hamming_variant", &mlpl_ctx::opt_hamming_variant, 3, 0, 3},
    {"hamming_mfma_qt", &mlpl_ctx::opt_hamming_mfma_qt, 0, 0, 4, [](int v) { return v != 3; }},
    {"hamming_mfma_blocks_per_cu", &mlpl_ctx::opt_hamming_mfma_blocks_per_cu, 3, 1, 64},
    {"hamming_mfma_lds", &mlpl_ctx::opt_hamming_mfma_lds, 1, 0, 2},
    {"hamming_expand_fine", &mlpl_ctx::opt_hamming_expand_fine, 1, 0, 1},
    {"hamming_mfma_prio", &mlpl_ctx::opt_hamming_mfma_prio, 0, 0, 3, [](int v) { return v != 2; }},
    {"hamming_mfma_prefetch", &mlpl_ctx::opt_hamming_mfma_prefetch, 0, 0, 6, [](int v) { return v % 2 == 0; }},
    {"hamming_split_rows", &mlpl_ctx::opt_hamming_split_rows, 0, 0, 8192, [](int v) { return v % 4096 == 0; }},
    {"hamming_mfma_waves", &mlpl_ctx::opt_hamming_mfma_waves, 0, 0, 16, [](int v) { return v % 4 == 0 && v != 12; }},
    {"hamming_mfma_weighted", &mlpl_ctx::opt_hamming_mfma_weighted, 1, 0, 1},
    {"hamming_fused_merge", &mlpl_ctx::opt_hamming_fused_merge, 1, 0, 1},
    {"hamming_stamps", &mlpl_ctx::opt_hamming_stamps, 0, 0, 2},
    {"hamming_train01", &mlpl_ctx::opt_hamming_train01, 0, 0, 1},
    {"hamming_merge_emit", &mlpl_ctx::opt_hamming_merge_emit, 0, 0, 1},   // measured (tools/single_pair_probe.py): the launch it saves is what the chained look-back costs -- 21.2-22.2 against 20.8-21.4 us
    {"l2_mfma_waves", &mlpl_ctx::opt_l2_mfma_waves, 0, 0, 8, [](int v) { return v % 4 == 0; }},
    {"l2_mfma_blocks_per_cu", &mlpl_ctx::opt_l2_mfma_blocks_per_cu, 0, 0, 16},
    {"hamming_qpl", &mlpl_ctx::opt_hamming_qpl, 1, 1, 2},
    {"hamming_blocks_per_cu", &mlpl_ctx::opt_hamming_blocks_per_cu, 32, 1, 64},
    {"ransac_lazy_sums", &mlpl_ctx::opt_ransac_lazy_sums, 1, 0, 1},
    {"ransac_overlap", &mlpl_ctx::opt_ransac_overlap, 1, 0, 1},
    {"ransac_dev_split", &mlpl_ctx::opt_ransac_dev_split, 0, 0, 900},
    {"rand_cache_max", &mlpl_ctx::opt_rand_cache_max, 0, 0, kAnyCount},
    {"ransac_f32_filter", &mlpl_ctx::opt_ransac_f32_filter, 1, 0, 1},
    {"arrsac_refine_warm_start", &mlpl_ctx::opt_arrsac_refine_warm_start, 1, 0, 1},
    {"ransac_count_mpl", &mlpl_ctx::opt_ransac_count_mpl, 2, 1, 2},
    {"ransac_count_tiles", &mlpl_ctx::opt_ransac_count_tiles, 2, 1, 2},
    {"ransac_count_threads", &mlpl_ctx::opt_ransac_count_threads, 256, 256, 512, [](int v) { return v % 256 == 0; }},   // round 6: 4-wave workgroups at 96 VGPRs, five per CU (C5 counting -6-8 %, C3 equal)
    {"ransac_count_wpe", &mlpl_ctx::opt_ransac_count_wpe, 5, 5, 6},
    {"ransac_count_defer", &mlpl_ctx::opt_ransac_count_defer, 1, 0, 1},
    {"ransac_event_cap", &mlpl_ctx::opt_ransac_event_cap, 0, 0, 1024},
    {"solver_polish", &mlpl_ctx::opt_solver_polish, 1, 0, 1},   // the solver's accuracy safeguard stays on: measured CLOSER to the CPU path than the plain root path (tools/polish_default_ab.py)
    {"solver_wave3", &mlpl_ctx::opt_solver_wave3, 1, 0, 1},
    {"ransac_device_draw", &mlpl_ctx::opt_ransac_device_draw, 1, 0, 1},
    {"l2_float_mfma", &mlpl_ctx::opt_l2_float_mfma, 1, 0, 2},
    {"arrsac_flag_points", &mlpl_ctx::opt_arrsac_flag_points, 0, 0, 1024, [](int v) { return v == 0 || (v >= 128 && v % 64 == 0); }},
    {"pair_batch", &mlpl_ctx::opt_pair_batch, 0, 0, 1024},
    {"hub_lanes", &mlpl_ctx::opt_hub_lanes, 0, 0, 8},
    {"eig_inverse_iteration", &mlpl_ctx::opt_eig_inverse_iteration, 1, 0, 1},
    {"hub_blocking_sync", &mlpl_ctx::opt_hub_blocking_sync, 1, 0, 1},
    {"hub_workers", &mlpl_ctx::opt_hub_workers, 0, 0, 64},
    {"hub_cohort", &mlpl_ctx::opt_hub_cohort, 0, 0, 512, [](int v) { return v == 0 || v >= 8; }},
    {"pair_batch_seq", &mlpl_ctx::opt_pair_batch_seq, 0, 0, 1024},
    {"pair_batch_feed", &mlpl_ctx::opt_pair_batch_feed, 1, 0, 1},
    {"pair_batch_raw_cap", &mlpl_ctx::opt_pair_batch_raw_cap, 0, 0, 1 << 22, [](int v) { return v == 0 || v >= 64; }},
    {"usac_lo_stepwise", &mlpl_ctx::opt_usac_lo_stepwise, 0, 0, 1},
    {"usac_lo_warm_start", &mlpl_ctx::opt_usac_lo_warm_start, 1, 0, 1},
    {"usac_first_batch", &mlpl_ctx::opt_usac_first_batch, 0, 0, 128},
    {"usac_lo5_fused_fit", &mlpl_ctx::opt_usac_lo5_fused_fit, 1, 0, 1},
    {"usac_sprt_fast", &mlpl_ctx::opt_usac_sprt_fast, 1, 0, 1},
    {"ransac_host_table", &mlpl_ctx::opt_ransac_host_table, 0, 0, 1},
    {"ransac_chunk", &mlpl_ctx::opt_ransac_chunk, 0, 0, 32768},
};

const Option *find_option(const char *name) {
    for (const Option &o : kOptions)
        if (!std::strcmp(name, o.name)) return &o;
    return nullptr;
}

bool option_accepts(const Option &o, int value) { return value >= o.lo && value <= o.hi && (!o.ok || o.ok(value)); }

}  // namespace

extern "C" {

const char *mlpl_last_error(void) { return g_err; }
const char *mlpl_version(void) { return "mlpl-hip 0.1 (gfx950)"; }

int mlpl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mlpl_ctx_create(int device_ordinal, mlpl_ctx **out) try {
    if (!out) return MLPL_E_BAD_INPUT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device visible: this library has no CPU fallback");
        return MLPL_E_NO_DEVICE;
    }
    if (device_ordinal < 0 || device_ordinal >= n) {
        set_error("device ordinal %d out of range [0,%d)", device_ordinal, n);
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    MLPL_HIP_TRY(hipGetDeviceProperties(&prop, device_ordinal));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this library carries gfx950 code objects only", device_ordinal, prop.gcnArchName);
        return MLPL_E_NO_DEVICE;
    }
    mlpl_ctx *ctx = new (std::nothrow) mlpl_ctx();
    if (!ctx) return MLPL_E_NOMEM;
    std::memset(ctx, 0, sizeof(*ctx));
    ctx->device = device_ordinal;
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    for (const Option &o : kOptions) ctx->*(o.field) = o.def;
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        delete ctx;
        return MLPL_E_HIP;
    }
    e = hipStreamCreateWithFlags(&ctx->aux_stream[0], hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->aux_stream[1], hipStreamNonBlocking);
    for (int i = 0; e == hipSuccess && i < 8; ++i) e = hipEventCreateWithFlags(&ctx->aux_ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        set_error("helper stream / events: %s", hipGetErrorString(e));
        mlpl_ctx_destroy(ctx);
        return MLPL_E_HIP;
    }
    if (int rc = subpix_separate_init(ctx)) {   // the mask profiles of mlpl_subpix_separate*: 768 bytes, so that no entry uploads
        mlpl_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_ctx_create")

void mlpl_ctx_destroy(mlpl_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < WS_NUM_SLOTS; ++i)
        if (ctx->ws[i]) (void)hipFree(ctx->ws[i]);
    for (int k = 0; k < MLPL_PROF_NUM; ++k) {
        if (!ctx->prof_ev[k]) continue;
        for (int i = 0; i < 2 * kProfMaxLaunches; ++i) (void)hipEventDestroy(ctx->prof_ev[k][i]);
        delete[] ctx->prof_ev[k];
    }
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->pinned_batch) (void)hipHostFree(ctx->pinned_batch);
    mlpl::hub_streams_free(ctx->hub_streams);
    if (ctx->l2_hint_host) (void)hipHostFree(ctx->l2_hint_host);
    delete[] ctx->ransac_T_host;
    std::free(ctx->last_usac_flags);
    std::free(ctx->usac_prosac_tab);
    mlpl::free_rand_cache(ctx->rand_cache);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (int i = 0; i < 2; ++i)
        if (ctx->aux_stream[i]) (void)hipStreamDestroy(ctx->aux_stream[i]);
    for (int i = 0; i < 8; ++i)
        if (ctx->aux_ev[i]) (void)hipEventDestroy(ctx->aux_ev[i]);
    delete ctx;
}

void *mlpl_ctx_stream(mlpl_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int mlpl_ctx_device(mlpl_ctx *ctx) { return ctx ? ctx->device : -1; }
int mlpl_ctx_synchronize(mlpl_ctx *ctx) {
    if (!ctx) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MLPL_OK;
}

int mlpl_set_option(mlpl_ctx *ctx, const char *name, int value) {
    if (!ctx || !name) return MLPL_E_BAD_INPUT;
    const Option *o = find_option(name);
    if (!o || !option_accepts(*o, value)) {
        set_error("mlpl_set_option: unknown option or bad value: %s=%d", name, value);
        return MLPL_E_BAD_INPUT;
    }
    ctx->*(o->field) = value;
    return MLPL_OK;
}

int mlpl_get_option(mlpl_ctx *ctx, const char *name, int *value) {
    if (!ctx || !name || !value) return MLPL_E_BAD_INPUT;
    const Option *o = find_option(name);
    if (!o) {
        set_error("mlpl_get_option: unknown option: %s", name);
        return MLPL_E_BAD_INPUT;
    }
    *value = ctx->*(o->field);
    return MLPL_OK;
}

int mlpl_option_info(int index, const char **name, int *default_value) {
    const int count = (int)(sizeof(kOptions) / sizeof(kOptions[0]));
    if (index < 0 || index >= count || !name || !default_value) return MLPL_E_BAD_INPUT;
    *name = kOptions[index].name;
    *default_value = kOptions[index].def;
    return MLPL_OK;
}

int mlpl_option_accepts(const char *name, int value) {
    const Option *o = name ? find_option(name) : nullptr;
    return o ? (int)option_accepts(*o, value) : MLPL_E_BAD_INPUT;
}

int mlpl_debug_last_kernels(mlpl_ctx *ctx, int out[13]) {
    if (!ctx || !out) return MLPL_E_BAD_INPUT;
    out[0] = ctx->dbg_count_kernel[0], out[1] = ctx->dbg_count_kernel[1];
    for (int i = 0; i < 11; ++i) out[2 + i] = ctx->dbg_hamming_kernel[i];
    return 13;
}

int mlpl_debug_last_hamming_top2(mlpl_ctx *ctx) { return ctx ? ctx->dbg_hamming_top2 : MLPL_E_BAD_INPUT; }
int mlpl_debug_last_hamming_shape(mlpl_ctx *ctx) { return ctx ? ctx->dbg_hamming_shape : MLPL_E_BAD_INPUT; }
int mlpl_debug_last_hamming_block_rows(mlpl_ctx *ctx) { return ctx ? ctx->dbg_hamming_block_rows : MLPL_E_BAD_INPUT; }

int mlpl_debug_last_l2_match(mlpl_ctx *ctx, int out[4]) {
    if (!ctx || !out) return MLPL_E_BAD_INPUT;
    for (int i = 0; i < 4; ++i) out[i] = ctx->dbg_l2_match[i];
    return 4;
}

int mlpl_debug_hamming_stamps(mlpl_ctx *ctx, unsigned long long *out, int max_items) try {
    if (!ctx || !out) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    MLPL_HIP_TRY(hipDeviceSynchronize());
    // max_items < 0: the per-tile trace that follows the records (48 u64 per wave), -max_items waves at most
    if (max_items < 0) {
        const int n = ctx->dbg_stamp_items < -max_items ? ctx->dbg_stamp_items : -max_items;
        if (n > 0 && ctx->ws[WS_DEBUG])
            MLPL_HIP_TRY(hipMemcpy(out, (char *)ctx->ws[WS_DEBUG] + (size_t)ctx->dbg_stamp_items * 32, (size_t)n * 48 * 8, hipMemcpyDeviceToHost));
        return n;
    }
    const int n = ctx->dbg_stamp_items < max_items ? ctx->dbg_stamp_items : max_items;
    if (n > 0 && ctx->ws[WS_DEBUG]) MLPL_HIP_TRY(hipMemcpy(out, ctx->ws[WS_DEBUG], (size_t)n * 32, hipMemcpyDeviceToHost));
    return n;
} MLPL_ENTRY_END("mlpl_debug_hamming_stamps")

int mlpl_debug_hop_trace(mlpl_ctx *ctx, float *us, int *codes, int max_items, long long *ws_grows) {
    if (!ctx) return MLPL_E_BAD_INPUT;
    const int n = ctx->hop_n < max_items ? ctx->hop_n : max_items;
    for (int i = 0; i < n; ++i) {
        if (us) us[i] = ctx->hop_us[i];
        if (codes) codes[i] = ctx->hop_code[i];
    }
    if (ws_grows) *ws_grows = ctx->ws_grows;
    return n;
}

int mlpl_debug_hamming_clock(mlpl_ctx *ctx, unsigned long long *out, int max_items) try {
    if (!ctx || !out || max_items < 0) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    MLPL_HIP_TRY(hipDeviceSynchronize());
    const long long have = ctx->hamming_clock_launches < kClockRing ? ctx->hamming_clock_launches : kClockRing;
    const int n = (int)(have < max_items ? have : max_items);
    if (n <= 0 || !ctx->ws[WS_CLOCK]) return 0;
    unsigned long long ring[kClockRing * 4];
    MLPL_HIP_TRY(hipMemcpy(ring, ctx->ws[WS_CLOCK], sizeof(ring), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {  // oldest first
        const long long launch = ctx->hamming_clock_launches - n + i;
        std::memcpy(out + (size_t)i * 4, ring + (size_t)(launch % kClockRing) * 4, 32);
    }
    return n;
} MLPL_ENTRY_END("mlpl_debug_hamming_clock")

int mlpl_profile_enable(mlpl_ctx *ctx, int on) try {
    if (!ctx) return MLPL_E_BAD_INPUT;
    ctx->prof_on = on > 0 ? on : 0;  // N > 1: every Nth launch of a kernel is bracketed
    if (ctx->prof_on) {
        // event pools up front: creating them lazily put ~10^4 hipEventCreate calls into the caller's first timed launch
        for (int id = 0; id < MLPL_PROF_NUM; ++id) {
            if (ctx->prof_ev[id]) continue;
            ctx->prof_ev[id] = new hipEvent_t[2 * kProfMaxLaunches];
            for (int i = 0; i < 2 * kProfMaxLaunches; ++i) (void)hipEventCreate(&ctx->prof_ev[id][i]);
        }
    }
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_profile_enable")

int mlpl_profile_reset(mlpl_ctx *ctx) try {
    if (!ctx) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < MLPL_PROF_NUM; ++k) ctx->prof_n[k] = ctx->prof_calls[k] = 0;
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_profile_reset")

int mlpl_profile_read(mlpl_ctx *ctx, int kernel_id, double *total_ms, int *launches) try {
    if (!ctx || kernel_id < 0 || kernel_id >= MLPL_PROF_NUM || !total_ms || !launches) return MLPL_E_BAD_INPUT;
    double tot = 0.0;
    const int n = ctx->prof_n[kernel_id];
    for (int i = 0; i < n; ++i) {
        MLPL_HIP_TRY(hipEventSynchronize(ctx->prof_ev[kernel_id][2 * i + 1]));
        float ms = 0.f;
        MLPL_HIP_TRY(hipEventElapsedTime(&ms, ctx->prof_ev[kernel_id][2 * i], ctx->prof_ev[kernel_id][2 * i + 1]));
        tot += ms;
    }
    *total_ms = tot;
    *launches = n;
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_profile_read")

int mlpl_debug_l2_flags(mlpl_ctx *ctx, int flags[4]) try {
    if (!ctx || !flags) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    MLPL_HIP_TRY(hipDeviceSynchronize());
    flags[0] = flags[1] = flags[2] = flags[3] = 0;
    if (ctx->l2_flag_ptr) MLPL_HIP_TRY(hipMemcpy(flags, ctx->l2_flag_ptr, 16, hipMemcpyDeviceToHost));
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_debug_l2_flags")

int mlpl_set_l2_path(mlpl_ctx *ctx, int mode) {
    if (!ctx || mode < 0 || mode > 3) return MLPL_E_BAD_INPUT;
    ctx->l2_mode = mode;
    return MLPL_OK;
}

// ---------------------------------------------------------------------------------------------------------
// device-pointer entry points
// ---------------------------------------------------------------------------------------------------------

int mlpl_knn2_hamming_dev(mlpl_ctx *ctx, const uint8_t *d_q, int nq, size_t q_stride, size_t q_batch_stride,
                          const uint8_t *d_t, int nt, size_t t_stride, size_t t_batch_stride, int nbytes, int k,
                          int batch, int32_t *d_idx, int32_t *d_dist, void *stream) try {
    if (!ctx) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_knn_hamming(ctx, d_q, nq, q_stride, q_batch_stride, d_t, nt, t_stride, t_batch_stride, nbytes, k,
                              batch, d_idx, d_dist, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_knn2_hamming_dev")

int mlpl_knn2_l2sq_f32_dev(mlpl_ctx *ctx, const float *d_q, int nq, size_t q_stride, size_t q_batch_stride,
                           const float *d_t, int nt, size_t t_stride, size_t t_batch_stride, int dim, int k, int batch,
                           int32_t *d_idx, float *d_dist, void *stream) try {
    if (!ctx) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_knn_l2(ctx, d_q, nq, q_stride, q_batch_stride, d_t, nt, t_stride, t_batch_stride, dim, k, batch,
                         d_idx, d_dist, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_knn2_l2sq_f32_dev")

int mlpl_ratio_compact_i32_dev(mlpl_ctx *ctx, const int32_t *d_idx, const int32_t *d_dist, int nq, int k, int batch,
                               float ratio, mlpl_dmatch *d_out, int32_t *d_n_out, void *stream) try {
    if (!ctx) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_ratio_compact(ctx, d_idx, d_dist, 0, nq, k, batch, ratio, d_out, d_n_out, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_ratio_compact_i32_dev")

int mlpl_ratio_compact_f32_dev(mlpl_ctx *ctx, const int32_t *d_idx, const float *d_dist, int nq, int k, int batch,
                               float ratio, mlpl_dmatch *d_out, int32_t *d_n_out, void *stream) try {
    if (!ctx) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_ratio_compact(ctx, d_idx, d_dist, 1, nq, k, batch, ratio, d_out, d_n_out, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_ratio_compact_f32_dev")

int mlpl_gather_match_points_dev(mlpl_ctx *ctx, const mlpl_dmatch *d_matches, int n, const float *d_kp1, const float *d_kp2,
                                 const double K0[4], const double K1[4], double *d_p1, double *d_p2, void *stream) try {
    if (!ctx || !d_matches || !d_kp1 || !d_kp2 || !K0 || !K1 || !d_p1 || !d_p2 || n < 0) {
        set_error("mlpl_gather_match_points_dev: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_gather_match_points(d_matches, n, d_kp1, d_kp2, K0, K1, d_p1, d_p2, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_gather_match_points_dev")

int mlpl_vfc_filter(mlpl_ctx *ctx, const float *x1, const float *x2, int n, uint32_t seed, uint8_t *keep, int *n_keep, double *P, int info[4]) try {
    if (!ctx || n < 0 || n > 65535 || (n > 0 && (!x1 || !x2 || !keep))) {
        set_error("mlpl_vfc_filter: bad arguments (n in [0, 65535])");
        return MLPL_E_INTERNAL;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nn = (size_t)std::max(n, 1);
    void *d1, *d2;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, nn * 8, &d1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX1, nn * 8, &d2))) return rc;
    if (n > 0) {
        MLPL_HIP_TRY(hipMemcpyAsync(d1, x1, (size_t)n * 8, hipMemcpyHostToDevice, s));
        MLPL_HIP_TRY(hipMemcpyAsync(d2, x2, (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    VfcWork work{};
    if ((rc = launch_vfc(ctx, 1, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, (const float *)d1, (const float *)d2, n, &seed, 0, nullptr, nullptr,
                         nullptr, &work, s)))
        return rc;
    int32_t res[8];
    MLPL_HIP_TRY(hipMemcpyAsync(res, work.res, sizeof(res), hipMemcpyDeviceToHost, s));
    if (n > 0) MLPL_HIP_TRY(hipMemcpyAsync(keep, work.keep, (size_t)n, hipMemcpyDeviceToHost, s));
    if (n > 0 && P) MLPL_HIP_TRY(hipMemcpyAsync(P, work.P, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    if (n_keep) *n_keep = res[1];
    if (info) info[0] = res[2], info[1] = res[3], info[2] = res[4], info[3] = res[5];
    return res[0];
} MLPL_ENTRY_END("mlpl_vfc_filter")

int mlpl_vfc_filter_matches_dev(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches,
                                const float *d_kp1, int nq, const float *d_kp2, int nt, const uint32_t *seeds, int getmatches_rule,
                                mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_status, void *stream) try {
    if (!ctx || batch < 1 || batch > 65535 || !d_matches || match_stride < 1 || match_stride > 65535 || !d_n_matches || !d_kp1 || !d_kp2 ||
        nq < 1 || nt < 1 || !d_out || d_out == d_matches || !d_n_out || !d_status) {
        set_error("mlpl_vfc_filter_matches_dev: bad arguments (batch, match_stride in [1, 65535]; d_out apart from d_matches)");
        return MLPL_E_INTERNAL;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_vfc(ctx, batch, d_matches, match_stride, d_n_matches, d_kp1, nq, d_kp2, nt, nullptr, nullptr, 0, seeds, getmatches_rule, d_out,
                      d_n_out, d_status, nullptr, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_vfc_filter_matches_dev")

int mlpl_gms_filter(mlpl_ctx *ctx, const float *kp1, int n1, int width1, int height1, const float *kp2, int n2, int width2, int height2,
                    const mlpl_dmatch *matches, int n, int use_scale, int use_rotation, uint8_t *keep, int *n_keep, int info[4]) try {
    if (!ctx || n < 0 || n > 65535 || n1 < 0 || n2 < 0 || width1 <= 0 || height1 <= 0 || width2 <= 0 || height2 <= 0 ||
        (n > 0 && (!kp1 || !kp2 || !matches || !keep))) {
        set_error("mlpl_gms_filter: bad arguments (n in [0, 65535], positive image sizes)");
        return MLPL_E_BAD_INPUT;
    }
    for (int i = 0; i < n; ++i)
        if (matches[i].queryIdx < 0 || matches[i].queryIdx >= n1 || matches[i].trainIdx < 0 || matches[i].trainIdx >= n2) {
            set_error("mlpl_gms_filter: match %d points outside the keypoint arrays", i);
            return MLPL_E_BAD_INPUT;
        }
    if (n_keep) *n_keep = 0;
    if (info) info[0] = -1, info[1] = -1, info[2] = 0, info[3] = 0;
    if (n == 0) return MLPL_OK;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    void *d1, *d2, *dm;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, (size_t)n1 * 8, &d1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX1, (size_t)n2 * 8, &d2))) return rc;
    if ((rc = ws_get(ctx, WS_AUX2, (size_t)n * sizeof(mlpl_dmatch), &dm))) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(d1, kp1, (size_t)n1 * 8, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(d2, kp2, (size_t)n2 * 8, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(dm, matches, (size_t)n * sizeof(mlpl_dmatch), hipMemcpyHostToDevice, s));
    GmsWork work{};
    if ((rc = launch_gms(ctx, 1, (const mlpl_dmatch *)dm, n, nullptr, n, (const float *)d1, n1, (const float *)d2, n2, width1, height1, width2,
                         height2, use_scale, use_rotation, 0, nullptr, nullptr, nullptr, &work, s)))
        return rc;
    int32_t res[8];
    MLPL_HIP_TRY(hipMemcpyAsync(res, work.res, sizeof(res), hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipMemcpyAsync(keep, work.keep, (size_t)n, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    if (n_keep) *n_keep = res[0];
    if (info) info[0] = res[1], info[1] = res[2], info[2] = res[3], info[3] = 0;
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_gms_filter")

int mlpl_gms_filter_matches_dev(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches,
                                const float *d_kp1, int nq, const float *d_kp2, int nt, int width1, int height1, int width2, int height2,
                                int use_scale, int use_rotation, int min_final_rule, mlpl_dmatch *d_out, int32_t *d_n_out,
                                int32_t *d_n_inliers, void *stream) try {
    if (!ctx || batch < 1 || batch > 65535 || !d_matches || match_stride < 1 || match_stride > 65535 || !d_n_matches || !d_kp1 || !d_kp2 ||
        nq < 1 || nt < 1 || width1 <= 0 || height1 <= 0 || width2 <= 0 || height2 <= 0 || !d_out || d_out == d_matches || !d_n_out ||
        !d_n_inliers) {
        set_error("mlpl_gms_filter_matches_dev: bad arguments (batch, match_stride in [1, 65535]; positive image sizes; d_out apart from d_matches)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_gms(ctx, batch, d_matches, match_stride, d_n_matches, 0, d_kp1, nq, d_kp2, nt, width1, height1, width2, height2, use_scale,
                      use_rotation, min_final_rule, d_out, d_n_out, d_n_inliers, nullptr, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_gms_filter_matches_dev")

int mlpl_subpix_matches(mlpl_ctx *ctx, const uint8_t *img1, int width1, int height1, size_t step1, const uint8_t *img2, int width2, int height2,
                        size_t step2, const float *kp1, float *kp2, const float *size1, const float *size2, int n, uint8_t *inlier,
                        int *n_refined, int *status, int info[4]) try {
    if (!ctx || n < 0 || n > 65535 || !img1 || !img2 || width1 <= 0 || height1 <= 0 || width2 <= 0 || height2 <= 0 || step1 < (size_t)width1 ||
        step2 < (size_t)width2 || (n > 0 && (!kp1 || !kp2 || !inlier))) {
        set_error("mlpl_subpix_matches: bad arguments (n in [0, 65535], 8-bit images of positive size, row step >= width)");
        return MLPL_E_BAD_INPUT;
    }
    if (n_refined) *n_refined = 0;
    if (status) *status = -1;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (n == 0) return MLPL_OK;
    // LDS is provisioned for the largest side in the list; nothing else depends on it
    int max_side = 17;
    if (size1 || size2)
        for (int i = 0; i < n; ++i) max_side = std::max(max_side, mlpl_subpix_template_side(size1 ? size1[i] : 0.0f, size2 ? size2[i] : 0.0f));
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    void *di1, *di2, *d1, *d2, *dsz, *dinl;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, (size_t)width1 * height1, &di1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX1, (size_t)width2 * height2, &di2))) return rc;
    if ((rc = ws_get(ctx, WS_AUX2, (size_t)n * 8, &d1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX3, (size_t)n * 8, &d2))) return rc;
    if ((rc = ws_get(ctx, WS_AUX4, (size_t)n * 8, &dsz))) return rc;
    if ((rc = ws_get(ctx, WS_AUX5, (size_t)n, &dinl))) return rc;
    float *ds1 = size1 ? (float *)dsz : nullptr, *ds2 = size2 ? (float *)dsz + n : nullptr;
    MLPL_HIP_TRY(hipMemcpy2DAsync(di1, (size_t)width1, img1, step1, (size_t)width1, (size_t)height1, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpy2DAsync(di2, (size_t)width2, img2, step2, (size_t)width2, (size_t)height2, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(d1, kp1, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(d2, kp2, (size_t)n * 8, hipMemcpyHostToDevice, s));
    if (ds1) MLPL_HIP_TRY(hipMemcpyAsync(ds1, size1, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (ds2) MLPL_HIP_TRY(hipMemcpyAsync(ds2, size2, (size_t)n * 4, hipMemcpyHostToDevice, s));
    SubpixWork work{};
    if ((rc = launch_subpix(ctx, 1, nullptr, n, nullptr, n, (const float *)d1, n, (const float *)d2, n, ds1, ds2, (const uint8_t *)di1, width1,
                            height1, (size_t)width1, 0, (const uint8_t *)di2, width2, height2, (size_t)width2, 0, max_side, 0, nullptr, nullptr,
                            nullptr, (float *)d2, (uint8_t *)dinl, &work, s)))
        return rc;
    int32_t res[8];
    MLPL_HIP_TRY(hipMemcpyAsync(res, work.res, sizeof(res), hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipMemcpyAsync(kp2, d2, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipMemcpyAsync(inlier, dinl, (size_t)n, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    if (n_refined) *n_refined = res[0];
    if (status) *status = res[1];
    if (info) info[0] = res[2], info[1] = res[3], info[2] = res[4], info[3] = res[5];
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_subpix_matches")

int mlpl_subpix_matches_dev(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches,
                            const float *d_kp1, int nq, const float *d_kp2, int nt, const float *d_size1, const float *d_size2,
                            const uint8_t *d_img1, int width1, int height1, size_t step1, size_t batch_stride1, const uint8_t *d_img2,
                            int width2, int height2, size_t step2, size_t batch_stride2, int max_side, int correspondences_rule,
                            mlpl_dmatch *d_out, int32_t *d_n_out, int32_t *d_status, float *d_kp2_out, uint8_t *d_inlier, void *stream) try {
    if (!ctx || batch < 1 || batch > 65535 || !d_matches || match_stride < 1 || match_stride > 65535 || !d_n_matches || !d_kp1 || !d_kp2 ||
        nq < 1 || nt < 1 || !d_img1 || !d_img2 || width1 <= 0 || height1 <= 0 || width2 <= 0 || height2 <= 0 || step1 < (size_t)width1 ||
        step2 < (size_t)width2 || max_side < 0 || max_side > 255 || !d_out || d_out == d_matches || !d_n_out || !d_status || !d_kp2_out) {
        set_error("mlpl_subpix_matches_dev: bad arguments (batch, match_stride in [1, 65535]; 8-bit images of positive size, row step >= width; "
                  "max_side in [0, 255]; d_out apart from d_matches)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_subpix(ctx, batch, d_matches, match_stride, d_n_matches, 0, d_kp1, nq, d_kp2, nt, d_size1, d_size2, d_img1, width1, height1,
                         step1, batch_stride1, d_img2, width2, height2, step2, batch_stride2, max_side, correspondences_rule, d_out, d_n_out,
                         d_status, d_kp2_out, d_inlier, nullptr, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_subpix_matches_dev")

int mlpl_subpix_separate(mlpl_ctx *ctx, const uint8_t *img1, int width1, int height1, size_t step1, const uint8_t *img2, int width2, int height2,
                         size_t step2, float *kp1, float *kp2, const float *size1, const float *size2, int n, uint8_t *inlier, int32_t *iters,
                         int *n_refined, int *status, int info[4]) try {
    if (!ctx || n < 0 || n > 65535 || !img1 || !img2 || width1 <= 0 || height1 <= 0 || width2 <= 0 || height2 <= 0 || step1 < (size_t)width1 ||
        step2 < (size_t)width2 || (n > 0 && (!kp1 || !kp2 || !inlier))) {
        set_error("mlpl_subpix_separate: bad arguments (n in [0, 65535], 8-bit images of positive size, row step >= width)");
        return MLPL_E_BAD_INPUT;
    }
    // step 1 on the host as well: the image size rule needs the windows in front of the launch
    float m1 = FLT_MAX, m2 = FLT_MAX;
    for (int i = 0; i < n; ++i) {
        if (size1 && size1[i] > 0.f && size1[i] < m1) m1 = size1[i];
        if (size2 && size2[i] > 0.f && size2[i] < m2) m2 = size2[i];
    }
    const int w1 = mlpl_subpix_separate_window(m1), w2 = mlpl_subpix_separate_window(m2);
    if (width1 < 2 * w1 + 5 || height1 < 2 * w1 + 5 || width2 < 2 * w2 + 5 || height2 < 2 * w2 + 5) {
        set_error("mlpl_subpix_separate: an image is smaller than 2 w + 5 pixels (w = %d, %d)", w1, w2);
        return MLPL_E_BAD_INPUT;
    }
    if (n_refined) *n_refined = 0;
    if (status) *status = -1;
    if (info) info[0] = w1, info[1] = w2, info[2] = info[3] = 0;
    if (n == 0) return MLPL_OK;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    void *di1, *di2, *d1, *d2, *dsz, *dinl, *dit;
    int rc;
    if ((rc = ws_get(ctx, WS_AUX0, (size_t)width1 * height1, &di1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX1, (size_t)width2 * height2, &di2))) return rc;
    if ((rc = ws_get(ctx, WS_AUX2, (size_t)n * 8, &d1))) return rc;
    if ((rc = ws_get(ctx, WS_AUX3, (size_t)n * 8, &d2))) return rc;
    if ((rc = ws_get(ctx, WS_AUX4, (size_t)n * 8, &dsz))) return rc;
    if ((rc = ws_get(ctx, WS_AUX5, (size_t)n, &dinl))) return rc;
    if ((rc = ws_get(ctx, WS_AUX6, (size_t)n * 8, &dit))) return rc;
    float *ds1 = size1 ? (float *)dsz : nullptr, *ds2 = size2 ? (float *)dsz + n : nullptr;
    MLPL_HIP_TRY(hipMemcpy2DAsync(di1, (size_t)width1, img1, step1, (size_t)width1, (size_t)height1, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpy2DAsync(di2, (size_t)width2, img2, step2, (size_t)width2, (size_t)height2, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(d1, kp1, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MLPL_HIP_TRY(hipMemcpyAsync(d2, kp2, (size_t)n * 8, hipMemcpyHostToDevice, s));
    if (ds1) MLPL_HIP_TRY(hipMemcpyAsync(ds1, size1, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (ds2) MLPL_HIP_TRY(hipMemcpyAsync(ds2, size2, (size_t)n * 4, hipMemcpyHostToDevice, s));
    SubpixWork work{};
    if ((rc = launch_subpix_separate(ctx, 1, nullptr, n, nullptr, n, (const float *)d1, n, (const float *)d2, n, ds1, ds2, (const uint8_t *)di1,
                                     width1, height1, (size_t)width1, 0, (const uint8_t *)di2, width2, height2, (size_t)width2, 0, 0, nullptr,
                                     nullptr, nullptr, (float *)d1, (float *)d2, (uint8_t *)dinl, (int32_t *)dit, &work, s)))
        return rc;
    int32_t res[8];
    MLPL_HIP_TRY(hipMemcpyAsync(res, work.res, sizeof(res), hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipMemcpyAsync(kp1, d1, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipMemcpyAsync(kp2, d2, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipMemcpyAsync(inlier, dinl, (size_t)n, hipMemcpyDeviceToHost, s));
    if (iters) MLPL_HIP_TRY(hipMemcpyAsync(iters, dit, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    MLPL_HIP_TRY(hipStreamSynchronize(s));
    if (n_refined) *n_refined = res[0];
    if (status) *status = res[1];
    if (info) info[0] = res[2], info[1] = res[3], info[2] = res[4], info[3] = res[5];
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_subpix_separate")

int mlpl_subpix_separate_dev(mlpl_ctx *ctx, int batch, const mlpl_dmatch *d_matches, int match_stride, const int32_t *d_n_matches,
                             const float *d_kp1, int nq, const float *d_kp2, int nt, const float *d_size1, const float *d_size2,
                             const uint8_t *d_img1, int width1, int height1, size_t step1, size_t batch_stride1, const uint8_t *d_img2,
                             int width2, int height2, size_t step2, size_t batch_stride2, int correspondences_rule, mlpl_dmatch *d_out,
                             int32_t *d_n_out, int32_t *d_status, float *d_kp1_out, float *d_kp2_out, uint8_t *d_inlier, void *stream) try {
    // the windows are taken on the device, so the image size rule is applied for the largest one: 2 * 10 + 5
    if (!ctx || batch < 1 || batch > 65535 || !d_matches || match_stride < 1 || match_stride > 65535 || !d_n_matches || !d_kp1 || !d_kp2 ||
        nq < 1 || nt < 1 || !d_img1 || !d_img2 || width1 < 25 || height1 < 25 || width2 < 25 || height2 < 25 || step1 < (size_t)width1 ||
        step2 < (size_t)width2 || !d_out || d_out == d_matches || !d_n_out || !d_status || !d_kp2_out) {
        set_error("mlpl_subpix_separate_dev: bad arguments (batch, match_stride in [1, 65535]; 8-bit images of at least 25 x 25 pixels, row step "
                  ">= width; d_out apart from d_matches)");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    return launch_subpix_separate(ctx, batch, d_matches, match_stride, d_n_matches, 0, d_kp1, nq, d_kp2, nt, d_size1, d_size2, d_img1, width1,
                                  height1, step1, batch_stride1, d_img2, width2, height2, step2, batch_stride2, correspondences_rule, d_out,
                                  d_n_out, d_status, d_kp1_out, d_kp2_out, d_inlier, nullptr, nullptr, pick_stream(ctx, stream));
} MLPL_ENTRY_END("mlpl_subpix_separate_dev")

int mlpl_match_hamming_dev(mlpl_ctx *ctx, const uint8_t *d_q, int nq, size_t q_stride, size_t q_batch_stride,
                           const uint8_t *d_t, int nt, size_t t_stride, size_t t_batch_stride, int nbytes,
                           int ratio_test, float ratio, int batch, int32_t *d_idx, int32_t *d_dist, mlpl_dmatch *d_out,
                           int32_t *d_n_out, void *stream) try {
    if (!ctx) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const int k = ratio_test ? 2 : 1;
    void *gc = nullptr;
    const int ncnt = (nq + kCountGroup - 1) / kCountGroup;
    int rc = ws_get(ctx, WS_COUNT, (size_t)batch * std::max(ncnt, 1) * sizeof(int32_t), &gc);
    if (rc) return rc;
    HammingEmitOut emit{d_out, d_n_out, 0};
    rc = launch_knn_hamming(ctx, d_q, nq, q_stride, q_batch_stride, d_t, nt, t_stride, t_batch_stride, nbytes, k, batch,
                            d_idx, d_dist, s, ratio, (int32_t *)gc, &emit);
    if (rc) return rc;
    if (emit.emitted) return MLPL_OK;  // (the latency shape: the merge kernel wrote the matches and their number)
    return launch_ratio_compact(ctx, d_idx, d_dist, 0, nq, k, batch, ratio, d_out, d_n_out, s, (int32_t *)gc);
} MLPL_ENTRY_END("mlpl_match_hamming_dev")

int mlpl_match_l2_dev(mlpl_ctx *ctx, const float *d_q, int nq, size_t q_stride, size_t q_batch_stride, const float *d_t, int nt,
                      size_t t_stride, size_t t_batch_stride, int dim, int ratio_test, float ratio, int batch, int32_t *d_idx, float *d_dist,
                      mlpl_dmatch *d_out, int32_t *d_n_out, void *stream) try {
    if (!ctx) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const int k = ratio_test ? 2 : 1;
    // The pass counts come out of the split fold (knn_l2_fold_ratio_kernel) wherever a fold runs; the fp16 candidate path ends in its own
    // re-rank kernel and leaves them to ratio_count_kernel.  (Arguments out of range: launch_knn_l2 refuses them, nothing is sized by them.)
    void *gc = nullptr;
    if (ctx->opt_l2_fold_counts && nq > 0 && batch >= 1 && batch <= 65535) {
        const int ncnt = (nq + kCountGroup - 1) / kCountGroup;
        int rc = ws_get(ctx, WS_COUNT, (size_t)batch * ncnt * sizeof(int32_t), &gc);
        if (rc) return rc;
    }
    int counted = 0;
    int rc = launch_knn_l2(ctx, d_q, nq, q_stride, q_batch_stride, d_t, nt, t_stride, t_batch_stride, dim, k, batch, d_idx, d_dist, s, 0, ratio,
                           (int32_t *)gc, &counted);
    if (rc) return rc;
    rc = launch_ratio_compact(ctx, d_idx, d_dist, 1, nq, k, batch, ratio, d_out, d_n_out, s, counted ? (int32_t *)gc : nullptr);
    if (rc == MLPL_OK && nq > 0) ctx->dbg_l2_match[3] += counted ? 1 : 2;  // ratio_write_kernel [+ ratio_count_kernel]
    return rc;
} MLPL_ENTRY_END("mlpl_match_l2_dev")

// (tests) the float knn with the fused fold alone: the counts the fold stored, read back
int mlpl_debug_l2_fold_counts(mlpl_ctx *ctx, const float *d_q, int nq, size_t q_stride, size_t q_batch_stride, const float *d_t, int nt,
                               size_t t_stride, size_t t_batch_stride, int dim, int ratio_test, float ratio, int batch, int32_t *d_idx, float *d_dist,
                               int32_t *counts) try {
    if (!ctx || !counts || nq < 1 || batch < 1 || batch > 65535) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    const int ncnt = (nq + kCountGroup - 1) / kCountGroup;
    void *gc = nullptr;
    int rc = ws_get(ctx, WS_COUNT, (size_t)batch * ncnt * sizeof(int32_t), &gc);
    if (rc) return rc;
    MLPL_HIP_TRY(hipMemsetAsync(gc, 0xFF, (size_t)batch * ncnt * sizeof(int32_t), ctx->stream));  // (-1: a group nobody wrote shows)
    int counted = 0;
    rc = launch_knn_l2(ctx, d_q, nq, q_stride, q_batch_stride, d_t, nt, t_stride, t_batch_stride, dim, ratio_test ? 2 : 1, batch, d_idx, d_dist, ctx->stream, 0,
                       ratio, (int32_t *)gc, &counted);
    if (rc) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(counts, gc, (size_t)batch * ncnt * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return counted ? batch * ncnt : 0;
} MLPL_ENTRY_END("mlpl_debug_l2_fold_counts")

// ---------------------------------------------------------------------------------------------------------
// host-pointer entry points: stage through the context workspace, run the device path, copy back
// ---------------------------------------------------------------------------------------------------------

namespace {

// Copies `rows` rows of `row_bytes` bytes (host stride `stride`) into a dense device buffer.
int upload_rows(mlpl_ctx *ctx, WsSlot slot, const void *host, int rows, size_t row_bytes, size_t stride, void **dev) {
    int rc = ws_get(ctx, slot, (size_t)rows * row_bytes, dev);
    if (rc) return rc;
    if (rows == 0) return MLPL_OK;
    if (stride == row_bytes)  // dense rows: one linear copy (a 2-D copy of 32-byte rows is an order of magnitude slower)
        MLPL_HIP_TRY(hipMemcpyAsync(*dev, host, (size_t)rows * row_bytes, hipMemcpyHostToDevice, ctx->stream));
    else
        MLPL_HIP_TRY(hipMemcpy2DAsync(*dev, row_bytes, host, stride, row_bytes, rows, hipMemcpyHostToDevice, ctx->stream));
    return MLPL_OK;
}

}  // namespace

int mlpl_knn2_hamming(mlpl_ctx *ctx, const uint8_t *q, int nq, size_t q_stride, const uint8_t *t, int nt, size_t t_stride,
                      int nbytes, int k, int32_t *idx, int32_t *dist) try {
    if (!ctx || !q || !t || !idx || !dist || nq < 0 || nt < 0 || nbytes < 1 || q_stride < (size_t)nbytes ||
        t_stride < (size_t)nbytes || (k != 1 && k != 2) || nt < k) {
        set_error("mlpl_knn2_hamming: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    if (nq == 0) return MLPL_OK;
    void *dq, *dt, *didx, *ddist;
    int rc;
    if ((rc = upload_rows(ctx, WS_AUX0, q, nq, nbytes, q_stride, &dq))) return rc;
    if ((rc = upload_rows(ctx, WS_AUX1, t, nt, nbytes, t_stride, &dt))) return rc;
    if ((rc = ws_get(ctx, WS_IDX, (size_t)nq * k * 4, &didx))) return rc;
    if ((rc = ws_get(ctx, WS_DIST, (size_t)nq * k * 4, &ddist))) return rc;
    rc = launch_knn_hamming(ctx, (const uint8_t *)dq, nq, nbytes, 0, (const uint8_t *)dt, nt, nbytes, 0, nbytes, k, 1,
                            (int32_t *)didx, (int32_t *)ddist, ctx->stream);
    if (rc) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(idx, didx, (size_t)nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipMemcpyAsync(dist, ddist, (size_t)nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_knn2_hamming")

int mlpl_knn2_l2sq_f32(mlpl_ctx *ctx, const float *q, int nq, size_t q_stride, const float *t, int nt, size_t t_stride,
                       int dim, int k, int32_t *idx, float *dist) try {
    if (!ctx || !q || !t || !idx || !dist || nq < 0 || nt < 0 || dim < 1 || q_stride < (size_t)dim ||
        t_stride < (size_t)dim || (k != 1 && k != 2) || nt < k) {
        set_error("mlpl_knn2_l2sq_f32: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    if (nq == 0) return MLPL_OK;
    void *dq, *dt, *didx, *ddist;
    int rc;
    if ((rc = upload_rows(ctx, WS_AUX0, q, nq, (size_t)dim * 4, q_stride * 4, &dq))) return rc;
    if ((rc = upload_rows(ctx, WS_AUX1, t, nt, (size_t)dim * 4, t_stride * 4, &dt))) return rc;
    if ((rc = ws_get(ctx, WS_IDX, (size_t)nq * k * 4, &didx))) return rc;
    if ((rc = ws_get(ctx, WS_DIST, (size_t)nq * k * 4, &ddist))) return rc;
    rc = launch_knn_l2(ctx, (const float *)dq, nq, dim, 0, (const float *)dt, nt, dim, 0, dim, k, 1, (int32_t *)didx,
                       (float *)ddist, ctx->stream);
    if (rc) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(idx, didx, (size_t)nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipMemcpyAsync(dist, ddist, (size_t)nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_knn2_l2sq_f32")

static int ratio_compact_host(mlpl_ctx *ctx, const int32_t *idx, const void *dist, int is_float, int nq, int k,
                              float ratio, mlpl_dmatch *out, int *n_out) {
    if (!ctx || !idx || !dist || !out || !n_out || nq < 0 || (k != 1 && k != 2)) {
        set_error("mlpl_ratio_compact: bad arguments");
        return MLPL_E_BAD_INPUT;
    }
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    *n_out = 0;
    if (nq == 0) return MLPL_OK;
    void *didx, *ddist, *dout, *dcnt;
    int rc;
    if ((rc = ws_get(ctx, WS_IDX, (size_t)nq * k * 4, &didx))) return rc;
    if ((rc = ws_get(ctx, WS_DIST, (size_t)nq * k * 4, &ddist))) return rc;
    if ((rc = ws_get(ctx, WS_MATCH, (size_t)nq * sizeof(mlpl_dmatch), &dout))) return rc;
    if ((rc = ws_get(ctx, WS_SCALARS, 64, &dcnt))) return rc;
    MLPL_HIP_TRY(hipMemcpyAsync(didx, idx, (size_t)nq * k * 4, hipMemcpyHostToDevice, ctx->stream));
    MLPL_HIP_TRY(hipMemcpyAsync(ddist, dist, (size_t)nq * k * 4, hipMemcpyHostToDevice, ctx->stream));
    rc = launch_ratio_compact(ctx, (const int32_t *)didx, ddist, is_float, nq, k, 1, ratio, (mlpl_dmatch *)dout,
                              (int32_t *)dcnt, ctx->stream);
    if (rc) return rc;
    int32_t cnt = 0;
    MLPL_HIP_TRY(hipMemcpyAsync(&cnt, dcnt, 4, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (cnt > 0) MLPL_HIP_TRY(hipMemcpy(out, dout, (size_t)cnt * sizeof(mlpl_dmatch), hipMemcpyDeviceToHost));
    *n_out = cnt;
    return MLPL_OK;
}

int mlpl_ratio_compact_i32(mlpl_ctx *ctx, const int32_t *idx, const int32_t *dist, int nq, int k, float ratio,
                           mlpl_dmatch *out, int *n_out) try {
    return ratio_compact_host(ctx, idx, dist, 0, nq, k, ratio, out, n_out);
} MLPL_ENTRY_END("mlpl_ratio_compact_i32")

int mlpl_ratio_compact_f32(mlpl_ctx *ctx, const int32_t *idx, const float *dist, int nq, int k, float ratio,
                           mlpl_dmatch *out, int *n_out) try {
    return ratio_compact_host(ctx, idx, dist, 1, nq, k, ratio, out, n_out);
} MLPL_ENTRY_END("mlpl_ratio_compact_f32")

int mlpl_get_matches_linear(mlpl_ctx *ctx, int n_keypoints1, int n_keypoints2, const void *desc1, int rows1, size_t step1,
                            const void *desc2, int rows2, size_t step2, int cols, int desc_type, int ratio_test,
                            mlpl_dmatch *out, int *n_out) try {
    if (!ctx || !n_out) return MLPL_E_BAD_INPUT;
    *n_out = 0;
    // reference matchers.cpp:123-133
    if (n_keypoints1 < 15 || n_keypoints2 < 15) return MLPL_E_FEW_KEYPOINTS;
    if (n_keypoints1 != rows1 || n_keypoints2 != rows2) return MLPL_E_BAD_INPUT;
    // reference matchers.cpp:540-547
    if (desc_type != 0 && desc_type != 5) return MLPL_E_BAD_INPUT;
    if (!desc1 || !desc2 || !out || cols < 1) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    const int k = ratio_test ? 2 : 1;  // matchers.cpp:529-538
    const size_t elem = desc_type == 0 ? 1 : 4;
    if (step1 < (size_t)cols * elem || step2 < (size_t)cols * elem) return MLPL_E_BAD_INPUT;
    void *dq, *dt, *didx, *ddist, *dout, *dcnt;
    int rc;
    if ((rc = upload_rows(ctx, WS_AUX0, desc1, rows1, (size_t)cols * elem, step1, &dq))) return rc;
    if ((rc = upload_rows(ctx, WS_AUX1, desc2, rows2, (size_t)cols * elem, step2, &dt))) return rc;
    if ((rc = ws_get(ctx, WS_IDX, (size_t)rows1 * k * 4, &didx))) return rc;
    if ((rc = ws_get(ctx, WS_DIST, (size_t)rows1 * k * 4, &ddist))) return rc;
    if ((rc = ws_get(ctx, WS_MATCH, (size_t)rows1 * sizeof(mlpl_dmatch), &dout))) return rc;
    if ((rc = ws_get(ctx, WS_SCALARS, 64, &dcnt))) return rc;
    if (desc_type == 0) {
        rc = launch_knn_hamming(ctx, (const uint8_t *)dq, rows1, cols, 0, (const uint8_t *)dt, rows2, cols, 0, cols, k, 1,
                                (int32_t *)didx, (int32_t *)ddist, ctx->stream);
    } else {
        rc = launch_knn_l2(ctx, (const float *)dq, rows1, cols, 0, (const float *)dt, rows2, cols, 0, cols, k, 1,
                           (int32_t *)didx, (float *)ddist, ctx->stream);
    }
    if (rc) return rc == MLPL_E_BAD_INPUT ? MLPL_E_BAD_INPUT : rc;
    rc = launch_ratio_compact(ctx, (const int32_t *)didx, ddist, desc_type == 5, rows1, k, 1, 0.75f, (mlpl_dmatch *)dout,
                              (int32_t *)dcnt, ctx->stream);
    if (rc) return rc;
    int32_t cnt = 0;
    MLPL_HIP_TRY(hipMemcpyAsync(&cnt, dcnt, 4, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (cnt > 0) MLPL_HIP_TRY(hipMemcpy(out, dout, (size_t)cnt * sizeof(mlpl_dmatch), hipMemcpyDeviceToHost));
    *n_out = cnt;
    if (cnt < 2) return MLPL_E_FAILED;  // matchers.cpp:709-713 (MIN_FINAL_MATCHES = 2)
    return MLPL_OK;
} MLPL_ENTRY_END("mlpl_get_matches_linear")

int mlpl_get_matches_bruteforce_nms(mlpl_ctx *ctx, int n_keypoints1, int n_keypoints2, const void *desc1, int rows1,
                                    size_t step1, const void *desc2, int rows2, size_t step2, int cols, int desc_type,
                                    int ratio_test, mlpl_dmatch *out, int *n_out) try {
    if (!ctx || !n_out) return MLPL_E_BAD_INPUT;
    *n_out = 0;
    if (n_keypoints1 < 15 || n_keypoints2 < 15) return MLPL_E_FEW_KEYPOINTS;                 // matchers.cpp:123-127
    if (n_keypoints1 != rows1 || n_keypoints2 != rows2) return MLPL_E_BAD_INPUT;             // matchers.cpp:129-133
    if (desc_type != 0 && desc_type != 5) {
        set_error("BRUTEFORCENMS: CV_8U and CV_32F descriptors are built (the reference also takes CV_64F)");
        return desc_type == 6 ? MLPL_E_UNSUPPORTED : MLPL_E_BAD_INPUT;                       // matchers.cpp:514-518
    }
    if (!desc1 || !desc2 || !out || cols < 1 || rows2 < 2) return MLPL_E_BAD_INPUT;
    MLPL_HIP_TRY(hipSetDevice(ctx->device));
    const size_t elem = desc_type == 0 ? 1 : 4;
    if (step1 < (size_t)cols * elem || step2 < (size_t)cols * elem) return MLPL_E_BAD_INPUT;
    const int k = 2;  // K = 2 always (nmslib_matchers.h:182)
    void *dq, *dt, *didx, *ddist, *dout, *dcnt;
    int rc;
    if ((rc = upload_rows(ctx, WS_AUX0, desc1, rows1, (size_t)cols * elem, step1, &dq))) return rc;
    if ((rc = upload_rows(ctx, WS_AUX1, desc2, rows2, (size_t)cols * elem, step2, &dt))) return rc;
    if ((rc = ws_get(ctx, WS_IDX, (size_t)rows1 * k * 4, &didx))) return rc;
    if ((rc = ws_get(ctx, WS_DIST, (size_t)rows1 * k * 4, &ddist))) return rc;
    if ((rc = ws_get(ctx, WS_MATCH, (size_t)rows1 * sizeof(mlpl_dmatch), &dout))) return rc;
    if ((rc = ws_get(ctx, WS_SCALARS, 64, &dcnt))) return rc;
    if (desc_type == 0) {
        // two bytes per int, last int dropped by SpaceBitHamming::HiddenDistance: the last 2 bytes (1 for odd widths) are ignored
        const int eff = (cols % 2 == 0) ? cols - 2 : cols - 1;
        if (eff < 1) return MLPL_E_BAD_INPUT;
        rc = launch_knn_hamming(ctx, (const uint8_t *)dq, rows1, cols, 0, (const uint8_t *)dt, rows2, cols, 0, eff, k, 1,
                                (int32_t *)didx, (int32_t *)ddist, ctx->stream);
    } else {
        rc = launch_knn_l2(ctx, (const float *)dq, rows1, cols, 0, (const float *)dt, rows2, cols, 0, cols, k, 1,
                           (int32_t *)didx, (float *)ddist, ctx->stream, /*nms_order=*/1);
    }
    if (rc) return rc;
    rc = launch_ratio_compact(ctx, (const int32_t *)didx, ddist, desc_type == 5, rows1, k, 1, 0.75f, (mlpl_dmatch *)dout,
                              (int32_t *)dcnt, ctx->stream, nullptr, ratio_test ? 1 : 2);
    if (rc) return rc;
    int32_t cnt = 0;
    MLPL_HIP_TRY(hipMemcpyAsync(&cnt, dcnt, 4, hipMemcpyDeviceToHost, ctx->stream));
    MLPL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (cnt > 0) MLPL_HIP_TRY(hipMemcpy(out, dout, (size_t)cnt * sizeof(mlpl_dmatch), hipMemcpyDeviceToHost));
    *n_out = cnt;
    return MLPL_OK;  // no minimum-match check on this branch of getMatches
} MLPL_ENTRY_END("mlpl_get_matches_bruteforce_nms")

}  // extern "C"
