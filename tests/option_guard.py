"""Test helper (imported by test modules, not a fixture file): a guard that snapshots EVERY tuning option of a context through
mlpl_get_option and restores all of them afterwards -- a test that fails half-way leaves the next one on the library's own settings,
not on a variant.  The guard takes the names from the library's option table (mlpl_option_info), so an option is guarded the moment
it has a row.  SETTABLE, REJECTED and DEFAULTS are test data: what test_option_guard.py expects of that table."""
import contextlib
import ctypes

from matchinglib_poselib_amd import _lib

# name -> valid values (ranges: both ends and a value inside)
SETTABLE = {
    "l2_fold_counts": (0, 1),
    "hamming_expand_inkernel": (0, 1),
    "hamming_block_top2": (0, 4),
    "hamming_mfma_shape": (16, 32),
    "vfc_store_u": (0, 1),
    "hamming_variant": (0, 1, 2, 3),
    "hamming_mfma_qt": (0, 1, 2, 4),
    "hamming_mfma_blocks_per_cu": (1, 3, 64),
    "hamming_mfma_lds": (0, 1, 2),
    "hamming_expand_fine": (0, 1),
    "hamming_mfma_prio": (0, 1, 3),
    "hamming_mfma_prefetch": (0, 2, 4, 6),
    "hamming_split_rows": (0, 4096, 8192),
    "hamming_mfma_waves": (0, 4, 8, 16),
    "hamming_mfma_weighted": (0, 1),
    "hamming_fused_merge": (0, 1),
    "hamming_stamps": (0, 1, 2),
    "hamming_train01": (0, 1),
    "hamming_merge_emit": (0, 1),
    "l2_mfma_waves": (0, 4, 8),
    "l2_mfma_blocks_per_cu": (0, 7, 16),
    "hamming_qpl": (1, 2),
    "hamming_blocks_per_cu": (1, 32, 64),
    "ransac_lazy_sums": (0, 1),
    "ransac_overlap": (0, 1),
    "ransac_dev_split": (0, 450, 900),
    "rand_cache_max": (0, 1, 1 << 22, 2**31 - 1),
    "ransac_f32_filter": (0, 1),
    "arrsac_refine_warm_start": (0, 1),
    "ransac_count_mpl": (1, 2),
    "ransac_count_tiles": (1, 2),
    "ransac_count_threads": (256, 512),
    "ransac_count_wpe": (5, 6),
    "ransac_count_defer": (0, 1),
    "ransac_event_cap": (0, 17, 1024),
    "solver_polish": (0, 1),
    "solver_wave3": (0, 1),
    "ransac_device_draw": (0, 1),
    "l2_float_mfma": (0, 1, 2),
    "arrsac_flag_points": (0, 128, 640, 1024),
    "pair_batch": (0, 1, 1024),
    "hub_lanes": (0, 3, 8),
    "eig_inverse_iteration": (0, 1),
    "hub_blocking_sync": (0, 1),
    "hub_workers": (0, 5, 64),
    "hub_cohort": (0, 8, 100, 512),
    "pair_batch_seq": (0, 1, 1024),
    "pair_batch_feed": (0, 1),
    "pair_batch_raw_cap": (0, 64, 4096, 1 << 22),
    "usac_lo_stepwise": (0, 1),
    "usac_lo_warm_start": (0, 1),
    "usac_first_batch": (0, 1, 128),
    "usac_lo5_fused_fit": (0, 1),
    "usac_sprt_fast": (0, 1),
    "ransac_host_table": (0, 1),
    "ransac_chunk": (0, 1, 32768),
}

# values mlpl_set_option must refuse: for every option that does not take all non-negative ints, one below, one above and one in
# every gap of a closed value set
REJECTED = {
    "l2_fold_counts": (-1, 2),
    "hamming_expand_inkernel": (-1, 2),
    "hamming_block_top2": (-1, 1, 2, 3, 5),
    "hamming_mfma_shape": (15, 17, 24, 33),
    "vfc_store_u": (-1, 2),
    "hamming_variant": (-1, 4),
    "hamming_mfma_qt": (-1, 3, 5, 8),
    "hamming_mfma_blocks_per_cu": (0, 65),
    "hamming_mfma_lds": (-1, 3),
    "hamming_expand_fine": (-1, 2),
    "hamming_mfma_prio": (-1, 2, 4),
    "hamming_mfma_prefetch": (-1, 1, 3, 5, 7, 8),
    "hamming_split_rows": (-1, 2048, 6144, 8193, 12288),
    "hamming_mfma_waves": (-1, 2, 6, 12, 17, 32),
    "hamming_mfma_weighted": (-1, 2),
    "hamming_fused_merge": (-1, 2),
    "hamming_stamps": (-1, 3),
    "hamming_train01": (-1, 2),
    "hamming_merge_emit": (-1, 2),
    "l2_mfma_waves": (-1, 2, 6, 9, 16),
    "l2_mfma_blocks_per_cu": (-1, 17),
    "hamming_qpl": (0, 3),
    "hamming_blocks_per_cu": (0, 65),
    "ransac_lazy_sums": (-1, 2),
    "ransac_overlap": (-1, 2),
    "ransac_dev_split": (-1, 901),
    "rand_cache_max": (-1,),
    "ransac_f32_filter": (-1, 2),
    "arrsac_refine_warm_start": (-1, 2),
    "ransac_count_mpl": (0, 3),
    "ransac_count_tiles": (0, 3, 4),
    "ransac_count_threads": (128, 255, 384, 513, 1024),
    "ransac_count_wpe": (4, 7),
    "ransac_count_defer": (-1, 2),
    "ransac_event_cap": (-1, 1025),
    "solver_polish": (-1, 2),
    "solver_wave3": (-1, 2),
    "ransac_device_draw": (-1, 2),
    "l2_float_mfma": (-1, 3),
    "arrsac_flag_points": (-1, 64, 100, 127, 192 + 1, 1025, 1088),
    "pair_batch": (-1, 1025),
    "hub_lanes": (-1, 9),
    "eig_inverse_iteration": (-1, 2),
    "hub_blocking_sync": (-1, 2),
    "hub_workers": (-1, 65),
    "hub_cohort": (-1, 4, 7, 513),
    "pair_batch_seq": (-1, 1025),
    "pair_batch_feed": (-1, 2),
    "pair_batch_raw_cap": (-1, 32, 63, (1 << 22) + 1),
    "usac_lo_stepwise": (-1, 2),
    "usac_lo_warm_start": (-1, 2),
    "usac_first_batch": (-1, 129),
    "usac_lo5_fused_fit": (-1, 2),
    "usac_sprt_fast": (-1, 2),
    "ransac_host_table": (-1, 2),
    "ransac_chunk": (-1, 32769),
}

# the library's defaults, written down independently of its table
DEFAULTS = {
    "l2_fold_counts": 1, "hamming_expand_inkernel": 1, "hamming_block_top2": 4, "hamming_mfma_shape": 16, "vfc_store_u": 0,
    "hamming_variant": 3, "hamming_mfma_qt": 0, "hamming_mfma_blocks_per_cu": 3, "hamming_mfma_lds": 1, "hamming_expand_fine": 1,
    "hamming_mfma_prio": 0, "hamming_mfma_prefetch": 0, "hamming_split_rows": 0, "hamming_mfma_waves": 0, "hamming_mfma_weighted": 1,
    "hamming_fused_merge": 1, "hamming_stamps": 0, "hamming_train01": 0, "hamming_merge_emit": 0, "l2_mfma_waves": 0,
    "l2_mfma_blocks_per_cu": 0, "hamming_qpl": 1, "hamming_blocks_per_cu": 32, "ransac_lazy_sums": 1, "ransac_overlap": 1,
    "ransac_dev_split": 0, "rand_cache_max": 0, "ransac_f32_filter": 1, "arrsac_refine_warm_start": 1, "ransac_count_mpl": 2,
    "ransac_count_tiles": 2, "ransac_count_threads": 256, "ransac_count_wpe": 5, "ransac_count_defer": 1, "ransac_event_cap": 0,
    "solver_polish": 1, "solver_wave3": 1, "ransac_device_draw": 1, "l2_float_mfma": 1, "arrsac_flag_points": 0, "pair_batch": 0,
    "hub_lanes": 0, "eig_inverse_iteration": 1, "hub_blocking_sync": 1, "hub_workers": 0, "hub_cohort": 0, "pair_batch_seq": 0,
    "pair_batch_feed": 1, "pair_batch_raw_cap": 0, "usac_lo_stepwise": 0, "usac_lo_warm_start": 1, "usac_first_batch": 0,
    "usac_lo5_fused_fit": 1, "usac_sprt_fast": 1, "ransac_host_table": 0, "ransac_chunk": 0,
}


def option_table() -> list:
    """[(name, default)] of every row of the library's option table, in its order (mlpl_option_info; needs no device)."""
    lib = _lib.load_library()
    rows, name, default = [], ctypes.c_char_p(), ctypes.c_int()
    while lib.mlpl_option_info(len(rows), ctypes.byref(name), ctypes.byref(default)) == _lib.MLPL_OK:
        rows.append((name.value.decode(), default.value))
    return rows


def snapshot(ctx) -> dict:
    return {name: ctx.get_option(name) for name, _ in option_table()}


def restore(ctx, snap: dict) -> None:
    for name, value in snap.items():
        ctx.set_option(name, value)


@contextlib.contextmanager
def options(ctx, **settings):
    """with options(ctx, ransac_count_wpe=6): ... -- sets the knobs, restores EVERY knob on the way out (exception or not)."""
    snap = snapshot(ctx)
    try:
        for name, value in settings.items():
            ctx.set_option(name, value)
        yield
    finally:
        restore(ctx, snap)
