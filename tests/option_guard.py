"""Test helper (imported by test modules, not a fixture file): every tuning knob mlpl_set_option accepts, with representative valid
values, and a guard that snapshots all of them through mlpl_get_option and restores all of them afterwards -- a test that fails half-way
leaves the next one on the library's own settings, not on a variant."""
import contextlib

# name -> valid values (ranges: both ends and a value inside); must name exactly what mlpl_set_option accepts (test_option_guard.py)
SETTABLE = {
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
    "rand_cache_max": (0, 1, 1 << 22),
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
    "hub_cohort": (0, 8, 512),
    "pair_batch_seq": (0, 1, 1024),
    "pair_batch_feed": (0, 1),
    "pair_batch_raw_cap": (0, 64, 1 << 22),
    "usac_lo_stepwise": (0, 1),
    "usac_lo_warm_start": (0, 1),
    "usac_first_batch": (0, 1, 128),
    "usac_lo5_fused_fit": (0, 1),
    "usac_sprt_fast": (0, 1),
    "ransac_host_table": (0, 1),
    "ransac_chunk": (0, 1, 32768),
}

# values mlpl_set_option must refuse (one or two per knob with a closed value set)
REJECTED = {
    "hamming_variant": (-1, 4), "hamming_mfma_qt": (3, 8), "hamming_mfma_blocks_per_cu": (0, 65), "hamming_mfma_lds": (3,),
    "hamming_mfma_prio": (2, 4), "hamming_mfma_prefetch": (1, 8), "hamming_split_rows": (2048,), "hamming_mfma_waves": (2, 32),
    "hamming_stamps": (3,), "l2_mfma_waves": (16,), "l2_mfma_blocks_per_cu": (17,), "hamming_qpl": (0, 3), "ransac_count_mpl": (3,),
    "ransac_count_tiles": (0, 4), "ransac_count_threads": (128, 1024), "ransac_count_wpe": (4, 7), "ransac_dev_split": (901,),
    "arrsac_flag_points": (100,), "hub_cohort": (4,), "pair_batch_raw_cap": (32,), "ransac_chunk": (32769,),
}


def snapshot(ctx) -> dict:
    return {name: ctx.get_option(name) for name in SETTABLE}


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
