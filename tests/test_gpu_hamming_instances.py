"""Every selectable Hamming 2-NN kernel instance against the oracle, bit for bit, with the instance each option set names asserted through
mlpl_debug_last_kernels (a silent fallback to another instance would make a case vacuous).

Record fields (include/mlpl_debug.h): [2] kernel (0-2 VALU, 3 register-prefetch MFMA, 4 static LDS ring, 5 dynamic ring), [3] query tiles
per wave / queries per lane, [4] PRIO, [5] waves per workgroup, [6] prefetch distance, [7] fused merge, [8] split table, [9] fine expand,
[10] train splits, [11] K-steps, [12] in-kernel train expansion."""
import numpy as np
import pytest

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import _lib, synth
from hamming_cases import check_hamming_cases
from option_guard import options

pytestmark = pytest.mark.gpu

KIND, QT, PRIO, NWV, PD, FUSED, TAB, FINE, NSPLIT, KS, INKERNEL = range(2, 13)

# name -> (options, {record field: value} on the 32-byte-descriptor calls with >= 32 train rows)
# Precedence of the static ring kernel's options (knn_hamming_mfma.hip): waves 16 beats prefetch 4 / 6, which beats prio; prefetch and
# prio 3 exist with 8 waves only and are ignored with 4 (prio 0 runs).
OPTION_SETS = {
    "qt4_waves4": (dict(hamming_mfma_qt=4, hamming_mfma_waves=4), {KIND: 4, QT: 4, NWV: 4, PRIO: 0, PD: 2}),
    "qt4_waves8": (dict(hamming_mfma_qt=4, hamming_mfma_waves=8), {KIND: 4, QT: 4, NWV: 8, PRIO: 0, PD: 2}),
    "qt4_waves16": (dict(hamming_mfma_qt=4, hamming_mfma_waves=16), {KIND: 4, QT: 4, NWV: 16, PRIO: 0, PD: 2}),
    "prefetch4": (dict(hamming_mfma_qt=4, hamming_mfma_prefetch=4), {KIND: 4, NWV: 8, PD: 4, PRIO: 0}),
    "prefetch6": (dict(hamming_mfma_qt=4, hamming_mfma_prefetch=6), {KIND: 4, NWV: 8, PD: 6, PRIO: 0}),
    "prio1_qt4": (dict(hamming_mfma_qt=4, hamming_mfma_prio=1), {KIND: 4, NWV: 8, PD: 2, PRIO: 1}),
    "prio3_qt4": (dict(hamming_mfma_qt=4, hamming_mfma_prio=3), {KIND: 4, NWV: 8, PD: 2, PRIO: 3}),
    "prio1_qt2": (dict(hamming_mfma_qt=2, hamming_mfma_prio=1), {KIND: 4, QT: 2, NWV: 4, PRIO: 1}),
    "prio3_qt2": (dict(hamming_mfma_qt=2, hamming_mfma_prio=3), {KIND: 4, QT: 2, NWV: 4, PRIO: 0}),
    "prio1_qt1": (dict(hamming_mfma_qt=1, hamming_mfma_prio=1), {KIND: 4, QT: 1, NWV: 4, PRIO: 1}),
    "prio3_qt1": (dict(hamming_mfma_qt=1, hamming_mfma_prio=3), {KIND: 4, QT: 1, NWV: 4, PRIO: 0}),
    "waves16_beats_prefetch_and_prio": (dict(hamming_mfma_qt=4, hamming_mfma_waves=16, hamming_mfma_prefetch=4, hamming_mfma_prio=3),
                                        {KIND: 4, NWV: 16, PD: 2, PRIO: 0}),
    "prefetch_beats_prio": (dict(hamming_mfma_qt=4, hamming_mfma_prefetch=6, hamming_mfma_prio=1), {KIND: 4, NWV: 8, PD: 6, PRIO: 0}),
    "waves4_ignores_prefetch_and_prio3": (dict(hamming_mfma_qt=4, hamming_mfma_waves=4, hamming_mfma_prefetch=4, hamming_mfma_prio=3),
                                          {KIND: 4, NWV: 4, PD: 2, PRIO: 0}),
    "lds0_register_prefetch": (dict(hamming_mfma_lds=0), {KIND: 3, KS: 4}),
    "lds2_dynamic": (dict(hamming_mfma_lds=2), {KIND: 5, KS: 4}),
    "fused_merge0": (dict(hamming_mfma_qt=2, hamming_fused_merge=0), {KIND: 4, FUSED: 0}),
    "fused_merge1": (dict(hamming_mfma_qt=2, hamming_fused_merge=1), {KIND: 4, FUSED: 1}),
    "mfma_blocks_per_cu1": (dict(hamming_mfma_blocks_per_cu=1), {KIND: 4}),
    "mfma_blocks_per_cu8": (dict(hamming_mfma_blocks_per_cu=8), {KIND: 4}),
    "mfma_blocks_per_cu64": (dict(hamming_mfma_blocks_per_cu=64), {KIND: 4}),
    "valu_blocks_per_cu1": (dict(hamming_variant=0, hamming_blocks_per_cu=1), {KIND: 0}),
    "valu_blocks_per_cu8": (dict(hamming_variant=0, hamming_blocks_per_cu=8), {KIND: 0}),
    "valu_blocks_per_cu64": (dict(hamming_variant=0, hamming_blocks_per_cu=64), {KIND: 0}),
    "stamps1": (dict(hamming_stamps=1), {KIND: 4}),
    "stamps2": (dict(hamming_stamps=2), {KIND: 4}),
    "variant1_qpl2": (dict(hamming_variant=1, hamming_qpl=2), {KIND: 1}),
    # paths of the shared key decode that no row above pins: the pop(query) - ip rule of the {0, +1} train operand (never expanded in the
    # kernel) and, under hamming_split_rows, the decode's frame with several splits (asserted below)
    "train01": (dict(hamming_train01=1), {KIND: 4, INKERNEL: 0}),
    "split_rows4096": (dict(hamming_split_rows=4096), {KIND: 4}),
}


@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_hamming_instance_bit_exact(ctx, oracle, name):
    opts, expect = OPTION_SETS[name]
    seen = []

    def after_call(nq, nt, nbytes):
        rec = ctx.last_kernels()
        if nbytes == 32 and nt >= 32:
            got = {f: rec[f] for f in expect}
            assert got == expect, (name, nq, nt, rec)
            if name == "split_rows4096" and nt == 4097:   # several splits (the launcher cuts this shape far below the cap anyway)
                assert rec[NSPLIT] >= 2, rec
            seen.append(rec)

    with options(ctx, **opts):
        check_hamming_cases(ctx, oracle, name, after_call)
        if name == "variant1_qpl2":   # two queries per lane only above 8192 queries
            q, t = synth.orb_pair(8200, 700, seed=8200)
            idx, dist = mpa.knn_hamming(q, t, ctx=ctx)
            rec = ctx.last_kernels()
            assert (rec[KIND], rec[QT]) == (1, 2), rec
            oi, od = oracle.knn_hamming(q, t)
            assert np.array_equal(idx, oi) and np.array_equal(dist, od)
    assert seen, name


def test_hamming_mfma_prio_2_is_refused(ctx):
    """prio 2 was a diagnostic that streamed the same train tiles into every workgroup (wrong results by design): no longer selectable."""
    with options(ctx):
        with pytest.raises(_lib.MlplError):
            ctx.set_option("hamming_mfma_prio", 2)
        assert ctx.get_option("hamming_mfma_prio") == 0


@pytest.mark.parametrize("fine", [0, 1])
def test_hamming_expand_fine_at_the_latency_shape(ctx, oracle, fine):
    """One image pair of 2048 x 2048 ORB descriptors (the single-pair latency shape): the train set expanded by the fine kernel or the
    coarse one, same pairs."""
    q, t = synth.orb_pair(2048, 2048, seed=606)
    with options(ctx, hamming_expand_fine=fine):
        idx, dist = mpa.knn_hamming(q, t, ctx=ctx)
        rec = ctx.last_kernels()
    assert rec[KIND] == 4 and rec[FINE] == fine, rec
    oi, od = oracle.knn_hamming(q, t)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od)


@pytest.mark.parametrize("weighted", [0, 1])
def test_hamming_age_weighted_split_table(ctx, oracle, weighted):
    """A shape at which the launcher builds the age-aware split table: 512 queries (one query tile per wave, four query blocks) against
    32 rows per CU, i.e. exactly four workgroups per CU with one split each; the table moves the split boundaries, never the pairs."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nt = 32 * min(cus, 256)
    q, t = synth.orb_pair(512, nt, seed=512 + nt)
    with options(ctx, hamming_mfma_weighted=weighted):
        idx, dist = mpa.knn_hamming(q, t, ctx=ctx)
        rec = ctx.last_kernels()
    assert rec[KIND] == 4 and rec[NWV] == 4 and rec[TAB] == weighted, rec
    oi, od = oracle.knn_hamming(q, t)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od)


@pytest.mark.parametrize("bpc", [1, 4, 16])
def test_l2_matrix_core_blocks_per_cu(ctx, oracle, bpc):
    """l2_mfma_blocks_per_cu on the forced int8 matrix-core path (integer descriptors) and the fp16 candidate path (fractional ones)."""
    qi, ti = synth.sift_pair(900, 3000, dim=128, seed=77 + bpc)
    ti[5] = ti[2]
    qi[0] = ti[2]
    qf, tf = qi + 0.25, ti.copy()
    tf[11, 3] += 0.5
    sub = np.arange(0, 900, 7)
    with options(ctx, l2_mfma_blocks_per_cu=bpc):
        _lib.check(ctx.lib.mlpl_set_l2_path(ctx.handle, 2), "set_l2_path")
        try:
            idx, dist = mpa.knn_l2sq(qi, ti, ctx=ctx)
        finally:
            _lib.check(ctx.lib.mlpl_set_l2_path(ctx.handle, 0), "set_l2_path")
        oi, od = oracle.knn_l2sq(qi[sub], ti)
        assert np.array_equal(idx[sub], oi) and dist[sub].tobytes() == od.tobytes()
        with options(ctx, l2_float_mfma=2):
            idx, dist = mpa.knn_l2sq(qf, tf, ctx=ctx)
        oi, od = oracle.knn_l2sq(qf[sub], tf)
        assert np.array_equal(idx[sub], oi) and dist[sub].tobytes() == od.tobytes()
