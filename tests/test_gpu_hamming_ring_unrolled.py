"""The unrolled steady state of the eight-wave LDS-ring Hamming kernel with the in-kernel train expansion (knn_hamming_mfma.hip, instance
<4, 0, 8, 2, XP>): a split's tiles run in pairs while a whole pair with its copies two tiles ahead fits, and a rolled tail takes the rest
(an odd tile, the last two tiles, the ragged tile).  Every case is bit-exact in (idx, dist) against the oracle AND against the same call
with the separate expansion kernel (hamming_expand_inkernel = 0, the four-slot fragment ring), and every call asserts through
mlpl_debug_last_kernels that the instance ran: kernel 4, four query tiles per wave, eight waves, prefetch distance 2, field 12 = the option.

How many tiles a workgroup walks through is the launcher's choice: it cuts the train set until the chip is full, so ONE pair of 1024 queries
gets one split per tile whatever hamming_mfma_blocks_per_cu says (the ring kernel never goes below four workgroups per CU).  The cases named
`single_pair` are therefore prologue / ragged-tile / ticket-merge cases; the cases named `one_split` run the same train sizes on 2 x CUs pairs
through the batched device entry, where the chip is full with one split per pair and a workgroup really walks through T tiles -- the record's
split count is asserted, so that they cannot turn vacuous."""
import ctypes as C
import functools

import numpy as np
import pytest

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import synth
from matchinglib_poselib_amd.matching import match_hamming_device
from option_guard import options

pytestmark = pytest.mark.gpu

KIND, QT, NWV, PD, TAB, NSPLIT, INKERNEL = 2, 3, 5, 6, 8, 10, 12
FORCE = dict(hamming_mfma_qt=4, hamming_mfma_waves=8)
NQ = 1024
T_MAX = 9


def _assert_instance(rec, inkernel):
    assert (rec[KIND], rec[QT], rec[NWV], rec[PD]) == (4, 4, 8, 2), rec
    assert rec[INKERNEL] == inkernel, rec


def _knn(ctx, q, t, k, inkernel, **extra):
    with options(ctx, **FORCE, **extra, hamming_expand_inkernel=inkernel):
        idx, dist = mpa.knn_hamming(q, t, k=k, ctx=ctx)
        rec = ctx.last_kernels()
    _assert_instance(rec, inkernel)
    return idx, dist, rec


def _both(ctx, oracle, q, t, k=2, **extra):
    """One pair through both paths and the oracle."""
    new_i, new_d, rec = _knn(ctx, q, t, k, 1, **extra)
    old_i, old_d, _ = _knn(ctx, q, t, k, 0, **extra)
    oi, od = oracle.knn_hamming(q, t, k=k)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d), (len(q), len(t))
    assert np.array_equal(new_i, oi) and np.array_equal(new_d, od), (len(q), len(t))
    return rec


def _batched(ctx, dq, dt, inkernel, k=2, **extra):
    with options(ctx, **FORCE, **extra, hamming_expand_inkernel=inkernel):
        out = match_hamming_device(dq, dt, ratio_test=k == 2, ctx=ctx)
        rec = ctx.last_kernels()
    _assert_instance(rec, inkernel)
    return {k: v.cpu().numpy() for k, v in out.items()}, rec


def _batched_both(ctx, oracle, dq, dt, hq, ht, check_pairs, k=2, **extra):
    """A batch through both paths (everything equal) and the oracle on the pairs `check_pairs`; hq / ht are the host copies."""
    new, rec = _batched(ctx, dq, dt, 1, k=k, **extra)
    old, _ = _batched(ctx, dq, dt, 0, k=k, **extra)
    assert np.array_equal(new["idx"], old["idx"]) and np.array_equal(new["dist"], old["dist"])
    assert np.array_equal(new["count"], old["count"])
    for b in range(len(hq)):
        c = int(new["count"][b])
        assert np.array_equal(new["matches"][b, :c], old["matches"][b, :c]), b
    for b in check_pairs:
        oi, od = oracle.knn_hamming(hq[b], ht[b], k=k)
        assert np.array_equal(new["idx"][b], oi) and np.array_equal(new["dist"][b], od), b
    return new, rec


@functools.lru_cache(maxsize=None)
def _full_chip_batch():
    """2 x CUs pairs of NQ queries against up to 32 T_MAX train rows, on the device and on the host: with this many pairs the launcher leaves
    every pair's train set in ONE split.  Random bytes; a few duplicated train rows per pair (ties: the smaller index wins)."""
    import torch
    dev = torch.device("cuda", 0)
    B = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(20261)
    hq = rng.integers(0, 256, (B, NQ, 32), dtype=np.uint8)
    ht = rng.integers(0, 256, (B, 32 * T_MAX, 32), dtype=np.uint8)
    ht[:, 40] = ht[:, 3]
    ht[:, 32 * T_MAX - 1] = ht[:, 100]
    hq[:, 5] = ht[:, 3]
    hq.setflags(write=False)
    ht.setflags(write=False)
    return torch.tensor(hq).to(dev), torch.tensor(ht).to(dev), hq, ht


def _train_sizes():
    out = []
    for T in range(1, T_MAX + 1):
        out += [(T, "full", 32 * T), (T, "ragged_minus1", 32 * T - 1), (T, "ragged_plus1", 32 * (T - 1) + 1)]
    return out


@pytest.mark.parametrize("T,shape,nt", _train_sizes(), ids=lambda v: str(v))
def test_tiles_per_split_one_split(ctx, oracle, T, shape, nt):
    """T = 1 ... 9 tiles in the one split of every pair: fewer tiles than the prefetch distance, no pair, one pair, pairs plus an odd tile, each
    with a full last tile, a last tile short of one row and a last tile of one row.  The train sets are slices of a larger tensor (batch stride
    above nt rows).  (A train set of ONE row has no second neighbour, and the library refuses k = 2 there: that size runs with k = 1.)"""
    dq, dt_all, hq, ht = _full_chip_batch()
    dt = dt_all[:, :nt]
    B = len(hq)
    new, rec = _batched_both(ctx, oracle, dq, dt, hq, ht[:, :nt], (0, B - 1), k=min(2, nt), hamming_mfma_blocks_per_cu=1)
    assert rec[NSPLIT] == 1, rec


@pytest.mark.parametrize("T,shape,nt", _train_sizes(), ids=lambda v: str(v))
def test_tiles_per_split_single_pair(ctx, oracle, T, shape, nt):
    """The same train sizes for ONE pair of 1024 queries with hamming_mfma_blocks_per_cu = 1 (see the module text: one tile per split)."""
    _, _, hq, ht = _full_chip_batch()
    _both(ctx, oracle, hq[1], ht[1, :nt], k=min(2, nt), hamming_mfma_blocks_per_cu=1)


@functools.lru_cache(maxsize=None)
def _pair(nq, nt):
    q, t = synth.orb_pair(nq, nt, seed=31000 + 3 * nq + nt)
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("nq", [1, 1025])
@pytest.mark.parametrize("nt", [96, 160, 257])
def test_one_tile_per_split(ctx, oracle, nt, nq, k):
    """Deep splits, as small shapes get them by default: every workgroup runs the prologue and one (full or ragged) tile."""
    q, t = _pair(nq, nt)
    rec = _both(ctx, oracle, q, t, k=k)
    assert rec[NSPLIT] == (nt + 31) // 32, rec


def test_split_boundaries_off_the_unroll_4097(ctx, oracle):
    """4097 train rows: 129 tiles in splits whose boundaries are no multiple of the unroll, the last split ending on a one-row tile."""
    q, t = _pair(1024, 4097)
    _both(ctx, oracle, q, t)


def test_split_boundaries_off_the_unroll_4097_batched(ctx, oracle):
    """The same train size for 64 pairs, where the launcher cuts it into a few splits of 17 tiles (the single pair above gets one tile per
    split): odd splits starting at odd multiples of 17 tiles, the last one shorter and ending on the one-row tile."""
    import torch
    B, nt = 64, 4097
    rng = np.random.default_rng(4097)
    hq = rng.integers(0, 256, (B, NQ, 32), dtype=np.uint8)
    ht = rng.integers(0, 256, (B, nt, 32), dtype=np.uint8)
    ht[:, nt - 1] = ht[:, 7]
    hq[:, 9] = ht[:, 7]
    dev = torch.device("cuda", 0)
    _, rec = _batched_both(ctx, oracle, torch.from_numpy(hq).to(dev), torch.from_numpy(ht).to(dev), hq, ht, (0, B - 1))
    tiles = (nt + 31) // 32
    assert 1 < rec[NSPLIT] < tiles, rec   # (eight splits of 17 tiles on 256 CUs)


def test_split_boundaries_age_table_geometry(ctx, oracle):
    """The geometry of test_hamming_age_weighted_split_table (512 queries against 32 rows per CU, the weighted table asked for) forced to
    the eight-wave instance.  The launcher builds the table for four-wave workgroups only, so the record must say that none was used:
    the kernel under test cannot be reached with one."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nt = 32 * min(cus, 256)
    q, t = _pair(512, nt)
    rec = _both(ctx, oracle, q, t, hamming_mfma_weighted=1)
    assert rec[TAB] == 0, rec


def test_ties_and_extremes_single_pair(ctx, oracle):
    """Five distinct descriptors (the smaller train index must win everywhere), all-zero and all-ones rows."""
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    z = np.zeros((70, 32), np.uint8)
    o = np.full((90, 32), 255, np.uint8)
    cases = [(base[rng.integers(0, 5, 500)], base[rng.integers(0, 5, 3000)]), (z, o), (z, z[:40]), (o, np.concatenate([z[:45], o[:3]]))]
    for q, t in cases:
        _both(ctx, oracle, q, t)


@pytest.mark.parametrize("nt", [32 * 7, 32 * 6 + 5, 32 * 8, 32 * 4 + 1])
def test_last_row_is_the_best_match_one_split(ctx, oracle, nt):
    """One split of several tiles per pair whose LAST train row is the unique best match of every query (distance 0; all other rows are
    random, and all-zero / all-ones rows sit in the first and in the second-to-last tile): a clamp or a peeled tail that drops the last
    row or the last tile loses every first neighbour."""
    import torch
    dq_all, dt_all, hq, ht = _full_chip_batch()
    B = len(hq)
    rng = np.random.default_rng(nt)
    p = rng.integers(0, 256, (B, 1, 32), dtype=np.uint8)
    hq2 = np.broadcast_to(p, (B, NQ, 32)).copy()
    ht2 = ht[:, :nt].copy()
    ht2[:, nt - 1] = p[:, 0]
    ht2[:, 1] = 0
    ht2[:, nt - 34] = 255
    dev = dq_all.device
    new, rec = _batched_both(ctx, oracle, torch.from_numpy(hq2).to(dev), torch.from_numpy(ht2).to(dev), hq2, ht2, (0, B - 1))
    assert rec[NSPLIT] == 1, rec
    assert (new["idx"][:, :, 0] == nt - 1).all() and (new["dist"][:, :, 0] == 0).all()


def test_batch_of_three_with_padded_batch_stride(ctx, oracle):
    """Three pairs with different train sets that are slices of a larger tensor: a source offset carried from one pair to the next, or a copy
    that is not clamped to the pair's own rows, shows here."""
    import torch
    B, nq, nt = 3, 1025, 300
    dev = torch.device("cuda", 0)
    qs, ts = zip(*[synth.orb_pair(nq, nt, seed=8900 + p) for p in range(B)])
    hq, ht = np.stack(qs), np.stack(ts)
    big = torch.full((B, nt + 40, 32), 0xA5, dtype=torch.uint8, device=dev)
    big[:, 8:8 + nt] = torch.from_numpy(ht).to(dev)
    dt = big[:, 8:8 + nt]
    assert dt.stride(0) > nt * 32
    _batched_both(ctx, oracle, torch.from_numpy(hq).to(dev), dt, hq, ht, range(B))


def test_stamps_keep_their_per_tile_records(ctx, oracle):
    """hamming_stamps = 1 runs the stamped (rolled) instance: same pairs, and the per-tile clock trace tools/hamming_trace.py reads holds a
    non-zero record for each of the nine tiles of every wave and nothing behind them."""
    dq, dt_all, hq, ht = _full_chip_batch()
    B = len(hq)
    plain, _ = _batched(ctx, dq, dt_all, 1)
    with options(ctx, **FORCE, hamming_stamps=1, hamming_expand_inkernel=1):
        out = match_hamming_device(dq, dt_all, ctx=ctx)
        rec = ctx.last_kernels()
        _assert_instance(rec, 1)
        assert rec[NSPLIT] == 1, rec
        stamped = {k: v.cpu().numpy() for k, v in out.items()}
        fn = ctx.lib.mlpl_debug_hamming_stamps
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        waves = B * (NQ // (32 * 4 * 8)) * 8
        recs = np.zeros((waves + 8, 4), np.uint64)
        m = fn(ctx.handle, recs.ctypes.data, len(recs))
        trace = np.zeros((m, 48), np.uint64)
        m2 = fn(ctx.handle, trace.ctypes.data, -m)
    assert m == waves and m2 == waves, (m, m2, waves)
    for key in ("idx", "dist", "count"):
        assert np.array_equal(stamped[key], plain[key]), key
    assert (recs[:m, 0] > 0).all() and ((recs[:m, 2] & np.uint64(0xFFFFFFFF)) == T_MAX * 4).all()
    assert (trace[:, :T_MAX] > 0).all() and (trace[:, T_MAX:] == 0).all()
    assert (np.diff(trace[:, :T_MAX].astype(np.int64), axis=1) > 0).all()
    oi, od = oracle.knn_hamming(hq[0], ht[0])
    assert np.array_equal(stamped["idx"][0], oi) and np.array_equal(stamped["dist"][0], od)


def test_one_pair_8192_by_8192(ctx, oracle):
    """The benchmark's pair shape, one pair: the launcher's splits hold a few tiles each (a pair of tiles and a rolled tail)."""
    q, t = _pair(8192, 8192)
    new_i, new_d, rec = _knn(ctx, q, t, 2, 1)
    old_i, old_d, _ = _knn(ctx, q, t, 2, 0)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d)
    sub = np.arange(0, 8192, 5)
    oi, od = oracle.knn_hamming(q[sub], t)
    assert np.array_equal(new_i[sub], oi) and np.array_equal(new_d[sub], od)
