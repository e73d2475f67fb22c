"""The 16x16x128 form of the throughput instance of the Hamming LDS-ring kernel (knn_hamming_mfma_lds16_kernel in knn_hamming_mfma.hip, option
hamming_mfma_shape = 16): the tile arithmetic runs on v_mfma_f32_16x16x128_f8f6f4 -- two chains of two per 16 queries, the accumulators of a
pair of tiles 32 * 2^-14 apart and one re-base of the running pairs per pair -- the fragments sit elsewhere in LDS and a query's keys in four
lanes instead of two.  Every output must be what the 32x32x64 instance gives.

Every case is bit-exact in (idx, dist) against the oracle AND against the same call with hamming_mfma_shape = 32, and every call asserts
through mlpl_debug_last_hamming_shape that the shape asked for ran, beside the instance record of mlpl_debug_last_kernels -- a silent
fall-back cannot make a case vacuous.  That the opcode's internal sum of 128 products plus a C carrying 2^-14 steps is exact at these
magnitudes is what the cases with extreme values check, not an assumption.  As in test_gpu_hamming_acc_bias.py each case runs in two forms:
`single_pair` (one pair of 1024 queries: one split per tile -- prologue, ragged tile, partial table, ticket merge) and `one_split` (2 x CUs
pairs through the batched device entry: one split per pair, a workgroup walks through all tiles; the oracle checks 8 of the pairs).

The cases: distance 0 in every tile (the largest value, ties decided by the row across lane groups and row halves), distance 256, the only
zero-distance rows on the first and last row of a full split, ragged last tiles around every lane-group and row-half boundary, a second
neighbour hidden in the best row's block at each of the three other offsets, in the same lane's other row half (+16) and in another lane
group (+4), the clusters of test_gpu_hamming_block_top2.py, zero / one pair of tiles with and without an odd tile, four pairs with a rolled
tail and a ragged tile, a ragged query group, a padded batch stride, one neighbour, and the benchmark's pair shape."""
import functools

import numpy as np
import pytest

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import synth
from matchinglib_poselib_amd.matching import match_hamming_device
from option_guard import options
from test_gpu_hamming_block_top2 import clustered_pair

pytestmark = pytest.mark.gpu

KIND, QT, NWV, PD, NSPLIT, INKERNEL = 2, 3, 5, 6, 10, 12
FORCE = dict(hamming_mfma_qt=4, hamming_mfma_waves=8)
NQ = 1024
FULL = 8192   # rows of a full split
N_CHECK = 8   # pairs of a batch the oracle checks


def _assert_instance(ctx, shape):
    rec = ctx.last_kernels()
    assert (rec[KIND], rec[QT], rec[NWV], rec[PD], rec[INKERNEL]) == (4, 4, 8, 2, 1), rec
    assert ctx.last_hamming_top2() == 4, ctx.last_hamming_top2()
    assert ctx.last_hamming_shape() == shape, (ctx.last_hamming_shape(), shape)
    return rec


def _knn(ctx, q, t, k, shape, **extra):
    with options(ctx, **FORCE, **extra, hamming_mfma_shape=shape):
        idx, dist = mpa.knn_hamming(q, t, k=k, ctx=ctx)
        rec = _assert_instance(ctx, shape)
    return idx, dist, rec


def _single_pair(ctx, oracle, q, t, k=2, **extra):
    """One pair through both shapes and the oracle; one split per tile."""
    new_i, new_d, rec = _knn(ctx, q, t, k, 16, hamming_mfma_blocks_per_cu=1, **extra)
    old_i, old_d, _ = _knn(ctx, q, t, k, 32, hamming_mfma_blocks_per_cu=1, **extra)
    oi, od = oracle.knn_hamming(q, t, k=k)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d), (len(q), len(t))
    assert np.array_equal(new_i, oi) and np.array_equal(new_d, od), (len(q), len(t))
    assert rec[NSPLIT] == (len(t) + 31) // 32, rec
    return new_i, new_d


def _batched(ctx, dq, dt, shape, k, **extra):
    with options(ctx, **FORCE, hamming_mfma_blocks_per_cu=1, **extra, hamming_mfma_shape=shape):
        out = match_hamming_device(dq, dt, ratio_test=k == 2, ctx=ctx)
        rec = _assert_instance(ctx, shape)
        out = {key: v.cpu().numpy() for key, v in out.items()}
    return out, rec


def _one_split(ctx, oracle, dq, dt, hq, ht, k=2, nsplit=1, **extra):
    """A batch through both shapes (everything equal) and the oracle on N_CHECK pairs; hq / ht are the host copies."""
    new, rec = _batched(ctx, dq, dt, 16, k, **extra)
    old, _ = _batched(ctx, dq, dt, 32, k, **extra)
    assert rec[NSPLIT] == nsplit, rec
    for key in ("idx", "dist", "count"):
        assert np.array_equal(new[key], old[key]), key
    for b in range(len(hq)):
        c = int(new["count"][b])
        assert np.array_equal(new["matches"][b, :c], old["matches"][b, :c]), b
    for b in _check_pairs(len(hq)):
        oi, od = oracle.knn_hamming(hq[b], ht[b], k=k)
        assert np.array_equal(new["idx"][b], oi) and np.array_equal(new["dist"][b], od), b
    return new


def _check_pairs(B):
    return sorted(set(int(b) for b in np.linspace(0, B - 1, N_CHECK)))


def _batch_size():
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a)).to(torch.device("cuda", 0))   # (a copy: the shared host arrays are read-only)


@functools.lru_cache(maxsize=None)
def _random_batch():
    """2 x CUs pairs of NQ random queries and FULL random train rows (host, read-only), one pattern per pair, and the device copy of the train
    rows: with this many pairs the launcher leaves every pair's train set in one split.  Shared by the cases; nobody writes to it."""
    B = _batch_size()
    rng = np.random.default_rng(20280)
    hq = rng.integers(0, 256, (B, NQ, 32), dtype=np.uint8)
    ht = rng.integers(0, 256, (B, FULL, 32), dtype=np.uint8)
    pat = rng.integers(0, 256, (B, 1, 32), dtype=np.uint8)
    for a in (hq, ht, pat):
        a.setflags(write=False)
    return hq, ht, pat, _dev(ht)


def _same_queries(pat):
    """every query of a pair = the pair's pattern"""
    return np.ascontiguousarray(np.broadcast_to(pat, (len(pat), NQ, 32)))


# ---- distance 0 in every tile: the largest value; ties decided by the row across lane groups and row halves --------------------------------

@pytest.mark.parametrize("nt", [64, FULL])
def test_identical_rows_one_split(ctx, oracle, nt):
    _, _, pat, _ = _random_batch()
    hq = _same_queries(pat)
    ht = np.ascontiguousarray(np.broadcast_to(pat, (len(pat), nt, 32)))
    new = _one_split(ctx, oracle, _dev(hq), _dev(ht), hq, ht)
    assert (new["idx"] == np.array([0, 1])).all() and (new["dist"] == 0).all()


@pytest.mark.parametrize("nt", [64, FULL])
def test_identical_rows_single_pair(ctx, oracle, nt):
    _, _, pat, _ = _random_batch()
    q = np.ascontiguousarray(np.broadcast_to(pat[1], (NQ, 32)))
    t = np.ascontiguousarray(np.broadcast_to(pat[1], (nt, 32)))
    idx, dist = _single_pair(ctx, oracle, q, t)
    assert (idx == np.array([0, 1])).all() and (dist == 0).all()


# ---- distance 256: the smallest value -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [2, 33])
def test_complement_rows_one_split(ctx, oracle, nt):
    _, _, pat, _ = _random_batch()
    hq = _same_queries(pat)
    ht = np.ascontiguousarray(np.broadcast_to(~pat, (len(pat), nt, 32)))
    new = _one_split(ctx, oracle, _dev(hq), _dev(ht), hq, ht)
    assert (new["idx"] == np.array([0, 1])).all() and (new["dist"] == 256).all()


@pytest.mark.parametrize("nt", [2, 33])
def test_complement_rows_single_pair(ctx, oracle, nt):
    _, _, pat, _ = _random_batch()
    q = np.ascontiguousarray(np.broadcast_to(pat[1], (NQ, 32)))
    t = np.ascontiguousarray(np.broadcast_to(~pat[1], (nt, 32)))
    idx, dist = _single_pair(ctx, oracle, q, t)
    assert (idx == np.array([0, 1])).all() and (dist == 256).all()


# ---- the only rows at distance 0 are the first and the last of a full split ----------------------------------------------------------------

def test_first_and_last_row_of_a_full_split_one_split(ctx, oracle):
    _, ht0, pat, _ = _random_batch()
    hq = _same_queries(pat)
    ht = ht0.copy()
    ht[:, 0] = pat[:, 0]
    ht[:, FULL - 1] = pat[:, 0]
    new = _one_split(ctx, oracle, _dev(hq), _dev(ht), hq, ht)
    assert (new["idx"] == np.array([0, FULL - 1])).all() and (new["dist"] == 0).all()


def test_first_and_last_row_of_a_full_split_single_pair(ctx, oracle):
    _, ht0, pat, _ = _random_batch()
    q = np.ascontiguousarray(np.broadcast_to(pat[1], (NQ, 32)))
    t = ht0[1].copy()
    t[0] = pat[1, 0]
    t[FULL - 1] = pat[1, 0]
    idx, dist = _single_pair(ctx, oracle, q, t)
    assert (idx == np.array([0, FULL - 1])).all() and (dist == 0).all()


# ---- ragged last tiles around every lane-group and row-half boundary, the best match on the last row ----------------------------------------

RAGGED = [1, 15, 16, 17, 31, 33, 47, 49, FULL - 31]


@pytest.mark.parametrize("nt", RAGGED)
def test_ragged_last_tile_best_on_last_row_one_split(ctx, oracle, nt):
    """(A train set of one row has no second neighbour, and the library refuses k = 2 there: that size runs with k = 1.)"""
    _, ht0, pat, _ = _random_batch()
    hq = _same_queries(pat)
    ht = ht0[:, :nt].copy()
    ht[:, nt - 1] = pat[:, 0]
    new = _one_split(ctx, oracle, _dev(hq), _dev(ht), hq, ht, k=min(2, nt))
    assert (new["idx"][:, :, 0] == nt - 1).all() and (new["dist"][:, :, 0] == 0).all()


@pytest.mark.parametrize("nt", RAGGED)
def test_ragged_last_tile_best_on_last_row_single_pair(ctx, oracle, nt):
    _, ht0, pat, _ = _random_batch()
    q = np.ascontiguousarray(np.broadcast_to(pat[1], (NQ, 32)))
    t = ht0[1, :nt].copy()
    t[nt - 1] = pat[1, 0]
    idx, dist = _single_pair(ctx, oracle, q, t, k=min(2, nt))
    assert (idx[:, 0] == nt - 1).all() and (dist[:, 0] == 0).all()


# ---- a planted second: in the best row's block (offsets 1, 2, 3), in another lane group (+4), in the same lane's other row half (+16) --------

N_SMALL = 32 * 9 + 5   # four pairs of tiles, a rolled tail and a ragged tile


@functools.lru_cache(maxsize=None)
def planted_pair(off, seed):
    """Random rows; for every aligned block of four rows whose row + off exists, row 4 j + off is one bit from row 4 j (blocks taken so that no
    row is used twice).  Query i is row 4 j or row 4 j + off of block j = i mod blocks, alternating with i: its best is that row at distance
    0 and its second the other one at distance 1 -- for the first kind the LATER row, for the second the earlier one."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (N_SMALL, 32), dtype=np.uint8)
    bases, used = [], set()
    for r in range(0, N_SMALL - off, 4):
        if r in used or r + off in used:
            continue
        used |= {r, r + off}
        bases.append(r)
        t[r + off] = t[r]
        bit = int(rng.integers(0, 256))
        t[r + off, bit >> 3] ^= np.uint8(1 << (bit & 7))
    q = np.stack([t[bases[i % len(bases)] + ((i // len(bases)) & 1) * off] for i in range(NQ)])
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


@pytest.mark.parametrize("off", [1, 2, 3, 4, 16])
def test_planted_second_single_pair(ctx, oracle, off):
    q, t = planted_pair(off, 500 + off)
    idx, dist = _single_pair(ctx, oracle, q, t)
    assert (dist == np.array([0, 1])).all() and (np.abs(idx[:, 0] - idx[:, 1]) == off).all()


@pytest.mark.parametrize("off", [1, 2, 3, 4, 16])
def test_planted_second_one_split(ctx, oracle, off):
    B = _batch_size()
    pairs = [planted_pair(off, 600 + 10 * off + s) for s in range(3)]
    hq = np.stack([pairs[b % 3][0] for b in range(B)])
    ht = np.stack([pairs[b % 3][1] for b in range(B)])
    new = _one_split(ctx, oracle, _dev(hq), _dev(ht), hq, ht)
    assert (new["dist"] == np.array([0, 1])).all()


@pytest.mark.parametrize("nt", [98, 197, 288])
def test_block_top2_clusters_single_pair(ctx, oracle, nt):
    """The clustered train sets of test_gpu_hamming_block_top2.py (1000 queries: no multiple of 16)."""
    q, t = clustered_pair(1000, nt, 77 + nt)
    _single_pair(ctx, oracle, q, t)


@pytest.mark.parametrize("nt", [98, 197, 288])
def test_block_top2_clusters_one_split(ctx, oracle, nt):
    B = _batch_size()
    pairs = [clustered_pair(NQ, nt, 1000 * nt + s) for s in range(3)]
    hq = np.stack([pairs[b % 3][0] for b in range(B)])
    ht = np.stack([pairs[b % 3][1] for b in range(B)])
    _one_split(ctx, oracle, _dev(hq), _dev(ht), hq, ht)


# ---- tile counts: zero and one pair of tiles, an odd tile; four pairs, a rolled tail and a ragged tile -------------------------------------

@pytest.mark.parametrize("nt", [32, 64, 96, N_SMALL])
def test_tile_counts_one_split(ctx, oracle, nt):
    hq, ht0, _, dt0 = _random_batch()
    _one_split(ctx, oracle, _dev(hq), dt0[:, :nt], hq, ht0[:, :nt])


@pytest.mark.parametrize("nt", [32, 64, 96, N_SMALL])
def test_tile_counts_single_pair(ctx, oracle, nt):
    hq, ht0, _, _ = _random_batch()
    _single_pair(ctx, oracle, hq[1], ht0[1, :nt])


# ---- a ragged query group, a padded batch stride, one neighbour ----------------------------------------------------------------------------

def test_ragged_query_group_single_pair(ctx, oracle):
    hq, ht0, _, _ = _random_batch()
    _single_pair(ctx, oracle, hq[1, :NQ - 3], ht0[1, :N_SMALL])


def test_ragged_query_group_one_split(ctx, oracle):
    hq, ht0, _, dt0 = _random_batch()
    _one_split(ctx, oracle, _dev(hq[:, :NQ - 3]), dt0[:, :N_SMALL], hq[:, :NQ - 3], ht0[:, :N_SMALL])


def test_padded_batch_stride_one_split(ctx, oracle):
    """The train sets are slices of a larger tensor: rows 8 .. 8 + nt of FULL rows per pair."""
    hq, ht0, _, dt0 = _random_batch()
    dt = dt0[:, 8:8 + N_SMALL]
    assert dt.stride(0) > N_SMALL * 32
    _one_split(ctx, oracle, _dev(hq), dt, hq, ht0[:, 8:8 + N_SMALL])


def test_padded_batch_stride_single_pair(ctx, oracle):
    """A batch of one pair through the device entry (one split per tile), query and train rows both slices of larger tensors."""
    hq, ht0, _, dt0 = _random_batch()
    dq = _dev(hq[:2])[1:2, :NQ - 3]
    dt = dt0[1:2, 8:8 + N_SMALL]
    _one_split(ctx, oracle, dq, dt, hq[1:2, :NQ - 3], ht0[1:2, 8:8 + N_SMALL], nsplit=(N_SMALL + 31) // 32)


def test_one_neighbour_one_split(ctx, oracle):
    hq, ht0, _, dt0 = _random_batch()
    _one_split(ctx, oracle, _dev(hq), dt0[:, :N_SMALL], hq, ht0[:, :N_SMALL], k=1)


def test_one_neighbour_single_pair(ctx, oracle):
    hq, ht0, _, _ = _random_batch()
    _single_pair(ctx, oracle, hq[1], ht0[1, :N_SMALL], k=1)


# ---- where the option does not apply the 32x32 shape runs and says so ----------------------------------------------------------------------

def test_shape_ignored_by_the_stamped_and_the_per_candidate_instances(ctx):
    hq, ht0, _, _ = _random_batch()
    with options(ctx, **FORCE, hamming_stamps=1, hamming_mfma_shape=16):
        mpa.knn_hamming(hq[1], ht0[1, :N_SMALL], k=2, ctx=ctx)
        assert ctx.last_hamming_shape() == 32
    with options(ctx, hamming_block_top2=0, **FORCE, hamming_mfma_shape=16):
        mpa.knn_hamming(hq[1], ht0[1, :N_SMALL], k=2, ctx=ctx)
        assert ctx.last_hamming_shape() == 32


def test_option_values(ctx):
    before = ctx.get_option("hamming_mfma_shape")
    assert before in (16, 32)
    for bad in (0, 8, 24, 64):
        with pytest.raises(mpa.MlplError):
            ctx.set_option("hamming_mfma_shape", bad)
    assert ctx.get_option("hamming_mfma_shape") == before


# ---- the benchmark's pair shape ------------------------------------------------------------------------------------------------------------

def test_random_pair_8192_by_8192(ctx, oracle):
    q, t = synth.orb_pair(FULL, FULL, seed=20281)
    new_i, new_d, _ = _knn(ctx, q, t, 2, 16)
    old_i, old_d, _ = _knn(ctx, q, t, 2, 32)
    oi, od = oracle.knn_hamming(q, t, k=2)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d)
    assert np.array_equal(new_i, oi) and np.array_equal(new_d, od)
