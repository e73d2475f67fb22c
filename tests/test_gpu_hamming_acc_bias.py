"""The accumulator bias of the in-kernel-expansion instances of the Hamming LDS-ring kernel (kAccBias in knn_hamming_mfma.hip): their MFMA
chains start at kAccBias - row * 2^-14 and the decode removes the bias again, so every output must be what it was.  The cases sit where the
biased value is extreme or the decode is delicate: distance 0 in every tile (the largest value, in the last tile of a full 8192-row split the
largest the kernel can hold) with ties decided by the row, distance 256 (the smallest), best matches on the first and the last row of a full
split, ragged last tiles whose rows behind the train set stay at -inf, one neighbour, the stamped instance, a padded batch stride and the
benchmark's pair shape.

Every case is bit-exact in (idx, dist) against the oracle AND against the same call with hamming_expand_inkernel = 0 (an unbiased instance of
the same build), and every call asserts through mlpl_debug_last_kernels that the instance <4, 0, 8, 2> ran with / without the in-kernel
expansion.  As in test_gpu_hamming_ring_unrolled.py each case runs in two forms: `single_pair` (one pair of 1024 queries: the launcher cuts
the train set into one split per tile -- prologue, ragged tile, partial table and ticket merge) and `one_split` (2 x CUs pairs through the
batched device entry: one split per pair, a workgroup walks through all tiles; the oracle checks 8 of the pairs)."""
import functools

import numpy as np
import pytest

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import synth
from matchinglib_poselib_amd.matching import match_hamming_device
from option_guard import options

pytestmark = pytest.mark.gpu

KIND, QT, NWV, PD, NSPLIT, INKERNEL = 2, 3, 5, 6, 10, 12
FORCE = dict(hamming_mfma_qt=4, hamming_mfma_waves=8)
NQ = 1024
FULL = 8192   # rows of a full split
N_CHECK = 8   # pairs of a batch the oracle checks


def _assert_instance(rec, inkernel):
    assert (rec[KIND], rec[QT], rec[NWV], rec[PD], rec[INKERNEL]) == (4, 4, 8, 2, inkernel), rec


def _knn(ctx, q, t, k, inkernel, **extra):
    with options(ctx, **FORCE, **extra, hamming_expand_inkernel=inkernel):
        idx, dist = mpa.knn_hamming(q, t, k=k, ctx=ctx)
        rec = ctx.last_kernels()
    _assert_instance(rec, inkernel)
    return idx, dist, rec


def _single_pair(ctx, oracle, q, t, k=2, **extra):
    """One pair through the biased instance, the unbiased one and the oracle; one split per tile."""
    new_i, new_d, rec = _knn(ctx, q, t, k, 1, hamming_mfma_blocks_per_cu=1, **extra)
    old_i, old_d, _ = _knn(ctx, q, t, k, 0, hamming_mfma_blocks_per_cu=1, **extra)
    oi, od = oracle.knn_hamming(q, t, k=k)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d), (len(q), len(t))
    assert np.array_equal(new_i, oi) and np.array_equal(new_d, od), (len(q), len(t))
    assert rec[NSPLIT] == (len(t) + 31) // 32, rec
    return new_i, new_d


def _batched(ctx, dq, dt, inkernel, k, **extra):
    with options(ctx, **FORCE, hamming_mfma_blocks_per_cu=1, **extra, hamming_expand_inkernel=inkernel):
        out = match_hamming_device(dq, dt, ratio_test=k == 2, ctx=ctx)
        rec = ctx.last_kernels()
        out = {key: v.cpu().numpy() for key, v in out.items()}
    _assert_instance(rec, inkernel)
    return out, rec


def _one_split(ctx, oracle, dq, dt, hq, ht, k=2, nsplit=1, **extra):
    """A batch through both instances (everything equal) and the oracle on N_CHECK pairs; hq / ht are the host copies."""
    new, rec = _batched(ctx, dq, dt, 1, k, **extra)
    old, _ = _batched(ctx, dq, dt, 0, k, **extra)
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
    rng = np.random.default_rng(20270)
    hq = rng.integers(0, 256, (B, NQ, 32), dtype=np.uint8)
    ht = rng.integers(0, 256, (B, FULL, 32), dtype=np.uint8)
    pat = rng.integers(0, 256, (B, 1, 32), dtype=np.uint8)
    for a in (hq, ht, pat):
        a.setflags(write=False)
    return hq, ht, pat, _dev(ht)


def _same_queries(pat):
    """every query of a pair = the pair's pattern"""
    return np.ascontiguousarray(np.broadcast_to(pat, (len(pat), NQ, 32)))


# ---- distance 0 in every tile: the largest value; ties decided by the row ------------------------------------------------------------------

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


# ---- ragged last tiles, the best match on the last row -------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [1, 31, 33, FULL - 31])
def test_ragged_last_tile_best_on_last_row_one_split(ctx, oracle, nt):
    """(A train set of one row has no second neighbour, and the library refuses k = 2 there: that size runs with k = 1.)"""
    _, ht0, pat, _ = _random_batch()
    hq = _same_queries(pat)
    ht = ht0[:, :nt].copy()
    ht[:, nt - 1] = pat[:, 0]
    new = _one_split(ctx, oracle, _dev(hq), _dev(ht), hq, ht, k=min(2, nt))
    assert (new["idx"][:, :, 0] == nt - 1).all() and (new["dist"][:, :, 0] == 0).all()


@pytest.mark.parametrize("nt", [1, 31, 33, FULL - 31])
def test_ragged_last_tile_best_on_last_row_single_pair(ctx, oracle, nt):
    _, ht0, pat, _ = _random_batch()
    q = np.ascontiguousarray(np.broadcast_to(pat[1], (NQ, 32)))
    t = ht0[1, :nt].copy()
    t[nt - 1] = pat[1, 0]
    idx, dist = _single_pair(ctx, oracle, q, t, k=min(2, nt))
    assert (idx[:, 0] == nt - 1).all() and (dist[:, 0] == 0).all()


# ---- one neighbour, the stamped instance, a padded batch stride ----------------------------------------------------------------------------

N_SMALL = 32 * 9 + 5   # four pairs of tiles, a rolled tail and a ragged tile


def test_one_neighbour_one_split(ctx, oracle):
    hq, ht0, _, dt0 = _random_batch()
    _one_split(ctx, oracle, _dev(hq), dt0[:, :N_SMALL], hq, ht0[:, :N_SMALL], k=1)


def test_one_neighbour_single_pair(ctx, oracle):
    hq, ht0, _, _ = _random_batch()
    _single_pair(ctx, oracle, hq[1], ht0[1, :N_SMALL], k=1)


def test_stamped_instance_one_split(ctx, oracle):
    hq, ht0, _, dt0 = _random_batch()
    dq, dt = _dev(hq), dt0[:, :N_SMALL]
    plain, _ = _batched(ctx, dq, dt, 1, 2)
    stamped = _one_split(ctx, oracle, dq, dt, hq, ht0[:, :N_SMALL], hamming_stamps=1)
    for key in ("idx", "dist", "count"):
        assert np.array_equal(stamped[key], plain[key]), key


def test_stamped_instance_single_pair(ctx, oracle):
    hq, ht0, _, _ = _random_batch()
    _single_pair(ctx, oracle, hq[1], ht0[1, :N_SMALL], hamming_stamps=1)


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


# ---- the benchmark's pair shape ------------------------------------------------------------------------------------------------------------

def test_random_pair_8192_by_8192(ctx, oracle):
    q, t = synth.orb_pair(FULL, FULL, seed=20271)
    new_i, new_d, _ = _knn(ctx, q, t, 2, 1)
    old_i, old_d, _ = _knn(ctx, q, t, 2, 0)
    oi, od = oracle.knn_hamming(q, t, k=2)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d)
    assert np.array_equal(new_i, oi) and np.array_equal(new_d, od)
