"""The block form of the running top-2 in the eight-wave LDS-ring Hamming kernel with the in-kernel train expansion (knn_hamming_mfma.hip,
option hamming_block_top2 = 4): in the tile loop a lane folds only the maxima of aligned groups of four train rows into its running pair,
and the epilogue re-scores the rows of the one group that holds a query's best row from the raw descriptors.  Every case is checked
three ways: (idx, dist) bit for bit against the oracle, bit for bit against the same call with hamming_block_top2 = 0 (the per-candidate
update), and mlpl_debug_last_hamming_top2 must name the block size asked for (0 for the reference call), so that a silent fallback cannot
make a case vacuous.  The instance is forced as in test_gpu_hamming_ring_unrolled.py, and the two forms of that file are used:
`single_pair` (one pair of <= 1024 queries: one split per tile, the partial table and the ticket merge) and `one_split` (2 x CUs pairs
through the batched entry: one split per pair, a workgroup walks through all the tiles; the record's split count is asserted).

The train sets are built so that the second neighbour is what the loop may have dropped: random rows (~128 bits from everything) with
CLUSTERS of two or three rows a few bits apart, and every query is a cluster row with 0, 1 or 2 bits flipped, so that its best and its
second are members of one cluster.  A tile carries these clusters (local rows; h = the lane half that holds a row, (row >> 2) & 1):
    (0, 1), (28, 29, 30)   the same group of four rows -- the rows the loop hides -- the triple with three IDENTICAL rows;
    (2, 10)                the same lane column, different groups: both are block maxima of one lane;
    (3, 7)                 different halves of the tile: the second is the other lane's exact maximum;
    (8, 9 | 4), (17, 18 | 21)   two rows of one group plus a row of the other half with a lower / a higher index: with the query on the
                           first row both others are one bit away -- the hidden second TIES with another block's maximum;
    (5 | 32 + 6)           different tiles;
    (24, 26 | 32 + 25), (32 + 14, 32 + 15 | 12)   the same tie against a row of the SAME lane column in the next / the previous tile.
Which cluster, which of its rows and how many flipped bits a query gets follows from its index (the cluster count is odd, so all lanes and
all four query tiles of a wave meet all clusters); the oracle alone decides what the right answer is."""
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
BLOCKS = (4,)   # the block sizes the library carries beside 0
NQ = 1024
# train rows: 1 ... 9 tiles, full and ragged (nt = 1, 2, 5 mod 32 with a cluster on the last two rows), 2 and 33 rows
TRAIN_SIZES = (2, 32, 33, 64, 96, 98, 129, 160, 197, 256, 288)

TILE_CLUSTERS = ((0, 1), (28, 29, 30), (2, 10), (3, 7), (8, 9, 4), (17, 18, 21), (5, 32 + 6), (24, 26, 32 + 25), (32 + 14, 32 + 15, 12))


def _assert_instance(ctx, block):
    rec = ctx.last_kernels()
    assert (rec[KIND], rec[QT], rec[NWV], rec[PD], rec[INKERNEL]) == (4, 4, 8, 2, 1), rec
    assert ctx.last_hamming_top2() == block, (ctx.last_hamming_top2(), block)
    return rec


def _flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


@functools.lru_cache(maxsize=None)
def clustered_pair(nq, nt, seed, identical_train=False):
    """(q, t): see the module text.  Clusters with a row >= nt are left out; the last two rows always form a cluster."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    clusters = [(nt - 2, nt - 1)] if nt >= 2 else [(0,)]
    used = set(clusters[0])
    for tile in range((nt + 31) // 32):
        for c in TILE_CLUSTERS:
            rows = tuple(32 * tile + r for r in c)
            if max(rows) < nt and not used & set(rows):
                clusters.append(rows)
                used |= set(rows)
    for rows in clusters:
        base = t[rows[0]]
        identical = len(rows) == 3 and rows[2] == rows[0] + 2   # (28, 29, 30)
        for j, r in enumerate(rows):
            t[r] = base if identical or j == 0 else _flip(base, [int(rng.integers(0, 256))])   # (one bit from the first row, two from each other)
    if identical_train:
        t[:] = t[0]
    q = np.empty((nq, 32), np.uint8)
    n = len(clusters)
    for i in range(nq):
        rows = clusters[i % n]
        anchor = rows[(i // n) % len(rows)]
        q[i] = _flip(t[anchor], [int(b) for b in rng.integers(0, 256, (i // (3 * n)) % 3)])
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


def _knn(ctx, q, t, k, block, **extra):
    with options(ctx, **FORCE, **extra, hamming_block_top2=block):
        idx, dist = mpa.knn_hamming(q, t, k=k, ctx=ctx)
        rec = _assert_instance(ctx, block)
    return idx, dist, rec


def _single_pair(ctx, oracle, q, t, block, k=2, **extra):
    new_i, new_d, rec = _knn(ctx, q, t, k, block, **extra)
    old_i, old_d, _ = _knn(ctx, q, t, k, 0, **extra)
    oi, od = oracle.knn_hamming(q, t, k=k)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d), (len(q), len(t))
    assert np.array_equal(new_i, oi) and np.array_equal(new_d, od), (len(q), len(t))
    return rec


def _batched(ctx, dq, dt, block, k=2, **extra):
    with options(ctx, **FORCE, **extra, hamming_block_top2=block):
        out = match_hamming_device(dq, dt, ratio_test=k == 2, ctx=ctx)
        rec = _assert_instance(ctx, block)
    return {name: v.cpu().numpy() for name, v in out.items()}, rec


def _batched_both(ctx, oracle, dq, dt, hq, ht, check_pairs, block, k=2, **extra):
    new, rec = _batched(ctx, dq, dt, block, k=k, **extra)
    old, _ = _batched(ctx, dq, dt, 0, k=k, **extra)
    for name in ("idx", "dist", "count"):
        assert np.array_equal(new[name], old[name]), name
    for b in range(len(hq)):
        c = int(new["count"][b])
        assert np.array_equal(new["matches"][b, :c], old["matches"][b, :c]), b
    for b in check_pairs:
        oi, od = oracle.knn_hamming(hq[b], ht[b], k=k)
        assert np.array_equal(new["idx"][b], oi) and np.array_equal(new["dist"][b], od), b
    return new, rec


DISTINCT = 3   # distinct (q, t) pairs of a full-chip batch; pair b holds pair b % DISTINCT


def _full_chip_batch(nq, nt, pad_rows=8):
    """2 x CUs pairs on the device and on the host; the train sets are slices of a larger tensor (a padded batch stride)."""
    import torch
    dev = torch.device("cuda", 0)
    B = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    pairs = [clustered_pair(nq, nt, 1000 * nt + s) for s in range(DISTINCT)]
    hq = np.stack([pairs[b % DISTINCT][0] for b in range(B)])
    ht = np.stack([pairs[b % DISTINCT][1] for b in range(B)])
    big = torch.full((B, nt + pad_rows, 32), 0x5A, dtype=torch.uint8, device=dev)
    big[:, 3:3 + nt] = torch.from_numpy(ht).to(dev)
    dt = big[:, 3:3 + nt]
    assert dt.stride(0) > nt * 32
    return torch.from_numpy(hq).to(dev), dt, hq, ht


@pytest.mark.parametrize("nt", TRAIN_SIZES)
@pytest.mark.parametrize("block", BLOCKS)
def test_clusters_one_split(ctx, oracle, block, nt):
    """One split per pair: the clusters sit in the first tile, in the tiles of the unrolled pairs, in the odd tile and the rolled tail, in
    the last (full or ragged) tile, and across every tile boundary."""
    dq, dt, hq, ht = _full_chip_batch(NQ, nt)
    _, rec = _batched_both(ctx, oracle, dq, dt, hq, ht, range(DISTINCT), block, hamming_mfma_blocks_per_cu=1)
    assert rec[NSPLIT] == 1, rec


@pytest.mark.parametrize("nt", TRAIN_SIZES)
@pytest.mark.parametrize("block", BLOCKS)
def test_clusters_single_pair(ctx, oracle, block, nt):
    """One tile per split: a cluster across a tile boundary has its best in one split and its second in another, a split of one row has no
    second at all (the key of no candidate), and the ticket merge folds partials that must be exact.  1000 queries: no multiple of 32."""
    q, t = clustered_pair(1000, nt, 77 + nt)
    rec = _single_pair(ctx, oracle, q, t, block, hamming_mfma_blocks_per_cu=1)
    assert rec[NSPLIT] == (nt + 31) // 32, rec


@pytest.mark.parametrize("block", BLOCKS)
def test_several_splits_of_several_tiles(ctx, oracle, block):
    """64 pairs against 1093 rows (35 tiles, the last one of five rows): the launcher cuts a few splits of several tiles, so clusters lie
    inside a split and across split boundaries.  900 queries: no multiple of 128."""
    import torch
    B, nq, nt = 64, 900, 1093
    pairs = [clustered_pair(nq, nt, 4242 + s) for s in range(DISTINCT)]
    hq = np.stack([pairs[b % DISTINCT][0] for b in range(B)])
    ht = np.stack([pairs[b % DISTINCT][1] for b in range(B)])
    dev = torch.device("cuda", 0)
    _, rec = _batched_both(ctx, oracle, torch.from_numpy(hq).to(dev), torch.from_numpy(ht).to(dev), hq, ht, range(DISTINCT), block)
    assert 1 < rec[NSPLIT] < (nt + 31) // 32, rec


@pytest.mark.parametrize("block", BLOCKS)
def test_all_train_rows_identical(ctx, oracle, block):
    """Every candidate ties: the best is row 0, the second row 1 -- always a hidden row of the best's block."""
    q, t = clustered_pair(1000, 197, 5, identical_train=True)
    _single_pair(ctx, oracle, q, t, block)
    dq, dt, hq, ht = _full_chip_batch(NQ, 197)
    import torch
    ht = np.broadcast_to(ht[:, :1], ht.shape).copy()
    _, rec = _batched_both(ctx, oracle, dq, torch.from_numpy(ht).to(dq.device), hq, ht, (0,), block, hamming_mfma_blocks_per_cu=1)
    assert rec[NSPLIT] == 1, rec


@pytest.mark.parametrize("block", BLOCKS)
def test_one_neighbour(ctx, oracle, block):
    """k = 1 needs no second look: the block instance runs (the record says so) and the first neighbour is exact.  A train set of ONE row has
    no second neighbour and the library refuses k = 2 there, so that size runs here."""
    for nt in (1, 197):
        q, t = clustered_pair(1000, nt, 300 + nt)
        _single_pair(ctx, oracle, q, t, block, k=1)
    dq, dt, hq, ht = _full_chip_batch(NQ, 197)
    _, rec = _batched_both(ctx, oracle, dq, dt, hq, ht, (0,), block, k=1, hamming_mfma_blocks_per_cu=1)
    assert rec[NSPLIT] == 1, rec


@pytest.mark.parametrize("block", BLOCKS)
def test_stamped_instance(ctx, oracle, block):
    """hamming_stamps = 1 runs the instance with the per-tile clock trace (the rolled loop throughout): the same outputs."""
    dq, dt, hq, ht = _full_chip_batch(NQ, 288)
    plain, _ = _batched(ctx, dq, dt, 0)
    stamped, rec = _batched(ctx, dq, dt, block, hamming_stamps=1)
    assert rec[NSPLIT] == 1, rec
    for name in ("idx", "dist", "count"):
        assert np.array_equal(stamped[name], plain[name]), name
    for b in range(DISTINCT):
        oi, od = oracle.knn_hamming(hq[b], ht[b])
        assert np.array_equal(stamped["idx"][b], oi) and np.array_equal(stamped["dist"][b], od), b


@pytest.mark.parametrize("block", BLOCKS)
def test_one_pair_8192_by_8192(ctx, oracle, block):
    """The benchmark's pair shape against the oracle on all rows."""
    q, t = synth.orb_pair(8192, 8192, seed=20260102)
    new_i, new_d, _ = _knn(ctx, q, t, 2, block)
    old_i, old_d, _ = _knn(ctx, q, t, 2, 0)
    oi, od = oracle.knn_hamming(q, t)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d)
    assert np.array_equal(new_i, oi) and np.array_equal(new_d, od)


def test_option_values(ctx):
    """0 and the block sizes are accepted, anything else is refused and leaves the option as it was."""
    with options(ctx):
        for v in (0,) + BLOCKS:
            ctx.set_option("hamming_block_top2", v)
            assert ctx.get_option("hamming_block_top2") == v
        for v in (-1, 1, 3, 5, 16):
            with pytest.raises(mpa.MlplError):
                ctx.set_option("hamming_block_top2", v)
            assert ctx.get_option("hamming_block_top2") == BLOCKS[-1]
