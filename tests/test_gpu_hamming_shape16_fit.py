"""The 16x16x128 throughput instance of the Hamming LDS-ring kernel (knn_hamming_mfma_lds16_kernel) after its vector work was cut down: a lane folds
its eight accumulator registers of a tile -- rows T + 16 h + 4 g + i, ONE block -- into the running pair with a single maximum, the epilogue
re-scores the seven other rows of the best row's block (two rows per lane of the query, clamped to the pair's last row), runs in phases over all
eight groups of a wave, and stores a query's pair from the lane group g with (group & 3) == g, 64 consecutive queries per store round.

Every case is bit-exact in idx, dist, count and matches against the same call with hamming_mfma_shape = 32, and in idx and dist against the oracle;
every call asserts through last_kernels() / last_hamming_shape() / last_hamming_block_rows() that the instance under test ran (8 rows per block in
the 16 shape, 4 in the 32 shape).  Two forms, both through the device entry: `single_pair` (a batch of one: one split per train tile, so the
partials, the ticket and the fold run behind the new stores) and `one_split` (2 x CUs pairs: one split per pair, the outputs leave the registers).

Shapes: 1, 17, 1000 and 1024 queries (ragged groups, the store mapping); 1 ... 100 and 8192 train rows (a clamped re-scan, a block cut by nt in
either row half, a full split); a second neighbour planted at each of the seven other rows of the block and just outside it; distance 0 in every
tile and distance 256; one neighbour; a padded batch stride."""
import functools

import numpy as np
import pytest

from matchinglib_poselib_amd.matching import match_hamming_device
from option_guard import options
from test_gpu_hamming_shape16 import FORCE, FULL, NQ, _assert_instance, _batch_size, _check_pairs, _dev, _random_batch

pytestmark = pytest.mark.gpu

NSPLIT = 10
BLOCK_ROWS = {16: 8, 32: 4}
FORMS = ["single_pair", "one_split"]


def _run(ctx, dq, dt, shape, k):
    with options(ctx, **FORCE, hamming_mfma_blocks_per_cu=1, hamming_mfma_shape=shape):
        out = match_hamming_device(dq, dt, ratio_test=k == 2, ctx=ctx)
        rec = _assert_instance(ctx, shape)
        assert ctx.last_hamming_block_rows() == BLOCK_ROWS[shape], (ctx.last_hamming_block_rows(), shape)
        out = {key: v.cpu().numpy() for key, v in out.items()}
    return out, rec


def _check(ctx, oracle, form, hq, ht, k=2, dq=None, dt=None):
    """hq [B][nq][32], ht [B][nt][32] host arrays (dq / dt: their device forms, if they are views); `form` picks how many pairs run."""
    if form == "single_pair":
        sel = slice(1, 2) if len(hq) > 1 else slice(0, 1)
        hq, ht = hq[sel], ht[sel]
        dq, dt = (None if dq is None else dq[sel]), (None if dt is None else dt[sel])
    dq = _dev(hq) if dq is None else dq
    dt = _dev(ht) if dt is None else dt
    new, rec = _run(ctx, dq, dt, 16, k)
    old, _ = _run(ctx, dq, dt, 32, k)
    nt = ht.shape[1]
    assert rec[NSPLIT] == ((nt + 31) // 32 if form == "single_pair" else 1), rec
    for key in ("idx", "dist", "count"):
        assert np.array_equal(new[key], old[key]), key
    for b in range(len(hq)):
        c = int(new["count"][b])
        assert np.array_equal(new["matches"][b, :c], old["matches"][b, :c]), b
    for b in _check_pairs(len(hq)):
        oi, od = oracle.knn_hamming(hq[b], ht[b], k=k)
        assert np.array_equal(new["idx"][b], oi) and np.array_equal(new["dist"][b], od), b
    return new


def _flip(row, bits):
    row = row.copy()
    for bit in bits:
        row[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return row


@functools.lru_cache(maxsize=None)
def near_batch(nq, nt, seed, n_pat=3):
    """n_pat pairs, repeated over the batch: every train row and every query is one pattern with 0 ... 5 bits flipped, so that a query's best and
    second are close, tie often, and fall into the same block as often as rows allow."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n_pat):
        p = rng.integers(0, 256, 32, dtype=np.uint8)
        t = np.stack([_flip(p, rng.integers(0, 256, int(rng.integers(0, 6)))) for _ in range(nt)])
        q = np.stack([_flip(p, rng.integers(0, 256, int(rng.integers(0, 4)))) for _ in range(nq)])
        pairs.append((q, t))
    B = _batch_size()
    hq = np.stack([pairs[b % n_pat][0] for b in range(B)])
    ht = np.stack([pairs[b % n_pat][1] for b in range(B)])
    hq.setflags(write=False)
    ht.setflags(write=False)
    return hq, ht


# ---- train row counts: a clamped re-scan, a block cut by nt in either row half, a full split ------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nt", [1, 2, 31, 33, 48, 52, 63, 65, 100])
def test_train_rows(ctx, oracle, form, nt):
    """(A train set of one row has no second neighbour, and the library refuses k = 2 there: that size runs with k = 1.)"""
    hq, ht = near_batch(NQ, nt, 1600 + nt)
    _check(ctx, oracle, form, hq, ht, k=min(2, nt))


@pytest.mark.parametrize("form", FORMS)
def test_full_split_near_rows(ctx, oracle, form):
    """8192 rows near one pattern: ties in every tile, the last tile of a full split included."""
    hq, ht = near_batch(NQ, FULL, 1699, n_pat=2)
    _check(ctx, oracle, form, hq, ht)


@pytest.mark.parametrize("form", FORMS)
def test_full_split_random_rows_best_in_last_block(ctx, oracle, form):
    """Random rows; the best is the last row of the split and the second sits in its block's other row half (row FULL - 17)."""
    hq0, ht0, pat, _ = _random_batch()
    hq = np.ascontiguousarray(np.broadcast_to(pat, hq0.shape))
    ht = ht0.copy()
    ht[:, FULL - 1] = pat[:, 0]
    for b in range(len(ht)):
        ht[b, FULL - 17] = _flip(pat[b, 0], [b % 256])
    new = _check(ctx, oracle, form, hq, ht)
    assert (new["idx"] == np.array([FULL - 1, FULL - 17])).all() and (new["dist"] == np.array([0, 1])).all()


# ---- query counts: ragged groups, the store mapping (group & 3) == lane group ---------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nq", [1, 17, 1000])
def test_query_counts(ctx, oracle, form, nq):
    hq, ht = near_batch(nq, 100, 1700 + nq)
    _check(ctx, oracle, form, hq, ht)


def test_every_query_gets_its_own_result(ctx, oracle):
    """Query i is train row i exactly (distance 0) and its second is planted one bit away, so a result stored for the wrong query shows."""
    rng = np.random.default_rng(1616)
    nt = 2 * NQ
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for i in range(NQ):
        t[NQ + i] = _flip(t[i], [i % 256])
    hq, ht = t[None, :NQ], t[None]
    for form in FORMS:
        B = 1 if form == "single_pair" else _batch_size()
        new = _check(ctx, oracle, form, np.repeat(hq, B, 0), np.repeat(ht, B, 0))
        assert (new["idx"][:, :, 0] == np.arange(NQ)).all() and (new["idx"][:, :, 1] == NQ + np.arange(NQ)).all()
        assert (new["dist"] == np.array([0, 1])).all()


# ---- a planted second at each of the seven other rows of the block (+1 ... +3, +16 ... +19 from its first row), and outside it (+4) ----------

N_SMALL = 32 * 9 + 5   # four pairs of tiles, a rolled tail and a ragged tile


@functools.lru_cache(maxsize=None)
def planted_pair(off, seed):
    """Random rows; for every block (tile T, lane group g) whose first row a = T + 4 g and row a + off exist, row a + off is one bit from row a.
    Query i is row a or row a + off of block i mod blocks, alternating with i: its best is that row at distance 0 and its second the other one at
    distance 1 -- for the first kind the LATER row, for the second the earlier one."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (N_SMALL, 32), dtype=np.uint8)
    bases, used = [], set()
    for a in range(0, N_SMALL - off, 4):
        if a % 32 >= 16 or a in used or a + off in used:
            continue
        used |= {a, a + off}
        bases.append(a)
        t[a + off] = _flip(t[a], [int(rng.integers(0, 256))])
    q = np.stack([t[bases[i % len(bases)] + ((i // len(bases)) & 1) * off] for i in range(NQ)])
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("off", [1, 2, 3, 16, 17, 18, 19, 4])
def test_planted_second(ctx, oracle, form, off):
    B = _batch_size()
    pairs = [planted_pair(off, 1800 + 10 * off + s) for s in range(3)]
    hq = np.stack([pairs[b % 3][0] for b in range(B)])
    ht = np.stack([pairs[b % 3][1] for b in range(B)])
    new = _check(ctx, oracle, form, hq, ht)
    assert (new["dist"] == np.array([0, 1])).all() and (np.abs(new["idx"][:, :, 0] - new["idx"][:, :, 1]) == off).all()


# ---- extremes: distance 0 in every tile, distance 256 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nt", [52, FULL])
def test_identical_rows(ctx, oracle, form, nt):
    hq0, _, pat, _ = _random_batch()
    hq = np.ascontiguousarray(np.broadcast_to(pat, hq0.shape))
    ht = np.ascontiguousarray(np.broadcast_to(pat, (len(pat), nt, 32)))
    new = _check(ctx, oracle, form, hq, ht)
    assert (new["idx"] == np.array([0, 1])).all() and (new["dist"] == 0).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nt", [2, 52])
def test_complement_rows(ctx, oracle, form, nt):
    hq0, _, pat, _ = _random_batch()
    hq = np.ascontiguousarray(np.broadcast_to(pat, hq0.shape))
    ht = np.ascontiguousarray(np.broadcast_to(~pat, (len(pat), nt, 32)))
    new = _check(ctx, oracle, form, hq, ht)
    assert (new["idx"] == np.array([0, 1])).all() and (new["dist"] == 256).all()


# ---- one neighbour, a padded batch stride ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_one_neighbour(ctx, oracle, form):
    hq, ht = near_batch(1000, 100, 1900)
    _check(ctx, oracle, form, hq, ht, k=1)


@pytest.mark.parametrize("form", FORMS)
def test_padded_batch_stride(ctx, oracle, form):
    """Query and train rows are slices of larger tensors: rows 8 .. 8 + nt of FULL train rows per pair, the first NQ - 3 queries."""
    hq, ht0, _, dt0 = _random_batch()
    dq = _dev(hq)[:, :NQ - 3]
    dt = dt0[:, 8:8 + N_SMALL]
    assert dt.stride(0) > N_SMALL * 32 and dq.stride(0) > (NQ - 3) * 32
    _check(ctx, oracle, form, hq[:, :NQ - 3], ht0[:, 8:8 + N_SMALL], dq=dq, dt=dt)
