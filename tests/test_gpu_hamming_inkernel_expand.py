"""The in-kernel train expansion of the eight-wave LDS-ring Hamming kernel (option hamming_expand_inkernel): every case bit-exact in
(idx, dist) against the oracle AND against the same call with the separate expansion kernel, and every case asserts through field 12 of
mlpl_debug_last_kernels which of the two paths ran (a silent fallback would make a case vacuous).

The throughput instance is forced (hamming_mfma_qt = 4, hamming_mfma_waves = 8).  The launcher cuts a small train set into one split per
tile, so the small shapes mostly exercise the prologue, the ragged tile and the ticket merge; the deep-split cases (eight pairs of 8192
queries) are the ones in which a workgroup walks through several tiles, wraps both rings and ends on a ragged tile."""
import functools

import numpy as np
import pytest

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import synth
from matchinglib_poselib_amd.matching import match_hamming_device
from hamming_cases import check_hamming_cases
from option_guard import options

pytestmark = pytest.mark.gpu

KIND, QT, NWV, PD, NSPLIT, INKERNEL = 2, 3, 5, 6, 10, 12
FORCE = dict(hamming_mfma_qt=4, hamming_mfma_waves=8)


NT = [32, 64, 96, 160, 33, 95, 129, 4097]
NQ = [1, 1024, 1025]


@functools.lru_cache(maxsize=None)
def _pair(nq, nt, nbytes=32):
    q, t = synth.orb_pair(nq, nt, nbytes=nbytes, seed=7000 + 3 * nq + nt + nbytes)
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


@functools.lru_cache(maxsize=None)
def _reference(oracle, nq, nt):
    """The oracle's top-2 of the shape, computed once and shared by the k = 1 and k = 2 cases (k = 1 is its first column)."""
    q, t = _pair(nq, nt)
    oi, od = oracle.knn_hamming(q, t, k=2)
    oi.setflags(write=False)
    od.setflags(write=False)
    return oi, od


def _knn(ctx, q, t, k, inkernel, expect_inkernel, **extra):
    with options(ctx, **FORCE, **extra, hamming_expand_inkernel=inkernel):
        idx, dist = mpa.knn_hamming(q, t, k=k, ctx=ctx)
        rec = ctx.last_kernels()
    assert (rec[KIND], rec[QT], rec[NWV], rec[PD]) == (4, 4, 8, 2), rec
    assert rec[INKERNEL] == expect_inkernel, rec
    return idx, dist, rec


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("nq", NQ)
@pytest.mark.parametrize("nt", NT)
def test_inkernel_expand_shapes(ctx, oracle, nt, nq, k):
    q, t = _pair(nq, nt)
    oi, od = _reference(oracle, nq, nt)
    new_i, new_d, _ = _knn(ctx, q, t, k, 1, 1)
    old_i, old_d, _ = _knn(ctx, q, t, k, 0, 0)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d)
    assert np.array_equal(new_i, oi[:, :k]) and np.array_equal(new_d, od[:, :k])


def test_inkernel_expand_ties_and_extremes(ctx, oracle):
    """Five distinct descriptors (the smaller train index must win everywhere) and all-zero / all-ones rows: a sign or plane mix-up
    between the two operands shows here."""
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    z = np.zeros((70, 32), np.uint8)
    o = np.full((90, 32), 255, np.uint8)
    cases = [(base[rng.integers(0, 5, 500)], base[rng.integers(0, 5, 3000)]), (z, o), (z, z[:40]), (o, np.concatenate([z[:45], o[:3]]))]
    for q, t in cases:
        new_i, new_d, _ = _knn(ctx, q, t, 2, 1, 1)
        old_i, old_d, _ = _knn(ctx, q, t, 2, 0, 0)
        oi, od = oracle.knn_hamming(q, t)
        assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d), (len(q), len(t))
        assert np.array_equal(new_i, oi) and np.array_equal(new_d, od), (len(q), len(t))


def test_inkernel_expand_on_the_shared_case_list(ctx, oracle):
    """The shape / tie / extremes / getMatches list every Hamming instance is checked on, with the option on: descriptors of 17..32 bytes
    (rows of eight words) expand in the kernel, every other width takes the expansion kernel or the VALU path -- the record says which."""
    seen = set()

    def after_call(nq, nt, nbytes):
        rec = ctx.last_kernels()
        eligible = 17 <= nbytes <= 32
        assert rec[INKERNEL] == int(eligible), (nq, nt, nbytes, rec)
        if eligible:
            assert (rec[KIND], rec[QT], rec[NWV]) == (4, 4, 8), rec
        seen.add(eligible)

    with options(ctx, **FORCE, hamming_expand_inkernel=1):
        check_hamming_cases(ctx, oracle, "inkernel", after_call)
    assert seen == {True, False}


@pytest.mark.parametrize("nt", [1000, 2049])
def test_inkernel_expand_deep_splits(ctx, oracle, nt):
    """Eight pairs of 8192 queries fill the chip with few train splits, so a workgroup walks through several tiles: the raw ring (4 slots)
    and the fragment ring wrap, the prefetch runs dry at the end and the last split ends on a ragged tile.  Twice on the same context with
    another train set the second time: ring and ticket state must not leak from one call to the next."""
    import torch
    B, nq = 8, 8192
    dev = torch.device("cuda", 0)
    qs, ts = zip(*[synth.orb_pair(nq, nt, seed=9100 + nt + p) for p in range(2 * B)])
    dq = torch.from_numpy(np.stack(qs[:B])).to(dev)
    sub = np.arange(0, nq, 61)
    for rnd in range(2):
        tset = ts[rnd * B:(rnd + 1) * B]
        dt = torch.from_numpy(np.stack(tset)).to(dev)
        res = []
        for on in (1, 0):
            with options(ctx, **FORCE, hamming_expand_inkernel=on):
                out = match_hamming_device(dq, dt, ctx=ctx)
                rec = ctx.last_kernels()
            assert (rec[KIND], rec[NWV], rec[INKERNEL]) == (4, 8, on), rec
            assert 1 < rec[NSPLIT] and rec[NSPLIT] * 4 * 32 <= nt + 127, rec   # several splits of at least four tiles
            res.append({k: v.cpu().numpy() for k, v in out.items()})
        new, old = res
        assert np.array_equal(new["idx"], old["idx"]) and np.array_equal(new["dist"], old["dist"])
        assert np.array_equal(new["count"], old["count"])
        for b in range(B):
            c = int(new["count"][b])
            assert np.array_equal(new["matches"][b, :c], old["matches"][b, :c])
        for b in (0, B - 1):
            oi, od = oracle.knn_hamming(qs[b][sub], tset[b])
            assert np.array_equal(new["idx"][b][sub], oi) and np.array_equal(new["dist"][b][sub], od), (rnd, b)


def test_inkernel_expand_batched_device_entry_with_padded_batch_stride(ctx, oracle):
    """match_hamming_device on three pairs whose train sets are a slice of a larger tensor (batch stride above nt rows): the copy of a ragged
    last tile is clamped to the pair's own rows, and the last pair ends where the tensor's used part ends."""
    import torch
    B, nq, nt = 3, 1025, 95
    dev = torch.device("cuda", 0)
    qs, ts = zip(*[synth.orb_pair(nq, nt, seed=8800 + p) for p in range(B)])
    dq = torch.from_numpy(np.stack(qs)).to(dev)
    big = torch.full((B, nt + 40, 32), 0xA5, dtype=torch.uint8, device=dev)
    big[:, 8:8 + nt] = torch.from_numpy(np.stack(ts)).to(dev)
    dt = big[:, 8:8 + nt]
    assert dt.stride(0) > nt * 32
    res = []
    for on in (1, 0):
        with options(ctx, **FORCE, hamming_expand_inkernel=on):
            out = match_hamming_device(dq, dt, ctx=ctx)
            rec = ctx.last_kernels()
        assert (rec[KIND], rec[NWV], rec[INKERNEL]) == (4, 8, on), rec
        res.append({k: v.cpu().numpy() for k, v in out.items()})
    new, old = res
    assert np.array_equal(new["count"], old["count"])
    for b in range(B):
        oi, od = oracle.knn_hamming(qs[b], ts[b])
        assert np.array_equal(new["idx"][b], oi) and np.array_equal(new["dist"][b], od), b
        assert np.array_equal(old["idx"][b], oi) and np.array_equal(old["dist"][b], od), b
        c = int(new["count"][b])
        assert np.array_equal(new["matches"][b, :c], old["matches"][b, :c]), b


def test_inkernel_expand_repeated_calls_with_many_splits(ctx, oracle):
    """The same call twice in a row on one context, another train set the second time, one split per tile merged by tickets."""
    nq, nt = 1025, 1000
    q, t1 = _pair(nq, nt)
    _, t2 = synth.orb_pair(nq, nt, seed=4242)
    for t in (t1, t2):
        new_i, new_d, rec = _knn(ctx, q, t, 2, 1, 1, hamming_mfma_blocks_per_cu=64)
        assert rec[NSPLIT] > 1, rec
        oi, od = oracle.knn_hamming(q, t)
        assert np.array_equal(new_i, oi) and np.array_equal(new_d, od)
    old_i, old_d, _ = _knn(ctx, q, t2, 2, 0, 0, hamming_mfma_blocks_per_cu=64)
    assert np.array_equal(new_i, old_i) and np.array_equal(new_d, old_d)


@pytest.mark.parametrize("case", ["bytes64", "train01", "waves4", "prefetch4"])
def test_inkernel_expand_falls_back(ctx, oracle, case):
    """Calls the variant does not cover take the expansion kernel with the option on; the record says so and the pairs are exact."""
    nbytes = 64 if case == "bytes64" else 32
    extra = {"train01": dict(hamming_train01=1), "waves4": dict(hamming_mfma_waves=4), "prefetch4": dict(hamming_mfma_prefetch=4)}.get(case, {})
    q, t = _pair(300, 700, nbytes)
    with options(ctx, **{**FORCE, **extra}, hamming_expand_inkernel=1):
        idx, dist = mpa.knn_hamming(q, t, ctx=ctx)
        rec = ctx.last_kernels()
    assert rec[INKERNEL] == 0, rec
    assert rec[KIND] == (3 if case == "bytes64" else 4), rec
    oi, od = oracle.knn_hamming(q, t)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od)
