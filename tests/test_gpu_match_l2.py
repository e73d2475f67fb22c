"""mlpl_match_l2_dev -- float knn, ratio test and ordered DMatch emission on the device (the CV_32F half of getMatches "LINEAR",
matchinglib/source/matchers.cpp:632-707) -- against the two-call chain mlpl_knn2_l2sq_f32_dev + mlpl_ratio_compact_f32_dev byte for byte
on every L2 path, with the fused fold (knn_l2_fold_ratio_kernel, option l2_fold_counts) and without it, and against the CPU oracle.

Mutants of knn_l2_fold_ratio_kernel these tests are built to catch: `<=` in the predicate (duplicated train rows: d0 == d1 == 0 must
fail); a last partial count group that counts queries qi >= nq (nq = 1, 63, 65, 255, 257, 1000 on both kernel geometries); an ignored
gate (non-integer data through the auto path's fused kernel with l2_float_mfma = 0); counts per 256 queries instead of 64 (any nq > 64)."""
import os

import numpy as np
import pytest

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import _lib, synth
from matchinglib_poselib_amd.matching import match_l2_device
from option_guard import options

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def _set_l2(ctx, mode):
    _lib.check(ctx.lib.mlpl_set_l2_path(ctx.handle, mode), "set_l2_path")


def _integer_rows(rng, n, dim):
    x = rng.gamma(0.6, 1.0, size=(n, dim))
    x = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-9) * 512.0
    return np.clip(np.rint(x), 0, 255).astype(np.float32)


def _data(B, nq, nt, dim, integer, seed):
    """B pairs: queries near train rows (so the ratio test passes about half of them), duplicated train rows with a query on them
    (d0 == d1 == 0: the predicate must fail, the smaller row comes first)."""
    rng = np.random.default_rng(seed)
    t = np.stack([_integer_rows(rng, nt, dim) for _ in range(B)])
    q = np.stack([_integer_rows(rng, max(nq, 1), dim) for _ in range(B)])[:, :nq]
    for b in range(B):
        if nq:
            near = rng.random(nq) < 0.5
            src = rng.integers(0, nt, nq)
            q[b, near] = np.clip(np.rint(t[b, src[near]] + rng.normal(0, 6.0, (int(near.sum()), dim))), 0, 255)
        t[b, 1] = t[b, 0]
        if nq:
            q[b, nq - 1] = t[b, 0]
    if not integer:   # RootSIFT-like: sqrt(x / sum(x))
        q = np.sqrt(q / np.maximum(q.sum(-1, keepdims=True), 1e-12)).astype(np.float32)
        t = np.sqrt(t / np.maximum(t.sum(-1, keepdims=True), 1e-12)).astype(np.float32)
    return q.astype(np.float32), t.astype(np.float32)


def _padded(x, row_pad, batch_pad):
    """x [B, n, dim] on the device inside a larger block: row stride dim + row_pad, batch stride n * (dim + row_pad) + batch_pad elements;
    the padding is filled with a value that would change every result if a kernel read it."""
    import torch
    B, n, dim = x.shape
    rs, bs = dim + row_pad, n * (dim + row_pad) + batch_pad
    flat = torch.full((B * bs + 8,), 7777.0, dtype=torch.float32, device="cuda")
    view = torch.as_strided(flat, (B, n, dim), (bs, rs, 1))
    view.copy_(torch.from_numpy(x))
    return view, flat


def _match(ctx, dq, dt, ratio_test, ratio=0.75):
    import torch
    out = match_l2_device(dq, dt, ratio_test=ratio_test, ratio=ratio, ctx=ctx)
    torch.cuda.synchronize()
    return out


def _chain(ctx, dq, dt, ratio_test, ratio=0.75):
    """The parent's two calls on the same inputs."""
    import torch
    B, nq, dim = dq.shape
    nt = dt.shape[1]
    k = 2 if ratio_test else 1
    rows = max(nq, 1)     # (an empty tensor has no address)
    out = {"idx": torch.empty((B, rows, k), dtype=torch.int32, device="cuda"), "dist": torch.empty((B, rows, k), dtype=torch.float32, device="cuda"),
           "matches": torch.empty((B, rows, 4), dtype=torch.int32, device="cuda"), "count": torch.full((B,), -1, dtype=torch.int32, device="cuda")}
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(ctx.lib.mlpl_knn2_l2sq_f32_dev(ctx.handle, dq.data_ptr() or dt.data_ptr(), nq, dq.stride(1), dq.stride(0), dt.data_ptr(), nt, dt.stride(1),
                                              dt.stride(0), dim, k, B, out["idx"].data_ptr(), out["dist"].data_ptr(), st), "knn2_l2sq_f32_dev")
    _lib.check(ctx.lib.mlpl_ratio_compact_f32_dev(ctx.handle, out["idx"].data_ptr(), out["dist"].data_ptr(), nq, k, B, ratio, out["matches"].data_ptr(),
                                                  out["count"].data_ptr(), st), "ratio_compact_f32_dev")
    if nq == 0:
        out = {k_: (v[:, :0] if k_ != "count" else v) for k_, v in out.items()}
    torch.cuda.synchronize()
    return out


def _same(a, b, where):
    cnt_a, cnt_b = a["count"].cpu().numpy(), b["count"].cpu().numpy()
    assert np.array_equal(cnt_a, cnt_b), (where, cnt_a, cnt_b)
    assert a["idx"].cpu().numpy().tobytes() == b["idx"].cpu().numpy().tobytes(), where
    assert a["dist"].cpu().numpy().tobytes() == b["dist"].cpu().numpy().tobytes(), where
    ma, mb = a["matches"].cpu().numpy(), b["matches"].cpu().numpy()
    for i, c in enumerate(cnt_a):
        assert ma[i, :c].tobytes() == mb[i, :c].tobytes(), (where, i)
    return cnt_a


# every nq of {1, 63, 64, 65, 255, 257, 1000, 4096}, nt of {2, 3, 500, 4096}, dim of {4, 64, 96, 128, 130} and batch of {1, 3, 64}; nt = 2, 3
# give one train split (the 256-thread fold), nt = 4096 and 500 more than four (the 1024-thread fold); odd rows: padded strides
SHAPES = [(1, 2, 4, 1), (63, 3, 64, 3), (64, 500, 96, 1), (65, 4096, 128, 3), (255, 500, 130, 64), (257, 3, 128, 64), (1000, 4096, 64, 3),
          (4096, 4096, 128, 1), (4096, 500, 96, 3), (1000, 2, 4, 64), (257, 4096, 130, 1), (64, 4096, 128, 64), (1000, 3, 96, 1), (0, 500, 128, 3)]


@pytest.mark.parametrize("case", range(len(SHAPES)))
@pytest.mark.parametrize("integer", [True, False])
def test_match_l2_equals_knn_then_ratio_compact_on_every_path(ctx, case, integer):
    """Byte equality of idx, dist, the DMatch rows and the counts with the two-call chain for mlpl_set_l2_path in {0, 1, 2 (integer data
    only), 3 (dim <= 128 only)} x l2_fold_counts in {0, 1} x ratio_test in {0, 1}; padded row and batch strides on every other shape; auto
    mode on non-integer data with l2_float_mfma = 0 as well, where the fused kernel's gate selects the exact kernel's partial table."""
    nq, nt, dim, B = SHAPES[case]
    q, t = _data(B, nq, nt, dim, integer, 1000 + case)
    pad = case % 2 == 1
    dq, keep_q = _padded(q, 5 if pad else 0, 11 if pad else 0)
    dt, keep_t = _padded(t, 3 if pad else 0, 17 if pad else 0)
    paths = [(0, 1), (1, 1)] + ([(2, 1)] if integer else [(0, 0)] + ([(3, 1)] if dim <= 128 else []))   # (path, l2_float_mfma)
    seen = set()
    try:
        for path, fmfma in paths:
            _set_l2(ctx, path)
            with options(ctx, l2_float_mfma=fmfma):
                for ratio_test in (1, 0):
                    with options(ctx, l2_fold_counts=1):
                        want = _chain(ctx, dq, dt, ratio_test)
                    for fold in (1, 0, 1):
                        with options(ctx, l2_fold_counts=fold):
                            got = _match(ctx, dq, dt, ratio_test)
                            dbg = ctx.last_l2_match()
                            cnt = _same(got, want, (SHAPES[case], integer, path, fmfma, ratio_test, fold))
                            if nq == 0:
                                assert (cnt == 0).all() and dbg == [0, 0, 0, 0]
                                continue
                            seen.add(dbg[0])
                            assert dbg[2] == (1 if fold and dbg[0] != 4 else 0), dbg
                            if path in (1, 2, 3):
                                assert dbg[0] == {1: 1, 2: 2, 3: 4}[path], dbg
                            if ratio_test and nq > 1:    # the query on the duplicated train rows never passes; somebody else does
                                m = got["matches"].cpu().numpy()
                                for b in range(B):
                                    assert nq - 1 not in m[b, :cnt[b], 0], (b, "d0 == d1 passed the ratio test")
                                idx = got["idx"].cpu().numpy()
                                assert (idx[:, nq - 1, 0] == 0).all() and (idx[:, nq - 1, 1] == 1).all()
                            if not ratio_test:
                                assert (cnt == nq).all()
    finally:
        _set_l2(ctx, 0)
    if nq:
        assert seen, "no path ran"


@pytest.mark.parametrize("case", [c for c in range(len(SHAPES)) if SHAPES[c][0] > 0])
def test_fold_kernel_group_counts(ctx, case):
    """The counts knn_l2_fold_ratio_kernel stores, read back directly (ratio_write_kernel never reads the counts of its own last 256
    queries, so the equality tests above cannot see them all): one count per 64 queries and batch item, equal to the number of queries of
    the group with d0 < 0.75f * d1 (all queries of the group for k = 1), the last partial group counting its own queries only.  Exact
    path (many splits or one: both geometries), the int8 path, and the auto path's gate on non-integer data."""
    import torch
    nq, nt, dim, B = SHAPES[case]
    ncnt = (nq + 63) // 64
    try:
        for integer, path in ((True, 1), (True, 2), (True, 0), (False, 0)):
            q, t = _data(B, nq, nt, dim, integer, 2000 + case)
            dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
            idx = torch.empty((B, nq, 2), dtype=torch.int32, device="cuda")
            dist = torch.empty((B, nq, 2), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            _set_l2(ctx, path)
            with options(ctx, l2_float_mfma=0):
                for ratio_test in (1, 0):
                    counts = np.full((B, ncnt), -7, np.int32)
                    n = ctx.lib.mlpl_debug_l2_fold_counts(ctx.handle, dq.data_ptr(), nq, dim, nq * dim, dt.data_ptr(), nt, dim, nt * dim, dim, ratio_test, 0.75, B,
                                                          idx.data_ptr(), dist.data_ptr(), counts.ctypes.data)
                    assert n == B * ncnt, (n, _lib.last_error())
                    k = 2 if ratio_test else 1
                    d = dist.cpu().numpy().reshape(-1)[: B * nq * k].reshape(B, nq, k)
                    ok = (d[:, :, 0] < np.float32(0.75) * d[:, :, 1]) if ratio_test else np.ones((B, nq), bool)
                    want = np.add.reduceat(ok.astype(np.int32), np.arange(0, nq, 64), axis=1)
                    assert np.array_equal(counts, want), (SHAPES[case], integer, path, ratio_test, counts[0][:8], want[0][:8])
                    if ratio_test and nq > 1:
                        assert not ok[:, nq - 1].any()      # d0 == d1 on the duplicated rows: `<`, not `<=`
    finally:
        _set_l2(ctx, 0)


def test_negative_and_bad_arguments_are_refused(ctx):
    import torch
    q, t = _data(1, 8, 4, 16, True, 1)
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    with pytest.raises(RuntimeError):
        match_l2_device(dq, dt[:, :1], ratio_test=True, ctx=ctx)          # nt < k
    big = torch.zeros((1, 4, 1025), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError):
        match_l2_device(big, big, ctx=ctx)                                # dim > 1024
    assert match_l2_device(dq, dt[:, :1], ratio_test=False, ctx=ctx)["count"].cpu().numpy()[0] == 8


@pytest.mark.parametrize("path", [0, 1, 2])
def test_debug_entry_reports_the_fold_and_one_launch_less(ctx, path):
    """mlpl_debug_last_l2_match: with l2_fold_counts on, paths 1, 2 and auto report out[2] == 1 and one launch fewer than with it off."""
    import torch
    q, t = synth.sift_pair(1000, 1500, seed=5)
    dq, dt = torch.from_numpy(q[None]).cuda(), torch.from_numpy(t[None]).cuda()
    try:
        _set_l2(ctx, path)
        with options(ctx, l2_float_mfma=0, l2_fold_counts=0):   # auto mode: the fused kernel whatever kind of data this context saw last (the hint word)
            _match(ctx, dq, dt, 1)
            off = ctx.last_l2_match()
        with options(ctx, l2_float_mfma=0, l2_fold_counts=1):
            _match(ctx, dq, dt, 1)
            on = ctx.last_l2_match()
    finally:
        _set_l2(ctx, 0)
    assert on[0] == off[0] == {0: 3, 1: 1, 2: 2}[path]
    assert on[1] == off[1] >= 1
    assert off[2] == 0 and on[2] == 1
    assert on[3] == off[3] - 1 == {0: 4, 1: 3, 2: 4}[path], (on, off)
    assert ctx.get_option("l2_fold_counts") == 1


def _oracle_equal(oracle, got, b, q, t, where):
    rc, mo = oracle.get_matches_linear(len(q), len(t), q, t)
    cnt = int(got["count"][b].item())
    m = got["matches"][b, :cnt].cpu().numpy()
    assert rc in (0, -3) and cnt == len(mo), (where, cnt, len(mo))
    assert np.array_equal(m[:, 0], mo["queryIdx"]) and np.array_equal(m[:, 1], mo["trainIdx"]) and (m[:, 2] == -1).all(), where
    assert m[:, 3].tobytes() == mo["distance"].tobytes(), where
    return mo


@pytest.mark.parametrize("fold", [1, 0])
def test_matches_equal_the_oracle_bit_for_bit(ctx, oracle, fold):
    """The golden integer SIFT vectors, C4 (4096 x 4096 x 128), a RootSIFT pair, and duplicated train rows: queryIdx ascending, trainIdx,
    imgIdx = -1 and the distance bits of the oracle's cvflann-order loop + ratio loop."""
    import torch
    g = np.load(os.path.join(GOLD, "l2_integer_sift.npz"))
    sets = [("golden128", g["sift128_q"], g["sift128_t"]), ("golden64", g["d64_q"], g["d64_t"])]
    sets.append(("C4",) + synth.sift_pair(4096, 4096, 128, seed=20260104))
    sp = synth.stereo_pair_f32(2048, 20260401, unmatched_frac=0.3, rootsift=True)
    sets.append(("rootsift", sp["desc1"], sp["desc2"]))
    qd, td = synth.sift_pair(600, 900, seed=77)
    td[450:] = td[:450]             # every train row twice: d0 == d1 for every query whose neighbour is exact, the smaller row first
    qd[:100] = td[:100]
    sets.append(("duplicates", qd, td))
    with options(ctx, l2_fold_counts=fold):
        for name, q, t in sets:
            dq, dt = torch.from_numpy(np.ascontiguousarray(q[None])).cuda(), torch.from_numpy(np.ascontiguousarray(t[None])).cuda()
            for rep in range(2):    # (auto mode: the second call on non-integer data takes the fp16 path)
                got = _match(ctx, dq, dt, 1)
                mo = _oracle_equal(oracle, got, 0, q, t, (name, rep))
            if name == "duplicates":
                assert not np.isin(np.arange(100), mo["queryIdx"]).any()
                idx = got["idx"][0].cpu().numpy()
                assert (idx[:100, 0] == np.arange(100)).all() and (idx[:100, 1] == np.arange(100) + 450).all()
            if name == "golden128":
                assert np.array_equal(np.sort(mo["queryIdx"]), np.sort(g["sift128_match_q"]))


def test_batch_of_64_c4_pairs_against_the_oracle_on_four_of_them(ctx, oracle):
    """batch = 64 x (4096 x 4096 x 128) in one call; the oracle runs on pairs 0, 21, 42 and 63."""
    import torch
    B = 64
    pairs = [synth.sift_pair(4096, 4096, 128, seed=20260500 + b) for b in range(B)]
    dq = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    dt = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    got = _match(ctx, dq, dt, 1)
    assert ctx.last_l2_match()[2] == 1
    for b in (0, 21, 42, 63):
        _oracle_equal(oracle, got, b, pairs[b][0], pairs[b][1], b)
    want = _chain(ctx, dq, dt, 1)
    _same(got, want, "batch 64")
