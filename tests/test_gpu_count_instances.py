"""Every compiled instance of the count-only inlier kernels against the CPU arithmetic, launched exactly as a RANSAC pass launches them
(mlpl_debug_count_pass: device live count, NaN-padded model list, ids scatter, point splits that add into the caller's table).

Reference: oracle.sampson_err(...) widened to double and compared with thresh^2 -- the pinned CPU restatement of modelest.cpp:69-83.
Every case also asserts the instance code mlpl_debug_last_kernels reports, so that a silent fallback cannot make a case vacuous."""
import numpy as np
import pytest

from matchinglib_poselib_amd import _lib, batch, pose, synth
from option_guard import options

pytestmark = pytest.mark.gpu

LARGE = 24577 + 123   # model bound of a pass that takes the large instances (> 24576 models)
SMALL = 3000          # ... and of one that takes the small ones

# name -> (options, large pass?, instance code, models per workgroup)
INSTANCES = {
    "fp64_512": (dict(ransac_f32_filter=0), True, 2, 128),
    "fp64_small": (dict(ransac_f32_filter=0), False, 3, 32),
    "f32_small_128_256": ({}, False, 4, 32),
    "f32_512_one_model_per_lane": (dict(ransac_count_mpl=1), True, 5, 128),
    "f32_512_mpl2": (dict(ransac_count_defer=0), True, 6, 256),
    "f32_512_mpl2_defer": (dict(ransac_count_threads=512), True, 7, 256),
    "f32_256_defer_wpe5": (dict(ransac_count_wpe=5), True, 8, 128),
    "f32_256_defer_wpe6": (dict(ransac_count_wpe=6), True, 9, 128),
}
N_LIST = [1, 5, 6, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2600, 8193]

_SCENE = {}


def _scene(oracle):
    """8193 correspondences of one scene and a pool of its 5-point models, plus an all-zero and a NaN model."""
    if not _SCENE:
        p1, p2, R, t, mask, th = synth.pose_scene(8193, inlier_frac=0.5, seed=4242)
        samples = oracle.sample_table(3, p1, p2, 16)
        Es = np.concatenate([oracle.run5point(p1[s], p2[s]) for s in samples])[:40].reshape(-1, 9)
        pool = np.concatenate([Es, np.zeros((1, 9)), np.full((1, 9), np.nan)])
        _SCENE.update(p1=p1, p2=p2, th=th, pool=pool)
    return _SCENE


def _errors(oracle, p1, p2, pool):
    return np.stack([oracle.sampson_err(p1, p2, E.reshape(3, 3)).astype(np.float64) for E in pool])


def count_pass(ctx, p1, p2, E, n_bound, t2, splits, ids=None, table=None):
    """mlpl_debug_count_pass; returns (table after the pass, instance code, point splits used)."""
    p1 = np.ascontiguousarray(p1, np.float64)
    p2 = np.ascontiguousarray(p2, np.float64)
    E = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
    n_live = E.shape[0]
    Ebuf = E if n_live else np.zeros((1, 9))
    tab = np.array(table, np.int32, copy=True)
    idb = None if ids is None else np.ascontiguousarray(ids, np.int32)
    _lib.check(ctx.lib.mlpl_debug_count_pass(ctx.handle, p1.ctypes.data, p2.ctypes.data, p1.shape[0], Ebuf.ctypes.data, n_live, n_bound,
                                             None if idb is None else idb.ctypes.data, len(tab), float(t2), int(splits), tab.ctypes.data),
               "mlpl_debug_count_pass")
    rec = ctx.last_kernels()
    return tab, rec[0], rec[1]


def auto_splits(n, n_bound, tiles=2):
    """score_point_splits of a count-only pass"""
    if n_bound <= 24576:
        return max(1, min(32, (n + 255) // 256))
    nt = (n + 511) // 512
    return max(1, min(16, nt)) if tiles == 1 else max(1, min(8, nt // 2))


def check_pass(ctx, p1, p2, pool, want_pool, assign, n_bound, t2, splits, code, rng, scatter):
    """One pass: models pool[assign] against the table, expected counts want_pool[assign]; asserts instance, splits and every slot."""
    n = p1.shape[0]
    n_live = len(assign)
    table_len = n_bound + 64
    init = rng.integers(-1000, 1000, table_len).astype(np.int32)   # sentinels: a slot no id names keeps its value
    ids = rng.permutation(table_len)[:n_live].astype(np.int32) if scatter else None
    got, got_code, got_splits = count_pass(ctx, p1, p2, pool[assign], n_bound, t2, splits, ids, init)
    assert got_code == code, (got_code, code)
    want_splits = auto_splits(n, n_bound) if splits < 0 else splits
    assert got_splits == want_splits
    dest = ids if scatter else np.arange(n_live)
    want = init.copy()
    if want_splits > 1:   # several workgroups per model group ADD to the table
        want[dest] += want_pool[assign]
    else:                 # one (or the block kernel): the count is stored
        want[dest] = want_pool[assign]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (n, n_live, n_bound, t2, splits, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("inst", sorted(INSTANCES) + ["block_per_model"])
def test_count_pass_every_instance_shape_split_and_threshold(ctx, oracle, inst):
    """Point counts around the tiles (256 / 512) and splits, model counts around the models per workgroup (32, 128, 256) with the model
    table bound far above the live count, point splits 1, 2, 3, the maximum, the pass's own and more than there are tiles, thresholds ON a
    float error and one double ulp either side, scatter through ids and identity."""
    S = _scene(oracle)
    if inst == "block_per_model":
        opts, large, code, kpb = {}, True, 1, 128
    else:
        opts, large, code, kpb = INSTANCES[inst]
    n_bound = LARGE if large else SMALL
    rng = np.random.default_rng(sum(map(ord, inst)))
    live_cycle = [1, kpb - 1, kpb, kpb + 1, 2 * kpb + 3, n_bound]
    k = 0
    with options(ctx, **opts):
        for n in N_LIST:
            p1, p2 = S["p1"][:n], S["p2"][:n]
            errs = _errors(oracle, p1, p2, S["pool"])
            fin = errs[0][np.isfinite(errs[0])]
            v = float(np.sort(fin)[len(fin) // 2]) if fin.size else S["th"] ** 2
            t2s = [v, float(np.nextafter(v, 0.0)), float(np.nextafter(v, 1.0)), S["th"] ** 2]
            tile = 512 if large else 256
            ntiles = (n + tile - 1) // tile
            split_list = [0] if inst == "block_per_model" else [1, 2, 3, 16 if large else 32, -1, ntiles + 2]
            for splits in split_list:
                t2 = t2s[k % len(t2s)]
                want_pool = (errs <= t2).sum(axis=1)
                n_live = live_cycle[k % len(live_cycle)]
                assign = rng.integers(0, len(S["pool"]), n_live)
                check_pass(ctx, p1, p2, S["pool"], want_pool, assign, n_bound, t2, splits, code, rng, scatter=(k % 2 == 0))
                k += 1


@pytest.mark.parametrize("scale,escale", [(1.0, 1.0), (800.0, 1.0), (1e-3, 1.0), (1e13, 1.0), (1.0, 1e-45)])
def test_count_pass_every_instance_at_every_scale(ctx, oracle, scale, escale):
    """Pixel, tiny and huge coordinates (1e13: the band is infinite, every evaluation takes the fp64 path / the queue and its
    overflow), models scaled by 1e-45 (denormal), all-zero and NaN models: every instance, one and three point splits."""
    S = _scene(oracle)
    p1, p2 = S["p1"][:2600] * scale, S["p2"][:2600] * scale
    pool = S["pool"] * escale
    errs = _errors(oracle, p1, p2, pool)
    fin = errs[np.isfinite(errs)]
    t2s = [float(np.quantile(fin, f)) for f in (0.2, 0.6)] if fin.size else [1.0]
    t2s = [t for t in t2s if t > 0 and np.isfinite(t)] or [1.0]
    f0 = np.sort(errs[0][np.isfinite(errs[0])])
    if f0.size > 100 and f0[100] > 0:
        t2s.append(float(f0[100]))   # ON a float error value
    rng = np.random.default_rng(int(scale * 7) % 1000 + int(-np.log10(escale)))
    for inst, (opts, large, code, kpb) in sorted(INSTANCES.items()):
        with options(ctx, **opts):
            for splits in (1, 3):
                for t2 in t2s:
                    want_pool = (errs <= t2).sum(axis=1)
                    assign = rng.integers(0, len(pool), kpb + 1)
                    check_pass(ctx, p1, p2, pool, want_pool, assign, LARGE if large else SMALL, t2, splits, code, rng, scatter=True)


def _on_threshold_point(oracle):
    """(p1 row, p2 row, model, t2) with t2 = the float error of that correspondence under that model, widened to double."""
    S = _scene(oracle)
    E = S["pool"][0]
    e = oracle.sampson_err(S["p1"][:64], S["p2"][:64], E.reshape(3, 3)).astype(np.float64)
    i = int(np.nonzero(np.isfinite(e) & (e > 0))[0][0])
    return S["p1"][i], S["p2"][i], E, float(e[i])


@pytest.mark.parametrize("inst", ["f32_512_mpl2_defer", "f32_256_defer_wpe5", "f32_256_defer_wpe6"])
@pytest.mark.parametrize("splits", [1, 3])
def test_deferred_queue_fill_at_its_capacity(ctx, oracle, inst, splits):
    """K copies of one correspondence whose float error equals t2: every evaluation of that model is undecided by the fp32 band and
    goes through the queue.  K is chosen so that one workgroup's share is 2047, 2048 (the capacity) and 2049 (overflow: recount of the
    workgroup's strided tile share) entries; t2 on the error counts all K, one ulp below counts none."""
    a1, a2, E, v = _on_threshold_point(oracle)
    opts, large, code, kpb = INSTANCES[inst]
    # one split: the workgroup walks all K; three: workgroup y walks tiles y, y + 3, ... -> 6143 / 6144 / 6145 points put 2047 / 2048 /
    # 2049 of them into workgroup 2 / 0 / 0
    ks = (2047, 2048, 2049) if splits == 1 else (6143, 6144, 6145)
    rng = np.random.default_rng(splits)
    with options(ctx, **opts):
        for K in ks:
            p1, p2 = np.tile(a1, (K, 1)), np.tile(a2, (K, 1))
            for n_live in (1, kpb):
                for t2, per in ((v, K), (float(np.nextafter(v, 0.0)), 0)):
                    ref = int((oracle.sampson_err(p1[:1], p2[:1], E.reshape(3, 3)).astype(np.float64) <= t2).sum()) * K
                    assert ref == per
                    check_pass(ctx, p1, p2, E.reshape(1, 9), np.array([per]), np.zeros(n_live, np.int64), LARGE, t2, splits, code, rng,
                               scatter=True)


@pytest.mark.parametrize("n", [(1 << 23) - 1, 1 << 23])
def test_queue_index_bound_at_two_to_the_23(ctx, oracle, n):
    """The deferred queue holds 23 bits of correspondence index: n = 2^23 - 1 still takes the deferred instance, 2^23 the inline
    one.  In-band correspondences sit at the last indices (queue entries with the largest index)."""
    S = _scene(oracle)
    a1, a2, E0, v = _on_threshold_point(oracle)
    reps = -(-n // 8192)
    p1 = np.tile(S["p1"][:8192], (reps, 1))[:n].copy()
    p2 = np.tile(S["p2"][:8192], (reps, 1))[:n].copy()
    p1[-64:], p2[-64:] = a1, a2
    models = np.stack([E0, S["pool"][1], S["pool"][2]])
    want = np.array([int((oracle.sampson_err(p1, p2, E.reshape(3, 3)).astype(np.float64) <= v).sum()) for E in models])
    rng = np.random.default_rng(n)
    for threads, code in ((256, 8), (512, 7)):
        with options(ctx, ransac_count_threads=threads):
            check_pass(ctx, p1, p2, models, want, np.arange(3), LARGE, v, -1, code if n < (1 << 23) else 6, rng, scatter=True)


def test_count_models_shape1_reaches_every_large_instance(ctx, oracle):
    """mlpl_count_models(shape = 1) goes through the same selection: ransac_count_wpe = 6 reaches <256, 512, 2, true, 6> (it used to run
    the wpe 5 instance)."""
    S = _scene(oracle)
    p1, p2, pool = S["p1"][:2600], S["p2"][:2600], S["pool"]
    t2 = S["th"] ** 2
    want = ((_errors(oracle, p1, p2, pool)) <= t2).sum(axis=1)
    for inst, (opts, large, code, kpb) in sorted(INSTANCES.items()):
        if not large:
            continue
        with options(ctx, **opts):
            got = pose.count_models(p1, p2, pool.reshape(-1, 3, 3), t2, shape=1, ctx=ctx)
            assert ctx.last_kernels()[:2] == [code, 1], inst
        assert np.array_equal(got, want), inst


# count option combinations for the end-to-end runs: (options, instance of a large RANSAC pass, instance of the pair batch's pass)
COMBOS = {
    "default": ({}, 8, 8),
    "wpe6": (dict(ransac_count_wpe=6), 9, 9),
    "threads512": (dict(ransac_count_threads=512), 7, 7),
    "tiles1": (dict(ransac_count_tiles=1), 8, 8),
    "mpl1": (dict(ransac_count_mpl=1), 5, 5),
    "defer0": (dict(ransac_count_defer=0), 6, 6),
    "f32_filter0": (dict(ransac_f32_filter=0), 2, 8),   # (the pair batch always filters: no batched fp64 kernel)
    "threads512_tiles1_defer0": (dict(ransac_count_threads=512, ransac_count_tiles=1, ransac_count_defer=0), 6, 6),
}


def _batch_inputs():
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    sizes = [5, 6, 9, 16, 40, 100, 333, 1000, 3000, 64] * 4
    stride = max(sizes)
    p1 = np.zeros((40, stride, 2))
    p2 = np.zeros((40, stride, 2))
    for i, n in enumerate(sizes):
        a, b, R, t, mask, th = synth.pose_scene(max(n, 8), inlier_frac=float(rng.choice([0.2, 0.5, 0.7, 0.9])), seed=1200 + i)
        if i == 17:
            b = rng.uniform(-0.4, 0.4, b.shape)
        p1[i, :n], p2[i, :n] = a[:n], b[:n]
    return torch.from_numpy(p1).to(dev), torch.from_numpy(p2).to(dev), sizes, [700 + 3 * i for i in range(40)], th


def test_every_count_combination_gives_the_default_results_end_to_end(ctx):
    """The batched RANSAC entry (the PairSlot form of the counting kernel) on the 5...3000-point mix and one C3-shaped ransac_essential
    (5000 correspondences, 25 % inliers: passes far above 24576 models) under every count option combination: byte-identical to the
    default options, and the instance the combination names."""
    import torch
    d1, d2, sizes, seeds, th = _batch_inputs()
    q1, q2, R, t, mask, th3 = synth.pose_scene(5000, inlier_frac=0.25, seed=3303)
    ref = None
    for name, (opts, code_single, code_batch) in COMBOS.items():
        with options(ctx, **opts):
            masks = torch.zeros(d1.shape[:2], dtype=torch.uint8, device=d1.device)
            got = batch.ransac_pose_batched(ctx, d1, d2, sizes, seeds, th, recover_pose=True, masks_out=masks)
            rec_b = ctx.last_kernels()
            single = pose.ransac_essential(q1, q2, th3, confidence=0.9999, max_iters=20000, refit=False, seed=5, ctx=ctx)
            rec_s = ctx.last_kernels()
        assert rec_b[0] == code_batch, (name, rec_b[:2])
        assert rec_s[0] == code_single, (name, rec_s[:2])
        out = (repr([sorted((k, np.asarray(v).tobytes() if isinstance(v, np.ndarray) else v) for k, v in r.items()) for r in got]),
               masks.cpu().numpy().tobytes(), single["E"].tobytes(), single["mask"].tobytes(), single["iters"], single["n_inliers"])
        if ref is None:
            ref = out
        assert out == ref, name


def test_every_option_round_trips(ctx):
    """mlpl_get_option reads back every value mlpl_set_option accepts, for every name; refused values leave the knob alone."""
    from option_guard import REJECTED, SETTABLE
    with options(ctx):
        for name, values in SETTABLE.items():
            for v in values:
                ctx.set_option(name, v)
                assert ctx.get_option(name) == v, (name, v)
            for bad in REJECTED.get(name, ()):
                with pytest.raises(_lib.MlplError):
                    ctx.set_option(name, bad)
                assert ctx.get_option(name) == values[-1], (name, bad)


def test_a_fresh_context_has_the_defaults_and_the_guard_puts_every_option_back(monkeypatch):
    """No kernel runs: a new context reads the written-down default of every option; a block that sets ALL of them to something else and
    then fails leaves all of them at their defaults; a refused value (a range option, a closed-set option) raises and changes nothing."""
    import matchinglib_poselib_amd as mpa
    from option_guard import DEFAULTS, SETTABLE
    monkeypatch.delenv("MLPL_OPTIONS", raising=False)
    c = mpa.Context(0)
    try:
        assert len(DEFAULTS) == 56 and {name: c.get_option(name) for name in DEFAULTS} == DEFAULTS
        other = {name: next(v for v in SETTABLE[name] if v != DEFAULTS[name]) for name in DEFAULTS}
        with pytest.raises(ZeroDivisionError):
            with options(c, **other):
                assert {name: c.get_option(name) for name in DEFAULTS} == other
                1 / 0
        assert {name: c.get_option(name) for name in DEFAULTS} == DEFAULTS
        for name, bad in (("hamming_mfma_blocks_per_cu", 65), ("hamming_mfma_blocks_per_cu", 0), ("hamming_block_top2", 2)):
            with pytest.raises(_lib.MlplError):
                c.set_option(name, bad)
            assert c.get_option(name) == DEFAULTS[name], (name, bad)
    finally:
        c.close()
