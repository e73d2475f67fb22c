"""The VFC match filter on the MI355X (mlpl_vfc_filter, mlpl_vfc_filter_matches_dev, getMatches(VFCrefine=True), the C++ drop-in) against the
numpy restatement in vfc_oracle.py.

What is compared: the KEPT SET, the return code and the number of control points.  On separable ("clean") scenes they must equal the
oracle's in both of its arithmetics (the reference's float32 and float64).  The scene seed of every size is the first in 0..31 on which the
oracle's two arithmetics themselves agree with every posterior at least 0.2 from the threshold -- the premise "separable" made explicit;
it is a property of the oracle alone (test_oracle_vfc.py explains why the reference's float32 run does not always end that way at small n).
On "graded" scenes the device is held to the float64 oracle inside a band of ten times the oracle's own recorded spread.  Iteration
counts are printed, never asserted: the m x m system is numerically singular and the stopping rule is not a reproducible quantity.
"""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import vfc_oracle as VO
from option_guard import options

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "vfc_facade")
SPREAD = json.load(open(os.path.join(ROOT, "tests", "golden", "vfc_spread.json")))["spread"]
BAND = 10.0 * SPREAD
CLEAN_N = [5, 15, 16, 17, 63, 64, 65, 257, 1025, 2000]
_separable = {}


def separable_scene(n):
    """(scene, float32 oracle, float64 oracle) of the first seed on which the oracle's two arithmetics agree with margins >= 0.2"""
    from matchinglib_poselib_amd import synth

    if n not in _separable:
        for seed in range(32):
            s = synth.vfc_scene("clean", n, seed)
            a, b = VO.vfc(s["x1"], s["x2"], 1, "float32_serial"), VO.vfc(s["x1"], s["x2"], 1, "float64")
            if (a["keep"] == b["keep"]).all() and a["rc"] == b["rc"] and min(a["margin"], b["margin"]) >= 0.2:
                _separable[n] = (s, a, b, seed)
                break
        else:
            raise AssertionError(f"no separable clean scene of {n} matches among seeds 0..31")
    return _separable[n]


def single(ctx, x1, x2, seed=1):
    from matchinglib_poselib_amd import matching

    return matching.vfc_filter_points(x1, x2, seed, ctx)


@pytest.mark.parametrize("n", CLEAN_N)
def test_clean_scenes_equal_both_oracles(ctx, n):
    s, a, b, seed = separable_scene(n)
    g = single(ctx, s["x1"], s["x2"])
    assert seed <= 15, f"the first separable scene of {n} matches is seed {seed}: the usable seeds have moved late"
    print(f"n={n}: {seed} scene seeds skipped before a separable one; kept {g['n_keep']} (oracle {a['n_keep']} / {b['n_keep']}), iterations {g['iterations']} (oracle "
          f"{a['iterations']} / {b['iterations']}), m {g['m']}, max|dP| vs float64 {np.abs(g['P'] - b['P']).max():.2e}, singular {g['singular']}")
    for o in (a, b):
        assert g["rc"] == o["rc"] and g["m"] == o["m"] and g["n_keep"] == o["n_keep"]
        assert (g["keep"] == o["keep"]).all()
    assert not g["refused"]


@pytest.mark.parametrize("n,seed", [(n, seed) for n in (257, 1025) for seed in range(4)])
def test_graded_scenes_within_the_oracles_band(ctx, n, seed):
    from matchinglib_poselib_amd import synth

    s = synth.vfc_scene("graded", n, seed)
    o = VO.vfc(s["x1"], s["x2"], 1, "float64")
    g = single(ctx, s["x1"], s["x2"])
    near = np.abs(o["P"] - 0.75) < BAND
    differ = g["keep"] != o["keep"]
    dP = np.abs(g["P"] - o["P"])
    print(f"n={n} seed={seed}: band {BAND:.2e}, {int(near.sum())} matches inside it, {int(differ.sum())} differ, max|dP| outside "
          f"{dP[~near].max():.2e} (inside {dP[near].max() if near.any() else 0:.2e}), iterations {g['iterations']} (oracle {o['iterations']})")
    assert g["rc"] == o["rc"] and g["m"] == o["m"]
    assert not (differ & ~near).any(), "a match differs whose oracle posterior is outside the band"
    assert differ.sum() <= 0.01 * n
    assert dP[~near].max() <= BAND


def test_edge_cases(ctx):
    from matchinglib_poselib_amd import synth
    from test_oracle_vfc import MINUS2, random_scene

    s = synth.vfc_scene("clean", 4, 0)
    g = single(ctx, s["x1"], s["x2"])
    assert g["rc"] == -1 and g["keep"].all() and g["n_keep"] == 4 and g["iterations"] == 0
    g = single(ctx, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    assert g["rc"] == -1 and g["n_keep"] == 0
    rng = np.random.default_rng(3)
    x1 = (np.array([600.0, 300.0]) + rng.random((50, 2)) * 0.1).astype(np.float32)
    x2 = (rng.random((50, 2)) * [1280, 720]).astype(np.float32)
    g = single(ctx, x1, x2)
    assert g["rc"] == 0 and g["refused"] and g["keep"].all() and g["n_keep"] == 50 and g["iterations"] == 0
    s = synth.vfc_scene("clean", 100, 0)
    g = single(ctx, s["x1"], (s["x1"] + np.float32([32.0, -16.0])).astype(np.float32))
    assert g["rc"] == 0 and not g["refused"] and g["keep"].all() and g["iterations"] == 0 and g["m"] == 16
    s = synth.vfc_scene("clean", 8, 0)
    x1, x2 = np.tile(s["x1"], (8, 1)), np.tile(s["x2"], (8, 1))
    g, o = single(ctx, x1, x2), VO.vfc(x1, x2, 1, "float64")
    assert g["m"] == o["m"] <= 8 and g["rc"] == o["rc"]
    for n, seed in MINUS2:
        x1, x2 = random_scene(n, seed)
        g, o = single(ctx, x1, x2), VO.vfc(x1, x2, 1, "float64")
        assert g["rc"] == o["rc"] == -2 and (g["keep"] == o["keep"]).all() and g["n_keep"] == o["n_keep"]


def test_seed_moves_the_control_points_only(ctx):
    """another seed draws other control points; on a separable scene the kept set stays the oracle's for that seed"""
    s, _, _, _ = separable_scene(300)
    for seed in (2, 77, 0xFFFFFFFF):
        g, o = single(ctx, s["x1"], s["x2"], seed), VO.vfc(s["x1"], s["x2"], seed, "float64")
        assert g["m"] == o["m"] and g["rc"] == o["rc"]
        if o["margin"] >= 0.2:
            assert (g["keep"] == o["keep"]).all()


def test_store_u_instance_gives_the_same_bits(ctx):
    from matchinglib_poselib_amd import synth

    s = synth.vfc_scene("graded", 1025, 2)
    res = []
    for v in (0, 1):
        with options(ctx, vfc_store_u=v):
            res.append(single(ctx, s["x1"], s["x2"]))
    assert res[0]["P"].tobytes() == res[1]["P"].tobytes() and res[0]["keep"].tobytes() == res[1]["keep"].tobytes()
    assert res[0]["iterations"] == res[1]["iterations"]


RAGGED = [0, 3, 5, 16, 64, 65, 300, 1025, 4, 15, 17, 63, 257, 1100, 23, 24, 100, 128, 129, 511, 512, 513, 40, 1, 1099, 6, 31, 33, 200, 640, 641, 768, 999]


def _ragged_problem(b, n, stride):
    from matchinglib_poselib_amd import matching, synth
    from test_oracle_vfc import random_scene

    if b % 5 == 4:
        x1, x2 = random_scene(max(n, 1), b)     # mostly rejected lists: status -2, and the replacement rule's other branch
    else:
        s = synth.vfc_scene("graded" if b % 3 == 2 else "clean", max(n, 1), 100 + b)
        x1, x2 = s["x1"], s["x2"]
    rng = np.random.default_rng(b)
    kp1, kp2 = (rng.random((stride, 2)) * 1000).astype(np.float32), (rng.random((stride, 2)) * 1000).astype(np.float32)
    q, t = rng.permutation(stride)[:n], rng.permutation(stride)[:n]
    kp1[q], kp2[t] = x1[:n], x2[:n]
    m = np.zeros(stride, matching.DMATCH_DTYPE)
    m["queryIdx"][:n], m["trainIdx"][:n], m["imgIdx"], m["distance"][:n] = q, t, -1, rng.random(n)
    return kp1, kp2, m, x1[:n], x2[:n]


@pytest.mark.parametrize("rule", [False, True])
def test_ragged_batch_is_byte_identical_to_the_single_entry(ctx, rule):
    import torch
    from matchinglib_poselib_amd import matching

    assert len(RAGGED) == 33
    stride, B = 1100, len(RAGGED)
    probs = [_ragged_problem(b, n, stride) for b, n in enumerate(RAGGED)]
    seeds = np.arange(B, dtype=np.uint32) * 7 + 1
    dev = torch.device("cuda:0")
    d_m = torch.from_numpy(np.stack([p[2] for p in probs]).view(np.int32).reshape(B, stride, 4)).to(dev)
    d_n = torch.tensor(RAGGED, dtype=torch.int32, device=dev)
    d_k1, d_k2 = torch.from_numpy(np.stack([p[0] for p in probs])).to(dev), torch.from_numpy(np.stack([p[1] for p in probs])).to(dev)
    runs = []
    for _ in range(2):
        out = matching.vfc_filter_matches_device(d_m, d_n, d_k1, d_k2, seeds, getmatches_rule=rule, ctx=ctx)
        torch.cuda.synchronize()
        runs.append((out["matches"].cpu().numpy().copy(), out["count"].cpu().numpy().copy(), out["status"].cpu().numpy().copy()))
    statuses = set()
    for b, n in enumerate(RAGGED):
        _, _, m, x1, x2 = probs[b]
        g = single(ctx, x1, x2, int(seeds[b]))
        exp = m[:n][g["keep"]] if (g["rc"] != -1 and (not rule or VO.getmatches_rule(g["rc"], g["n_keep"], n))) else m[:n]
        got, cnt, st = runs[0][0][b], runs[0][1][b], runs[0][2][b]
        assert st == g["rc"] and cnt == len(exp), (b, n, st, g["rc"], cnt, len(exp))
        assert got[:cnt].tobytes() == exp.view(np.int32).reshape(-1, 4).tobytes(), (b, n)
        assert runs[1][0][b][:cnt].tobytes() == got[:cnt].tobytes() and runs[1][1][b] == cnt and runs[1][2][b] == st
        statuses.add(int(st))
    assert statuses == {0, -1, -2}


def _rule_scene(kept, n, seed):
    """`kept` matches of a clean scene's field among n - kept uniform outliers, in list order"""
    from matchinglib_poselib_amd import synth

    s = synth.vfc_scene("clean", 200, 300 + seed)
    idx = np.sort(np.concatenate([np.nonzero(s["inlier"])[0][:kept], np.nonzero(~s["inlier"])[0][:n - kept]]))
    return s["x1"][idx], s["x2"][idx]


def test_replacement_rule_boundary_on_the_device(ctx):
    """matchers.cpp:726-731 inside the kernel: lists of 23 and 24 matches of which the filter keeps exactly 8 and 9 (scene seeds found by a
    search with the float64 oracle alone: it keeps exactly the planted matches, every posterior at least 0.2 from the threshold).  With the
    rule, (24, 8) is the one list that passes through; without it every list is compacted."""
    import torch
    from matchinglib_poselib_amd import matching

    cases = [(24, 8, 2), (24, 9, 2), (23, 8, 2), (23, 9, 2), (30, 8, 4), (30, 9, 2)]
    stride, B = 32, len(cases)
    kp1, kp2 = np.zeros((B, stride, 2), np.float32), np.zeros((B, stride, 2), np.float32)
    m = np.zeros((B, stride), matching.DMATCH_DTYPE)
    exp_keep = []
    for b, (n, k, seed) in enumerate(cases):
        x1, x2 = _rule_scene(k, 24 if n == 23 else n, seed)
        x1, x2 = x1[:n], x2[:n]
        if n == 23:      # drop the last OUTLIER of the 24-match scene, so that the planted matches stay
            o = VO.vfc(*_rule_scene(k, 24, seed), 1, "float64")
            drop = np.nonzero(~o["keep"])[0][-1]
            a1, a2 = _rule_scene(k, 24, seed)
            x1, x2 = np.delete(a1, drop, 0), np.delete(a2, drop, 0)
        o = VO.vfc(x1, x2, 1, "float64")
        assert o["rc"] == 0 and o["n_keep"] == k and o["margin"] >= 0.2, (n, k, o["n_keep"], o["margin"])
        exp_keep.append(o["keep"])
        kp1[b, :n], kp2[b, :n] = x1, x2
        m["queryIdx"][b, :n] = m["trainIdx"][b, :n] = np.arange(n)
        m["distance"][b, :n] = np.arange(n)
    dev = torch.device("cuda:0")
    d_m = torch.from_numpy(m.view(np.int32).reshape(B, stride, 4)).to(dev)
    d_n = torch.tensor([c[0] for c in cases], dtype=torch.int32, device=dev)
    d_k1, d_k2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
    for rule in (False, True):
        out = matching.vfc_filter_matches_device(d_m, d_n, d_k1, d_k2, None, getmatches_rule=rule, ctx=ctx)
        cnt, st, lists = out["count"].cpu().numpy(), out["status"].cpu().numpy(), out["matches"].cpu().numpy()
        for b, (n, k, _) in enumerate(cases):
            through = rule and not (k > 8 or n < 24)
            assert through == (rule and (n, k) in ((24, 8), (30, 8)))
            exp = m[b, :n] if through else m[b, :n][exp_keep[b]]
            assert st[b] == 0 and cnt[b] == len(exp), (rule, n, k, st[b], cnt[b])
            assert lists[b, :cnt[b]].tobytes() == exp.view(np.int32).reshape(-1, 4).tobytes(), (rule, n, k)


def test_largest_list(ctx):
    """65535 matches (the match-list bound): single and batched entry agree; the index arithmetic of the per-point workspace at its largest"""
    import torch
    from matchinglib_poselib_amd import matching, synth

    n = 65535
    s = synth.vfc_scene("clean", n, 1)
    g = single(ctx, s["x1"], s["x2"])
    assert g["rc"] == 0 and g["m"] == 16 and g["n_keep"] == int(g["keep"].sum()) and 1 <= g["iterations"] <= 50
    m = np.zeros((2, n), matching.DMATCH_DTYPE)
    m["queryIdx"] = m["trainIdx"] = np.arange(n)
    dev = torch.device("cuda:0")
    kp1 = torch.from_numpy(np.stack([s["x1"], s["x1"]])).to(dev)
    kp2 = torch.from_numpy(np.stack([s["x2"], s["x2"]])).to(dev)
    out = matching.vfc_filter_matches_device(torch.from_numpy(m.view(np.int32).reshape(2, n, 4)).to(dev), torch.tensor([n, n], dtype=torch.int32, device=dev),
                                             kp1, kp2, None, ctx=ctx)
    cnt, lists = out["count"].cpu().numpy(), out["matches"].cpu().numpy()
    for b in range(2):
        assert cnt[b] == g["n_keep"] and (lists[b, :cnt[b], 0] == np.nonzero(g["keep"])[0]).all()
    print(f"n={n}: kept {g['n_keep']}, {int((g['keep'] != s['inlier']).sum())} differ from the scene's inlier flags, iterations {g['iterations']}")


@pytest.mark.parametrize("kind", ["hamming", "l2"])
def test_composition_match_filter_gather(ctx, kind):
    """mlpl_match_*_dev -> mlpl_vfc_filter_matches_dev -> mlpl_gather_match_points_dev, all on the device, equals the host composition"""
    import torch
    from matchinglib_poselib_amd import matching, synth

    n = 2048
    sp = synth.stereo_pair(n, seed=20261701) if kind == "hamming" else synth.stereo_pair_f32(n, seed=20261702)
    dev = torch.device("cuda:0")
    q, t = torch.from_numpy(sp["desc1"]).to(dev), torch.from_numpy(sp["desc2"]).to(dev)
    mo = (matching.match_hamming_device if kind == "hamming" else matching.match_l2_device)(q, t, ctx=ctx)
    kp1, kp2 = torch.from_numpy(sp["kp1"]).to(dev).unsqueeze(0), torch.from_numpy(sp["kp2"]).to(dev).unsqueeze(0)
    fo = matching.vfc_filter_matches_device(mo["matches"], mo["count"], kp1, kp2, [5], ctx=ctx)
    p1, p2 = torch.zeros((n, 2), dtype=torch.float64, device=dev), torch.zeros((n, 2), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    cnt = int(fo["count"][0])
    K = np.ascontiguousarray(sp["K"], np.float64)
    rc = ctx.lib.mlpl_gather_match_points_dev(ctx.handle, fo["matches"].data_ptr(), cnt, kp1.data_ptr(), kp2.data_ptr(), K.ctypes.data, K.ctypes.data,
                                              p1.data_ptr(), p2.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    # host composition: the matcher's list through the host-pointer filter, then the gather's arithmetic in numpy
    err, hm = matching.getMatches([None] * n, [None] * n, sp["desc1"], sp["desc2"], matcher_name="LINEAR", ctx=ctx)
    assert err == 0 and int(mo["count"][0]) == len(hm)
    assert mo["matches"][0, :len(hm)].cpu().numpy().tobytes() == hm.view(np.int32).reshape(-1, 4).tobytes()
    g = single(ctx, sp["kp1"][hm["queryIdx"]], sp["kp2"][hm["trainIdx"]], 5)
    exp = hm[g["keep"]]
    assert int(fo["status"][0]) == g["rc"] and cnt == len(exp) and 0 < cnt
    assert fo["matches"][0, :cnt].cpu().numpy().tobytes() == exp.view(np.int32).reshape(-1, 4).tobytes()
    e1 = ((sp["kp1"][exp["queryIdx"]].astype(np.float64) - K[2:]) / K[:2]).astype(np.float32).astype(np.float64)
    e2 = ((sp["kp2"][exp["trainIdx"]].astype(np.float64) - K[2:]) / K[:2]).astype(np.float32).astype(np.float64)
    assert p1[:cnt].cpu().numpy().tobytes() == e1.tobytes() and p2[:cnt].cpu().numpy().tobytes() == e2.tobytes()
    print(f"{kind}: {len(hm)} matches, {cnt} kept, status {g['rc']}, iterations {g['iterations']}")


def _matched_clean_pair(n=600, nbytes=32):
    """descriptors whose matches are known (synth.stereo_pair) on keypoints that carry a separable VFC scene"""
    from matchinglib_poselib_amd import synth

    sp = synth.stereo_pair(n, seed=20261703)
    s, _, _, _ = separable_scene(n)
    kp2 = np.empty_like(s["x2"])
    kp2[sp["train_of_query"]] = s["x2"]
    return sp["desc1"], sp["desc2"], s["x1"].copy(), kp2


@pytest.mark.parametrize("matcher", ["LINEAR", "BRUTEFORCENMS"])
def test_python_get_matches_with_vfc(ctx, matcher):
    """getMatches(VFCrefine=True) = the matcher, then the oracle's filter with getMatches' replacement rule"""
    from matchinglib_poselib_amd import matching

    d1, d2, kp1, kp2 = _matched_clean_pair()
    err0, plain = matching.getMatches(kp1, kp2, d1, d2, matcher_name=matcher, ctx=ctx)
    assert err0 == 0 and len(plain) > 100
    for seed in (1, 9):
        err, got = matching.getMatches(kp1, kp2, d1, d2, matcher_name=matcher, VFCrefine=True, vfc_seed=seed, ctx=ctx)
        o = VO.vfc(kp1[plain["queryIdx"]], kp2[plain["trainIdx"]], seed, "float64")
        assert o["margin"] >= 0.2 and o["rc"] == 0
        rc, exp = VO.filter_matches(kp1, kp2, plain, seed, rule=True)
        assert err == 0 and rc == 0 and len(exp) < len(plain)
        assert got.tobytes() == exp.tobytes()
    rc, out = matching.filter_with_vfc(kp1, kp2, plain[:4], ctx=ctx)
    assert rc == -1 and len(out) == 0


def _read_lists(blob):
    out, pos = [], 0
    while pos < len(blob):
        rc, cnt = struct.unpack_from("<ii", blob, pos)
        pos += 8
        out.append((rc, blob[pos:pos + 16 * cnt]))
        pos += 16 * cnt
    return out


def test_cpp_facade_equals_python(ctx, tmp_path):
    from matchinglib_poselib_amd import matching

    assert os.path.exists(FACADE_EXE), "run __graft_entry__.build() first"
    d1, d2, kp1, kp2 = _matched_clean_pair()
    seed = 9
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<iiiI", len(kp1), len(kp2), d1.shape[1], seed))
        f.write(kp1.tobytes() + kp2.tobytes() + d1.tobytes() + d2.tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "matchinglib_poselib_amd", "lib") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([FACADE_EXE, str(fin), str(fout)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout
    lists = _read_lists(open(fout, "rb").read())
    assert len(lists) == 11
    for k, matcher in enumerate(("LINEAR", "BRUTEFORCENMS")):
        plain, filt, direct, again, unseeded = lists[5 * k:5 * k + 5]
        e0, p_plain = matching.getMatches(kp1, kp2, d1, d2, matcher_name=matcher, ctx=ctx)
        e1, p_filt = matching.getMatches(kp1, kp2, d1, d2, matcher_name=matcher, VFCrefine=True, vfc_seed=seed, ctx=ctx)
        e2, p_uns = matching.getMatches(kp1, kp2, d1, d2, matcher_name=matcher, VFCrefine=True, ctx=ctx)
        rc, p_direct = matching.filter_with_vfc(kp1, kp2, p_plain, seed, ctx=ctx)
        assert plain == (e0, p_plain.tobytes()) and filt == (e1, p_filt.tobytes()) and again == filt
        assert direct == (rc, p_direct.tobytes()) and rc == 0 and len(p_direct) < len(p_plain)
        assert unseeded == (e2, p_uns.tobytes())
    assert lists[10] == (-1, b"")
    assert "Too less matches for refinement with VFC!" in r.stdout
