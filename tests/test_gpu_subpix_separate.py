"""GPU: cornerSubPix refinement of each image on its own (mlpl_subpix_separate, mlpl_subpix_separate_dev, the C++ drop-in
matchinglib::getSubPixMatches_seperate_Imgs) against the restatement tests/subpix_separate_oracle.py.  The contract fixes every rounding and
the order of the double sums, so every comparison is byte equality: mask, both keypoint arrays, the passes per point, refined count, status
and info."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import subpix_separate_oracle as O
import subpix_separate_scenes as S
from test_oracle_subpix_separate import edge_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "subpix_separate_facade")
BAD_INPUT = -1


def device(ctx, s):
    from matchinglib_poselib_amd import matching

    return matching.subpix_separate(s["img1"], s["img2"], s["kp1"], s["kp2"], s.get("size1"), s.get("size2"), ctx=ctx)


def same(got, exp, what=""):
    info = [got["w1"], got["w2"], got["dropped_coord"], got["reset_far"]]
    print(f"{what}: device refined {got['n_refined']} status {got['status']} info {info} passes <= {got['iters'].max(initial=0)}; "
          f"oracle refined {exp['n_refined']} status {exp['status']} info {exp['info']} passes <= {exp['iters'].max(initial=0)}")
    assert got["iters"].tobytes() == exp["iters"].tobytes()
    assert got["inlier"].astype(np.uint8).tobytes() == exp["inlier"].tobytes()
    assert (got["n_refined"], got["status"], info) == (exp["n_refined"], exp["status"], exp["info"])
    assert got["kp1"].tobytes() == exp["kp1"].tobytes() and got["kp2"].tobytes() == exp["kp2"].tobytes()


def check(ctx, s, exp=None, what=""):
    exp = exp or S.oracle(s)
    got = device(ctx, s)
    same(got, exp, what)
    return got, exp


def bad_input(fn):
    import matchinglib_poselib_amd as mpa

    with pytest.raises(mpa.MlplError) as e:
        fn()
    assert e.value.code == BAD_INPUT


# ---- 1. list lengths and the status rule

@pytest.mark.parametrize("n", S.N_LIST)
def test_list_lengths_equal_the_oracle(ctx, n):
    """clean, 70 % and all keypoints 2 moved beyond sqrt(12): both sides of refined < n / 3 and of refined < 2
    (tests/test_oracle_subpix_separate.py asserts that the set hits all four combinations)"""
    for sc in S.SCRAMBLES:
        s, exp = S.corners(n, 0, 2.0, sc)
        got, _ = check(ctx, s, exp, f"n {n} scramble {sc}")
        assert got["status"] == (-1 if (got["n_refined"] < n // 3 or got["n_refined"] < 2) else 0)
        if n:
            assert got["iters"].min() >= 2        # nothing here ends in its first pass


# ---- 2. windows

def test_windows_through_the_sizes(ctx):
    from matchinglib_poselib_amd import matching

    nan = float("nan")
    for size, w in ((0.0, 3), (5.9, 3), (6.0, 3), (6.1, 4), (9.5, 5), (10.5, 6), (13.0, 7), (14.1, 8), (16.1, 9), (18.1, 10), (3.4e38, 10), (nan, 10),
                    (-5.0, 3)):
        assert matching.subpix_separate_window(size, ctx=ctx) == O.window(size) == w
    n = 65
    base, _ = S.corners(n, 4)
    cases = [  # sizes of list 1, of list 2, the windows
        (np.zeros(n), np.zeros(n), 10, 10),
        (np.where(np.arange(n) == 40, 6.0, 31.0), np.full(n, 9.5), 3, 5),
        (np.where(np.arange(n) % 9 == 0, 13.0, 0.0), np.where(np.arange(n) == 64, 9.5, 17.0), 7, 5),
        (np.array([nan, -3.0] + [13.0] * (n - 2)), np.array([14.5] * (n - 2) + [-1.0, nan]), 7, 8),
        (np.array([nan, -3.0] + [0.0] * (n - 2)), np.full(n, 16.5), 10, 9),
        (np.full(n, 10.1), np.full(n, 11.9), 6, 6),
        (None, np.full(n, 6.0), 10, 3),           # NULL size arrays
        (np.full(n, 8.0), None, 4, 10),
        (None, None, 10, 10),
    ]
    for s1, s2, w1, w2 in cases:
        s = S.with_points(base, base["kp1"], base["kp2"], s1, s2)
        got, exp = check(ctx, s, what=f"windows {w1}, {w2}")
        assert (got["w1"], got["w2"]) == (w1, w2) and got["n_refined"] > n // 2


def test_both_ends_of_the_summation(ctx):
    """w = 3: 49 terms, lanes 49 .. 63 hold none; w = 10: 441 terms, seven in lanes 0 .. 56 and six in the rest"""
    for size, w in ((6.0, 3), (0.0, 10)):
        s, exp = S.corners(257, 5, 2.0, 0.0, size, size)
        got, _ = check(ctx, s, exp, f"w {w}")
        assert got["w1"] == w and got["status"] == 0


# ---- 3. edges, leaving the image, the "too far" rule, singular systems, drops

@pytest.mark.parametrize("size,w", [(6.0, 3), (9.5, 5), (None, 10)])
def test_points_on_the_edges_and_outside(ctx, size, w):
    """points on and next to every edge, in the corners and outside: the replicated edge, iterations that leave the image (step 3f), that
    run all 40 passes, that the "too far" rule resets"""
    s = edge_scene(size)
    got, exp = check(ctx, s, what=f"edges w {w}")
    assert exp["left"].any() and exp["far"].any() and got["w1"] == w
    assert got["reset_far"] == int(exp["far"].sum()) > 0
    if w == 3:
        assert (got["iters"] == 40).any()


def test_smooth_texture_resets_most_points(ctx):
    s, exp = S.texture()
    got, _ = check(ctx, s, exp, "texture")
    assert got["reset_far"] > 200 and got["iters"].max() == 40


def test_constant_images(ctx):
    s, exp = S.constant()
    got, _ = check(ctx, s, exp, "constant")
    assert (got["iters"] == 0).all() and got["inlier"].all() and got["status"] == 0 and got["n_refined"] == 6
    assert got["kp1"].tobytes() == s["kp1"].tobytes() and got["kp2"].tobytes() == s["kp2"].tobytes()


def test_non_finite_and_out_of_int_coordinates(ctx):
    b1, b2 = S.boards()
    nan, inf = float("nan"), float("inf")
    n = 12
    kp1 = b1["corners"][:n] + np.float32(0.4)
    kp2 = b2["corners"][:n] + np.float32(0.4)
    kp1[1, 0], kp1[3, 1], kp1[6, 0], kp1[7, 1] = nan, 3e9, inf, -3e9
    kp2[3, 0], kp2[4, 1], kp2[5, 0], kp2[8, 0], kp2[9] = -inf, 2147483648.0, -2147483648.0, 2147483520.0, (nan, nan)
    s = S.with_points(dict(img1=b1["img"], img2=b2["img"]), kp1, kp2)
    got, exp = check(ctx, s, what="coordinates")
    assert got["dropped_coord"] == 7 and got["inlier"].tolist() == [1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert (bits(got["kp1"]) == bits(s["kp1"]))[~got["inlier"]].all() and (bits(got["kp2"]) == bits(s["kp2"]))[~got["inlier"]].all()


def test_row_step_and_unequal_images(ctx):
    s, exp = S.corners(65, 3)
    wide1 = np.full((S.H, S.W + 13), 201, np.uint8)
    wide2 = np.full((S.H + 2, S.W + 64), 77, np.uint8)
    wide1[:, :S.W], wide2[:S.H, :S.W] = s["img1"], s["img2"]
    t = dict(s, img1=wide1[:, :S.W], img2=wide2[:S.H, :S.W])
    assert not t["img1"].flags["C_CONTIGUOUS"] and t["img1"].strides[0] == S.W + 13
    check(ctx, t, exp, "row step")
    small = dict(s, img2=np.ascontiguousarray(s["img2"][:200, :250]))       # keypoints beyond its edge read the replicated edge
    got, e2 = check(ctx, small, what="unequal sizes")
    assert e2["kp2"].tobytes() != exp["kp2"].tobytes() and e2["kp1"].tobytes() != exp["kp1"].tobytes()


def test_bad_input(ctx):
    from matchinglib_poselib_amd import matching

    s, _ = S.corners(65, 3)
    n = 65536
    idx = np.arange(n) % 65
    big = S.with_points(s, s["kp1"][idx], s["kp2"][idx])
    bad_input(lambda: device(ctx, big))
    bad_input(lambda: matching.subpix_separate(s["img1"].astype(np.float32), s["img2"], s["kp1"], s["kp2"], ctx=ctx))
    bad_input(lambda: matching.subpix_separate(s["img1"], np.stack([s["img2"]] * 3, axis=2), s["kp1"], s["kp2"], ctx=ctx))
    bad_input(lambda: matching.subpix_separate(s["img1"], s["img2"], s["kp1"][:5], s["kp2"][:6], ctx=ctx))
    # an image smaller than 2 w + 5: w = 5 needs 15 x 15, w = 10 needs 25 x 25
    tiny = np.ascontiguousarray(s["img1"][:14, :40])
    pts = np.float32([[7.0, 7.0], [8.5, 6.0]])
    bad_input(lambda: matching.subpix_separate(tiny, s["img2"], pts, pts, np.float32([9.5, 9.5]), None, ctx=ctx))
    bad_input(lambda: matching.subpix_separate(s["img1"], np.ascontiguousarray(s["img2"][:100, :24]), pts, pts, np.float32([9.5, 9.5]), None, ctx=ctx))
    ok = np.ascontiguousarray(s["img1"][20:35, 20:35])                       # exactly 15 x 15 at w = 5
    t = S.with_points(dict(img1=ok, img2=ok.copy()), pts, pts, [9.5, 9.5], [9.5, 9.5])
    check(ctx, t, what="15 x 15")


# ---- 4. the batched device entry

def _batch_problem(B, stride, nq, nt, seed):
    """B lists of different lengths (one empty, one full) on the two boards and on one of them twice, query and train indices drawn with
    repetition, a few indices outside the keypoint arrays, sizes that give the lists different windows"""
    rng = np.random.default_rng(seed)
    b1, b2 = S.boards()
    counts = rng.integers(0, stride + 1, B)
    counts[0] = stride
    if B > 1:
        counts[1] = 0
    if B > 2:
        counts[2] = stride
    if B > 3:
        counts[3] = 4
    swap = np.arange(B) % 3 == 2
    img1 = np.stack([b2["img"] if swap[b] else b1["img"] for b in range(B)])
    img2 = np.stack([b1["img"] if swap[b] else b2["img"] for b in range(B)])
    kp1 = np.zeros((B, nq, 2), np.float32)
    kp2 = np.zeros((B, nt, 2), np.float32)
    m = np.zeros((B, stride), O.DMATCH)
    size1 = np.zeros((B, nq), np.float32)
    size2 = np.zeros((B, nt), np.float32)
    for b in range(B):
        c1, c2 = (b2 if swap[b] else b1)["corners"], (b1 if swap[b] else b2)["corners"]
        kp1[b] = c1[rng.permutation(len(c1))[:nq]] + rng.uniform(-2, 2, (nq, 2))
        t2 = c2[rng.permutation(len(c2))[:nt]]
        kp2[b] = t2 + rng.uniform(-2, 2, (nt, 2))
        far = rng.random(nt) < (1.0 if b == 2 else 0.25)      # beyond sqrt(12), inside the window: outliers; list 2 fails as a whole
        kp2[b][far] = (t2 + rng.uniform(2.7, 3.3, (nt, 2)) * rng.choice([-1.0, 1.0], (nt, 2)))[far]
        m[b]["trainIdx"] = rng.integers(0, nt, stride)        # with repetition: several matches name one keypoint
        m[b]["queryIdx"] = rng.integers(0, nq, stride)
        m[b]["queryIdx"][stride // 2] = nq + 5                # clamped
        m[b]["trainIdx"][stride // 3] = -2
        m[b]["distance"] = rng.integers(0, 64, stride)
        size1[b] = np.where(rng.random(nq) < 0.3, (0.0, 13.0, 10.1, 9.5)[b % 4], 31.0)
        size2[b] = np.where(rng.random(nt) < 0.3, (9.5, 0.0, 16.5, 9.5)[b % 4], float("nan") if b % 2 else 20.0)
    return dict(img1=img1, img2=img2, kp1=kp1, kp2=kp2, m=m, counts=counts.astype(np.int32), size1=size1, size2=size2)


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_equals_the_oracle_and_the_single_entry(ctx, B):
    import torch
    from matchinglib_poselib_amd import matching

    stride, nq, nt = 40, 48, 30
    p = _batch_problem(B, stride, nq, nt, 100 + B)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(m=up(p["m"].view(np.int32).reshape(B, stride, 4)), n=up(p["counts"]), kp1=up(p["kp1"]), kp2=up(p["kp2"]), img1=up(p["img1"]),
             img2=up(p["img2"]), size1=up(p["size1"]), size2=up(p["size2"]))
    statuses, failed_lists, windows = set(), 0, set()
    for rule in (False, True):
        out = matching.subpix_separate_device(d["m"], d["n"], d["kp1"], d["kp2"], d["img1"], d["img2"], d["size1"], d["size2"],
                                              correspondences_rule=rule, ctx=ctx)
        torch.cuda.synchronize()
        om, oc, os_, ok1, ok2, oi = (out[k].cpu().numpy() for k in ("matches", "count", "status", "kp1", "kp2", "inlier"))
        for b in range(B):
            n = int(p["counts"][b])
            ml = p["m"][b, :n]
            exp = O.compose(p["img1"][b], p["img2"][b], ml, p["kp1"][b], p["kp2"][b], p["size1"][b], p["size2"][b], rule=rule)
            statuses.add(exp["status"])
            windows.add(tuple(exp["single"]["info"][:2]))
            failed_lists += 1 if (n > 0 and exp["status"] != 0) else 0
            assert os_[b] == exp["status"] and oc[b] == len(exp["matches"]), (b, n)
            assert om[b, :oc[b]].tobytes() == exp["matches"].tobytes(), (b, n)
            assert ok1[b].tobytes() == exp["kp1_out"].tobytes() and ok2[b].tobytes() == exp["kp2_out"].tobytes(), (b, n)
            assert oi[b, :n].tobytes() == exp["inlier"].tobytes(), (b, n)
            if rule:
                assert ok1[b].tobytes() == p["kp1"][b].tobytes()
            if b < 4:   # the single entry on the gathered keypoints: the same per-match results
                q, t = np.clip(ml["queryIdx"], 0, nq - 1), np.clip(ml["trainIdx"], 0, nt - 1)
                g = matching.subpix_separate(p["img1"][b], p["img2"][b], p["kp1"][b][q], p["kp2"][b][t], p["size1"][b][q], p["size2"][b][t], ctx=ctx)
                assert g["inlier"].astype(np.uint8).tobytes() == oi[b, :n].tobytes() and g["status"] == os_[b]
                if not (rule and g["status"] != 0):
                    for tt, i in {int(tt): i for i, tt in enumerate(t)}.items():
                        assert ok2[b, tt].tobytes() == g["kp2"][i].tobytes()
                    if not rule:
                        for qq, i in {int(qq): i for i, qq in enumerate(q)}.items():
                            assert ok1[b, qq].tobytes() == g["kp1"][i].tobytes()
        print(f"B {B} rule {rule}: counts {p['counts'].tolist()[:8]} -> {oc.tolist()[:8]}, status {os_.tolist()[:8]}, windows {sorted(windows)}")
    assert statuses == {0, -1} or B == 1
    assert failed_lists >= 2 or B < 3        # the pass-through of a list that is not empty, with the rule and without
    assert len(windows) >= 3 or B < 3


def test_batch_in_place_and_bad_arguments(ctx):
    import torch
    from matchinglib_poselib_amd import matching

    p = _batch_problem(1, 8, 48, 30, 1)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    m, n = up(p["m"].view(np.int32).reshape(1, 8, 4)), up(p["counts"])
    k1, k2, i1, i2 = up(p["kp1"]), up(p["kp2"]), up(p["img1"]), up(p["img2"])
    out = matching.subpix_separate_device(m, n, k1, k2, i1, i2, ctx=ctx)
    torch.cuda.synchronize()
    # d_kp1_out = NULL, and d_kp2_out = d_kp2
    c2 = k2.clone()
    o2 = matching.subpix_separate_device(m, n, k1, c2, i1, i2, ctx=ctx, out=dict(out, kp1=None, kp2=c2, matches=torch.empty_like(m)))
    torch.cuda.synchronize()
    assert o2["kp2"].cpu().numpy().tobytes() == out["kp2"].cpu().numpy().tobytes() != p["kp2"].tobytes()
    bad_input(lambda: matching.subpix_separate_device(m, n, k1, k2, i1, i2, ctx=ctx, out=dict(out, matches=m)))
    bad_input(lambda: matching.subpix_separate_device(m, n, k1, k2, i1[:, :24], i2, ctx=ctx))


def test_chain_match_subpix_gather(ctx):
    """match_hamming_device -> subpix_separate_device -> mlpl_gather_match_points_dev at 256 keypoints: the gathered points are the refined
    keypoints of the emitted matches"""
    import torch
    from matchinglib_poselib_amd import matching, synth
    from matchinglib_poselib_amd._lib import check as rc_check

    nk = 256
    dev = torch.device("cuda:0")
    sp = synth.stereo_pair(nk, seed=20261019)
    b1, b2 = S.boards()
    rng = np.random.default_rng(8)
    kp1 = (b1["corners"][np.arange(nk) % len(b1["corners"])] + rng.uniform(-2, 2, (nk, 2))).astype(np.float32)
    kp2 = np.empty_like(kp1)
    kp2[sp["train_of_query"]] = b2["corners"][np.arange(nk) % len(b2["corners"])] + rng.uniform(-2, 2, (nk, 2))
    mo = matching.match_hamming_device(torch.from_numpy(sp["desc1"]).to(dev), torch.from_numpy(sp["desc2"]).to(dev), ratio_test=False, ctx=ctx)
    d_k1, d_k2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
    d_i1, d_i2 = torch.from_numpy(b1["img"]).to(dev), torch.from_numpy(b2["img"]).to(dev)
    out = matching.subpix_separate_device(mo["matches"][0], mo["count"], d_k1, d_k2, d_i1, d_i2, ctx=ctx)
    torch.cuda.synchronize()
    n_in, n_out = int(mo["count"][0]), int(out["count"][0])
    ml = mo["matches"][0, :n_in].cpu().numpy().view(O.DMATCH).reshape(-1)
    exp = O.compose(b1["img"], b2["img"], ml, kp1, kp2)
    assert n_in == nk and int(out["status"][0]) == exp["status"] == 0 and n_out == len(exp["matches"]) == nk
    assert out["matches"][0, :n_out].cpu().numpy().tobytes() == exp["matches"].tobytes()
    assert out["kp1"][0].cpu().numpy().tobytes() == exp["kp1_out"].tobytes() != kp1.tobytes()
    assert out["kp2"][0].cpu().numpy().tobytes() == exp["kp2_out"].tobytes() != kp2.tobytes()
    K = (C.c_double * 4)(800.0, 800.0, 160.0, 120.0)
    p1, p2 = torch.empty((n_out, 2), dtype=torch.float64, device=dev), torch.empty((n_out, 2), dtype=torch.float64, device=dev)
    rc_check(ctx.lib.mlpl_gather_match_points_dev(ctx.handle, out["matches"].data_ptr(), n_out, out["kp1"].data_ptr(), out["kp2"].data_ptr(), K, K,
                                                  p1.data_ptr(), p2.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "gather")
    torch.cuda.synchronize()
    norm = lambda k: ((k.astype(np.float64) - [160.0, 120.0]) / 800.0).astype(np.float32).astype(np.float64)
    assert p1.cpu().numpy().tobytes() == norm(exp["kp1_out"][exp["matches"]["queryIdx"]]).tobytes()
    assert p2.cpu().numpy().tobytes() == norm(exp["kp2_out"][exp["matches"]["trainIdx"]]).tobytes()


# ---- 5. the C++ drop-in

def _run_facade(tmp_path, s, with_mask, n2=None, step_pad=0):
    assert os.path.exists(FACADE_EXE), "run __graft_entry__.build() first"
    n1 = len(s["kp1"])
    n2 = n1 if n2 is None else n2
    h1, w1 = s["img1"].shape
    h2, w2 = s["img2"].shape
    i1 = np.full((h1, w1 + step_pad), 255, np.uint8)
    i2 = np.full((h2, w2 + step_pad), 255, np.uint8)
    i1[:, :w1], i2[:, :w2] = s["img1"], s["img2"]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<9i", n1, n2, w1, h1, w1 + step_pad, w2, h2, w2 + step_pad, with_mask))
        f.write(i1.tobytes() + i2.tobytes())
        f.write(np.concatenate([s["kp1"], s["size1"][:, None]], axis=1).astype(np.float32).tobytes())
        f.write(np.concatenate([s["kp2"], s["size2"][:, None]], axis=1).astype(np.float32)[:n2].tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "matchinglib_poselib_amd", "lib") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([FACADE_EXE, str(fin), str(fout)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout
    blob = open(fout, "rb").read()
    rc, nm = struct.unpack_from("<2i", blob, 0)
    mask = np.frombuffer(blob, np.uint8, nm, 8)
    k1 = np.frombuffer(blob, np.float32, 2 * n1, 8 + nm).reshape(-1, 2)
    k2 = np.frombuffer(blob, np.float32, 2 * n2, 8 + nm + 8 * n1).reshape(-1, 2)
    return rc, mask, k1, k2, r.stdout


def test_cpp_facade(ctx, tmp_path):
    good, e_good = S.corners(65, 0)
    mixed, e_mixed = S.corners(65, 1, 2.0, 0.4, 13.0, 9.5)
    bad, e_bad = S.corners(65, 0, 2.0, 1.0)
    assert e_good["status"] == 0 and e_mixed["status"] == 0 and 0 < e_mixed["n_refined"] < 65 and e_bad["status"] == -1
    for s, exp, pad in ((good, e_good, 0), (mixed, e_mixed, 11), (bad, e_bad, 0)):
        rc, mask, k1, k2, _ = _run_facade(tmp_path, s, 1, step_pad=pad)
        assert rc == exp["status"] and mask.tobytes() == exp["inlier"].tobytes()
        assert k1.tobytes() == exp["kp1"].tobytes() and k2.tobytes() == exp["kp2"].tobytes()
    rc, mask, k1, k2, _ = _run_facade(tmp_path, good, 0)                 # inliers == NULL
    assert rc == 0 and mask.tolist() == [1, 0, 1] and k1.tobytes() == e_good["kp1"].tobytes() and k2.tobytes() == e_good["kp2"].tobytes()
    rc, mask, k1, k2, text = _run_facade(tmp_path, good, 1, n2=64)       # unequal sizes: the reference's message, nothing touched
    assert rc == -2 and mask.tolist() == [1, 0, 1] and k1.tobytes() == good["kp1"].tobytes() and k2.tobytes() == good["kp2"][:64].tobytes()
    assert "For subpixel-refinement the number of left and right keypoints must be the same as they must match!" in text
