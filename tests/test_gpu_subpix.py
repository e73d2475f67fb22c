"""GPU: sub-pixel refinement (mlpl_subpix_matches, mlpl_subpix_matches_dev, the C++ drop-in matchinglib::getSubPixMatches) against the
restatement tests/subpix_oracle.py.  The difference table is an exact integer and the fit is separately rounded float32, so every comparison
is exact: mask, refined count, status, the info counts, and the keypoints' bits."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import subpix_oracle as O
import subpix_scenes as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "subpix_facade")
BAD_INPUT = -1


def device(ctx, s, sizes=True):
    from matchinglib_poselib_amd import matching

    return matching.subpix_matches(s["img1"], s["img2"], s["kp1"], s["kp2"], s["size1"] if sizes else None, s["size2"] if sizes else None, ctx=ctx)


def same(got, exp, what=""):
    info = [got["dropped_border"], got["dropped_side"], got["dropped_coord"], got["max_side"]]
    print(f"{what}: device refined {got['n_refined']} status {got['status']} info {info}; oracle refined {exp['n_refined']} status {exp['status']} "
          f"info {exp['info']}")
    assert got["inlier"].astype(np.uint8).tobytes() == exp["inlier"].tobytes()
    assert (got["n_refined"], got["status"], info) == (exp["n_refined"], exp["status"], exp["info"])
    assert got["kp2"].tobytes() == exp["kp2"].tobytes()


def check(ctx, s, exp=None, what="", sizes=True):
    exp = exp or S.oracle(s)
    got = device(ctx, s, sizes)
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
    """all keypoints good, 70 % scrambled, all scrambled: both sides of refined < n / 3 and of refined < 2 (tests/test_oracle_subpix.py
    asserts that the set hits all four combinations)"""
    for sc in (0.0, 0.7, 1.0):
        s, exp = S.texture(n, n % 5, sc)
        got, _ = check(ctx, s, exp, f"n {n} scramble {sc}")
        assert got["status"] == (-1 if (got["n_refined"] < n // 3 or got["n_refined"] < 2) else 0)
        assert s["kp1"].tobytes() == S.texture(n, n % 5, sc)[0]["kp1"].tobytes()


def test_shifted_texture_and_noise(ctx):
    for noise in (0.0, 4.0):
        s, exp = S.texture(400, 0, noise=noise)
        got, _ = check(ctx, s, exp, f"noise {noise}")
        assert got["status"] == 0 and got["n_refined"] > 350


# ---- 2. sides

def _centre_scene(sizes1, sizes2, seed=3):
    """keypoints near the centre of the 320 x 240 texture, where a 255-pixel template stays inside the border"""
    s, _ = S.texture(16, seed)
    n = len(sizes1)
    rng = np.random.default_rng(5)
    kp1 = np.array([160.0, 118.0]) + rng.uniform(-6, 6, (n, 2))
    kp2 = kp1 + np.array([3.3, -2.6]) + rng.uniform(-1.5, 1.5, (n, 2))
    return S.with_points(s, kp1, kp2, sizes1, sizes2)


def test_template_sides(ctx):
    from matchinglib_poselib_amd import matching

    nan = float("nan")
    s1 = [0, 11.9, 12, 13, 14, 31, 111.1, 249, 250, 251, nan, -5, 40, 3, nan, 20, 1e30]
    s2 = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 40, 20, nan, 0]
    sides = [17, 17, 17, 19, 19, 37, 117, 255, 255, 0, 17, 17, 45, 45, 25, 17, 0]
    assert O.template_sides(s1, s2).tolist() == sides
    assert [matching.subpix_template_side(a, b, ctx=ctx) for a, b in zip(s1, s2)] == sides
    s = _centre_scene(s1, s2)
    got, exp = check(ctx, s, what="sides")
    assert exp["info"] == [0, 2, 0, 255] and got["n_refined"] == len(s1) - 2
    # each side on its own: the largest side of a call sizes its LDS, nothing else
    for i in (0, 3, 5, 6, 7, 9, 10):
        one = S.with_points(s, s["kp1"][i:i + 1], s["kp2"][i:i + 1], s["size1"][i:i + 1], s["size2"][i:i + 1])
        g, _ = check(ctx, one, what=f"side {sides[i]}")
        assert g["kp2"].tobytes() == got["kp2"][i:i + 1].tobytes() and g["max_side"] == sides[i]


def test_null_size_arrays(ctx):
    s, exp = S.texture(65, 0)
    got, _ = check(ctx, s, exp, "NULL sizes", sizes=False)
    assert got["max_side"] == 17
    t = S.with_points(s, s["kp1"], s["kp2"], np.full(65, 31.0), None)
    exp = S.oracle(t)
    from matchinglib_poselib_amd import matching

    same(matching.subpix_matches(t["img1"], t["img2"], t["kp1"], t["kp2"], t["size1"], None, ctx=ctx), exp, "size2 NULL")
    same(matching.subpix_matches(t["img1"], t["img2"], t["kp1"], t["kp2"], None, t["size1"], ctx=ctx), exp, "size1 NULL")
    assert exp["info"][3] == 37


# ---- 3. rounding of the coordinates, borders, drops

def test_half_coordinates_round_to_even(ctx):
    s, _ = S.texture(16, 2)
    base = np.array([[60.0, 50.0], [61.0, 51.0], [100.0, 121.0], [201.0, 90.0]])
    kp1 = np.concatenate([base + 0.5, base + np.array([0.5, 0.0]), base - 0.5])
    kp2 = kp1 + np.array([3.5, -2.5])
    t = S.with_points(s, kp1, kp2)
    got, exp = check(ctx, t, what="halves")
    assert got["n_refined"] >= 10
    assert O.cv_round(kp1[:4, 0]).tolist() == [60, 62, 100, 202]


def test_borders_and_drops(ctx):
    s, _ = S.texture(16, 1)
    W, H = S.W, S.H
    inf, nan = float("inf"), float("nan")
    pts = [
        ((0.0, 0.0), (0.0, 0.0), 0),                       # corner keypoints: rectangles partly outside, read as 0
        ((W - 1.0, H - 1.0), (W - 1.0, H - 1.0), 0),
        ((3.0, 100.0), (6.3, 97.4), 0),
        ((150.0, 236.0), (153.3, 233.4), 31),
        ((-91.0, 100.0), (100.0, 100.0), 0),               # template origin -99: inside the border
        ((-93.0, 100.0), (100.0, 100.0), 0),               # -101: dropped
        ((100.0, 100.0), (W + 86.0, 100.0), 0),            # window end W + 100: inside
        ((100.0, 100.0), (W + 87.0, 100.0), 0),            # W + 101: dropped
        ((10.0, 10.0), (14.0, 8.0), 249),                  # a 255 template near the corner leaves the border
        ((160.0, 118.0), (163.0, 115.0), 249),             # and fits in the middle
        ((nan, 100.0), (100.0, 100.0), 0),
        ((100.0, 100.0), (100.0, inf), 0),
        ((100.0, 100.0), (-inf, 100.0), 0),
        ((100.0, 3e9), (100.0, 100.0), 0),
        ((100.0, 100.0), (-2147483648.0, 100.0), 0),       # fits an int: the border rule drops it
        ((2147483648.0, 100.0), (100.0, 100.0), 0),        # does not fit
        ((nan, 100.0), (100.0, 100.0), 300),               # coordinate rule before the side rule
        ((10.0, 10.0), (14.0, 8.0), 300),                  # side rule before the border rule
    ]
    t = S.with_points(s, [p[0] for p in pts], [p[1] for p in pts], [p[2] for p in pts], [0.0] * len(pts))
    got, exp = check(ctx, t, what="borders")
    assert exp["info"] == [4, 1, 6, 255]
    dropped = np.array([0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1], bool)
    assert not got["inlier"][dropped].any() and got["kp2"][dropped].tobytes() == t["kp2"][dropped].tobytes()
    assert got["inlier"][[2, 3, 9]].all()


def test_constant_images(ctx):
    s, exp = S.constant()
    got, _ = check(ctx, s, exp, "constant")
    assert not got["inlier"].any() and got["status"] == -1 and got["n_refined"] == 0 and got["kp2"].tobytes() == s["kp2"].tobytes()


@pytest.mark.parametrize("seed", S.ROUNDING_SEEDS)
def test_float_rounding_scenes(ctx, seed):
    s, exp = S.rounding(seed)
    got, _ = check(ctx, s, exp, f"rounding seed {seed}")
    assert got["inlier"].all() and got["max_side"] == 117


def test_row_step_and_unequal_images(ctx):
    s, exp = S.texture(65, 3)
    wide1 = np.full((S.H, S.W + 13), 201, np.uint8)
    wide2 = np.full((S.H + 2, S.W + 64), 77, np.uint8)
    wide1[:, :S.W], wide2[:S.H, :S.W] = s["img1"], s["img2"]
    t = dict(s, img1=wide1[:, :S.W], img2=wide2[:S.H, :S.W])
    assert not t["img1"].flags["C_CONTIGUOUS"] and t["img1"].strides[0] == S.W + 13
    check(ctx, t, exp, "row step")
    small = dict(s, img2=np.ascontiguousarray(s["img2"][:200, :290]))       # keypoints beyond its edge read 0 or are dropped
    got, e2 = check(ctx, small, what="unequal sizes")
    assert e2["inlier"].tobytes() != exp["inlier"].tobytes() or e2["kp2"].tobytes() != exp["kp2"].tobytes()


def test_largest_list_and_one_more(ctx):
    """65535 matches at side 17: 257 distinct keypoint pairs repeated (the oracle's per-match results repeat with them)"""
    from matchinglib_poselib_amd import matching

    s, base = S.texture(257, 2, 0.7)
    n = 65535
    idx = np.arange(n) % 257
    t = S.with_points(s, s["kp1"][idx], s["kp2"][idx])
    refined = int(base["inlier"][idx].sum())
    exp = dict(inlier=base["inlier"][idx], kp2=base["kp2"][idx], n_refined=refined, status=-1 if refined < n // 3 else 0, info=[0, 0, 0, 17])
    got, _ = check(ctx, t, exp, "65535")
    big = S.with_points(s, s["kp1"][np.arange(n + 1) % 257], s["kp2"][np.arange(n + 1) % 257])
    bad_input(lambda: device(ctx, big))
    bad_input(lambda: matching.subpix_matches(s["img1"].astype(np.float32), s["img2"], s["kp1"], s["kp2"], ctx=ctx))
    bad_input(lambda: matching.subpix_matches(np.stack([s["img1"]] * 3, axis=2), s["img2"], s["kp1"], s["kp2"], ctx=ctx))
    bad_input(lambda: matching.subpix_matches(s["img1"], s["img2"], s["kp1"][:5], s["kp2"][:6], ctx=ctx))


# ---- 4. the batched device entry

def _batch_problem(B, stride, nq, nt, seed):
    """B lists of different lengths (one empty, one full) on three image pairs, train indices drawn with repetition, a few indices outside
    the keypoint arrays"""
    rng = np.random.default_rng(seed)
    scenes = [S.texture(nq, 10 + k, 0.3)[0] for k in range(min(B, 3))]
    counts = rng.integers(0, stride + 1, B)
    counts[0] = stride
    if B > 1:
        counts[1] = 0
    if B > 2:
        counts[2] = 4
    if B > 3:
        counts[3] = stride
    img1 = np.stack([scenes[b % 3 if B >= 3 else 0]["img1"] for b in range(B)])
    img2 = np.stack([scenes[b % 3 if B >= 3 else 0]["img2"] for b in range(B)])
    kp1 = np.stack([scenes[b % 3 if B >= 3 else 0]["kp1"] for b in range(B)])
    kp2q = np.stack([scenes[b % 3 if B >= 3 else 0]["kp2"] for b in range(B)])     # kp2q[b][i] matches kp1[b][i]
    m = np.zeros((B, stride), O.DMATCH)
    kp2 = np.zeros((B, nt, 2), np.float32)
    for b in range(B):
        perm = rng.permutation(nq)[:nt]                  # train keypoint j is the partner of query perm[j]
        kp2[b] = kp2q[b][perm]
        if b == 3:
            kp2[b] += np.float32(7.0)                    # every true position outside its window: a list that fails as a whole
        tr = rng.integers(0, nt, stride)                 # with repetition: several matches name one train keypoint
        m[b]["trainIdx"] = tr
        m[b]["queryIdx"] = perm[tr]
        wrong = rng.random(stride) < 0.25                # a quarter of the matches joins the wrong query: mostly outliers
        m[b]["queryIdx"][wrong] = rng.integers(0, nq, int(wrong.sum()))
        m[b]["queryIdx"][stride // 2] = nq + 5           # clamped
        m[b]["trainIdx"][stride // 3] = -2
        m[b]["distance"] = rng.integers(0, 64, stride)
    size1 = np.where(rng.random((B, nq)) < 0.2, 13.0, 0.0).astype(np.float32)
    size2 = np.where(rng.random((B, nt)) < 0.2, 16.0, 0.0).astype(np.float32)
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
    statuses, failed_lists = set(), 0
    for rule in (False, True):
        out = matching.subpix_matches_device(d["m"], d["n"], d["kp1"], d["kp2"], d["img1"], d["img2"], d["size1"], d["size2"], correspondences_rule=rule,
                                             ctx=ctx)
        hint = matching.subpix_matches_device(d["m"], d["n"], d["kp1"], d["kp2"], d["img1"], d["img2"], d["size1"], d["size2"], max_side=21,
                                              correspondences_rule=rule, ctx=ctx)
        torch.cuda.synchronize()
        for k in ("matches", "count", "status", "kp2", "inlier"):
            if k == "matches":
                continue
            assert out[k].cpu().numpy().tobytes() == hint[k].cpu().numpy().tobytes(), k     # the sides here are 17, 19 and 21: max_side = 21 drops none
        om, oc, os_, ok, oi = (out[k].cpu().numpy() for k in ("matches", "count", "status", "kp2", "inlier"))
        hm = hint["matches"].cpu().numpy()
        for b in range(B):
            n = int(p["counts"][b])
            ml = p["m"][b, :n]
            exp = O.compose(p["img1"][b], p["img2"][b], ml, p["kp1"][b], p["kp2"][b], p["size1"][b], p["size2"][b], rule=rule)
            statuses.add(exp["status"])
            failed_lists += 1 if (n > 0 and exp["status"] != 0) else 0
            assert os_[b] == exp["status"] and oc[b] == len(exp["matches"]), (b, n)
            assert om[b, :oc[b]].tobytes() == exp["matches"].tobytes() == hm[b, :oc[b]].tobytes(), (b, n)
            assert ok[b].tobytes() == exp["kp2_out"].tobytes(), (b, n)
            assert oi[b, :n].tobytes() == exp["inlier"].tobytes(), (b, n)
            if b < 4:   # the single entry on the gathered keypoints: the same per-match results
                q, t = np.clip(ml["queryIdx"], 0, nq - 1), np.clip(ml["trainIdx"], 0, nt - 1)
                g = matching.subpix_matches(p["img1"][b], p["img2"][b], p["kp1"][b][q], p["kp2"][b][t], p["size1"][b][q], p["size2"][b][t], ctx=ctx)
                assert g["inlier"].astype(np.uint8).tobytes() == oi[b, :n].tobytes() and g["status"] == os_[b]
                if not (rule and g["status"] != 0):
                    last = {int(tt): i for i, tt in enumerate(t)}
                    for tt, i in last.items():
                        assert ok[b, tt].tobytes() == g["kp2"][i].tobytes()
        print(f"B {B} rule {rule}: counts {p['counts'].tolist()[:8]} -> {oc.tolist()[:8]}, status {os_.tolist()[:8]}")
    assert statuses == {0, -1} or B == 1
    assert failed_lists >= 2 or B < 64       # the pass-through of a list that is not empty, with the rule and without


def test_batch_bad_arguments(ctx):
    import torch
    from matchinglib_poselib_amd import matching

    p = _batch_problem(1, 8, 48, 30, 1)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    m, n = up(p["m"].view(np.int32).reshape(1, 8, 4)), up(p["counts"])
    out = matching.subpix_matches_device(m, n, up(p["kp1"]), up(p["kp2"]), up(p["img1"]), up(p["img2"]), ctx=ctx)
    bad_input(lambda: matching.subpix_matches_device(m, n, up(p["kp1"]), up(p["kp2"]), up(p["img1"]), up(p["img2"]), max_side=256, ctx=ctx))
    bad_input(lambda: matching.subpix_matches_device(m, n, up(p["kp1"]), up(p["kp2"]), up(p["img1"]), up(p["img2"]), ctx=ctx,
                                                     out=dict(out, matches=m)))


def test_chain_match_subpix_gather(ctx):
    """match_hamming_device -> subpix_matches_device -> mlpl_gather_match_points_dev at 256 keypoints: the gathered points are the refined
    keypoints of the emitted matches"""
    import torch
    from matchinglib_poselib_amd import matching, synth
    from matchinglib_poselib_amd._lib import check as rc_check

    nk = 256
    dev = torch.device("cuda:0")
    sp = synth.stereo_pair(nk, seed=20261019)
    tex = synth.subpix_scene("texture", 1, seed=7, width=640, height=480)
    # keypoints 2 of the synthetic pair do not show the texture's shift: put them where it is, so that the refinement has something to find
    kp1 = np.clip(sp["kp1"], 12, [627, 467]).astype(np.float32)
    kp2 = np.empty_like(kp1)
    kp2[sp["train_of_query"]] = kp1 + np.float32([3.0, -3.0])
    mo = matching.match_hamming_device(torch.from_numpy(sp["desc1"]).to(dev), torch.from_numpy(sp["desc2"]).to(dev), ratio_test=False, ctx=ctx)
    d_k1, d_k2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
    d_i1, d_i2 = torch.from_numpy(tex["img1"]).to(dev), torch.from_numpy(tex["img2"]).to(dev)
    out = matching.subpix_matches_device(mo["matches"][0], mo["count"], d_k1, d_k2, d_i1, d_i2, max_side=17, correspondences_rule=True, ctx=ctx)
    torch.cuda.synchronize()
    n_in, n_out = int(mo["count"][0]), int(out["count"][0])
    ml = mo["matches"][0, :n_in].cpu().numpy().view(O.DMATCH).reshape(-1)
    exp = O.compose(tex["img1"], tex["img2"], ml, kp1, kp2, rule=True)
    assert n_in == nk and int(out["status"][0]) == exp["status"] == 0 and n_out == len(exp["matches"]) > nk // 2
    assert out["matches"][0, :n_out].cpu().numpy().tobytes() == exp["matches"].tobytes()
    assert out["kp2"][0].cpu().numpy().tobytes() == exp["kp2_out"].tobytes()
    K = (C.c_double * 4)(800.0, 800.0, 320.0, 240.0)
    p1, p2 = torch.empty((n_out, 2), dtype=torch.float64, device=dev), torch.empty((n_out, 2), dtype=torch.float64, device=dev)
    rc_check(ctx.lib.mlpl_gather_match_points_dev(ctx.handle, out["matches"].data_ptr(), n_out, d_k1.data_ptr(), out["kp2"].data_ptr(), K, K,
                                                  p1.data_ptr(), p2.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "gather")
    torch.cuda.synchronize()
    want = ((exp["kp2_out"][exp["matches"]["trainIdx"]].astype(np.float64) - [320.0, 240.0]) / 800.0).astype(np.float32).astype(np.float64)
    assert p2.cpu().numpy().tobytes() == want.tobytes()


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
    good, e_good = S.texture(65, 0)
    mixed = S.with_points(good, good["kp1"], good["kp2"], np.where(np.arange(65) % 7 == 0, 31.0, 0.0), np.where(np.arange(65) % 5 == 0, 14.0, 0.0))
    e_mixed = S.oracle(mixed)
    bad, e_bad = S.texture(65, 0, 1.0)
    assert e_good["status"] == 0 and e_mixed["status"] == 0 and e_bad["status"] == -1
    for s, exp, pad in ((good, e_good, 0), (mixed, e_mixed, 11), (bad, e_bad, 0)):
        rc, mask, k1, k2, _ = _run_facade(tmp_path, s, 1, step_pad=pad)
        assert rc == exp["status"] and mask.tobytes() == exp["inlier"].tobytes()
        assert k1.tobytes() == s["kp1"].tobytes() and k2.tobytes() == exp["kp2"].tobytes()
    rc, mask, k1, k2, _ = _run_facade(tmp_path, good, 0)                 # inliers == NULL
    assert rc == 0 and mask.tolist() == [1, 0, 1] and k2.tobytes() == e_good["kp2"].tobytes()
    rc, mask, k1, k2, text = _run_facade(tmp_path, good, 1, n2=64)       # unequal sizes: the reference's message, nothing touched
    assert rc == -2 and mask.tolist() == [1, 0, 1] and k2.tobytes() == good["kp2"][:64].tobytes()
    assert "For subpixel-refinement the number of left and right keypoints must be the same as they must match!" in text
