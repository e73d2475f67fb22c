"""GPU: the GMS match filter (mlpl_gms_filter, mlpl_gms_filter_matches_dev, the C++ drop-in filterMatchesGMS) against the restatement
tests/gms_oracle.py.  The filter is integer voting, so every comparison is exact: keep arrays, counts, the winning (scale level, rotation
type) and the compacted lists byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gms_oracle as G
import gms_scenes as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "gms_facade")
BAD_INPUT = -1


def device(ctx, s, use_scale=False, use_rotation=False):
    from matchinglib_poselib_amd import matching

    return matching.gms_filter(s["kp1"], s["size1"], s["kp2"], s["size2"], s["matches"], use_scale, use_rotation, ctx=ctx)


def check(ctx, s, use_scale=False, use_rotation=False, exp=None):
    """the device's result equals the oracle's in every field; returns (device, oracle)"""
    exp = exp or S.oracle(s, use_scale, use_rotation)
    got = device(ctx, s, use_scale, use_rotation)
    print(f"n {len(s['matches'])} scale {use_scale} rotation {use_rotation}: device kept {got['n_keep']} at ({got['scale']}, {got['rotation']}), dropped "
          f"{got['dropped']}; oracle kept {exp['n_keep']} at ({exp['scale']}, {exp['rotation']}), dropped {exp['dropped']}")
    assert got["keep"].tobytes() == exp["keep"].tobytes()
    assert (got["n_keep"], got["scale"], got["rotation"], got["dropped"]) == (exp["n_keep"], exp["scale"], exp["rotation"], exp["dropped"])
    assert got["n_keep"] == int(got["keep"].sum())
    return got, exp


def bad_input(fn):
    import matchinglib_poselib_amd as mpa

    with pytest.raises(mpa.MlplError) as e:
        fn()
    assert e.value.code == BAD_INPUT


# ---- 1. the single entry against the oracle

@pytest.mark.parametrize("n", [0, 1, 4, 63, 64, 65, 255, 256, 257, 1025, 4096])
def test_smooth_scenes_equal_the_oracle(ctx, n):
    from matchinglib_poselib_amd import synth

    got, _ = check(ctx, synth.gms_scene("smooth", n, seed=n % 5))
    assert n < 1025 or got["n_keep"] > n // 2   # the filter finds the field


def test_largest_list_and_one_more(ctx):
    from matchinglib_poselib_amd import synth

    s = synth.gms_scene("smooth", 65535, seed=1)
    got, _ = check(ctx, s)
    assert got["n_keep"] > 40000
    big = synth.gms_scene("smooth", 65536, seed=1)
    bad_input(lambda: device(ctx, big))


# ---- 2. scale and rotation

@pytest.mark.parametrize("use_rotation", [False, True])
@pytest.mark.parametrize("use_scale", [False, True])
@pytest.mark.parametrize("kind", ["rot90", "scale2"])
def test_scale_and_rotation_runs(ctx, kind, use_scale, use_rotation):
    from matchinglib_poselib_amd import synth

    s = synth.gms_scene(kind, 2000, seed=0)
    exp = S.oracle(s, use_scale, use_rotation)
    # the scene exercises the selection: its winning run is not (0, 0) once the switch it was built for is on
    if use_scale and use_rotation:
        assert (exp["scale"], exp["rotation"]) != (0, 0) and exp["n_keep"] > 1000
    if kind == "rot90" and use_rotation:
        assert exp["rotation"] > 0
    if kind == "scale2" and use_scale:
        assert exp["scale"] > 0
    check(ctx, s, use_scale, use_rotation, exp)


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("ratio,level", [(2.0, 1), (2.0 ** 0.5, 2), (0.5 ** 0.5, 3), (0.5, 4)])
def test_every_right_grid_size_wins_somewhere(ctx, ratio, level, rotate):
    """the second image's content scaled by 2, sqrt 2, 1 / sqrt 2 and 1 / 2: the winning run is on the right grid of 10, 14, 28 and 40 cells,
    so the device's mask and count at each of these sizes are the ones compared; turned by 90 degrees, it is at rotation type 6 there"""
    s = S.scaled_scene(ratio, 2000, seed=0, rotate=rotate)
    exp = S.oracle(s, True, True)
    assert exp["scale"] == level and G.RIGHT_SIZE[level] == (10, 14, 28, 40)[level - 1] and exp["n_keep"] > 1000
    assert exp["rotation"] == (6 if rotate else 0)
    check(ctx, s, True, True, exp)
    if not rotate:
        exp = S.oracle(s, True, False)
        assert exp["scale"] == level
        check(ctx, s, True, False, exp)


def test_first_of_two_tied_runs_wins(ctx):
    """smooth scene 21 of 120 matches: the runs (0, 0) and (2, 0) keep the same number of matches but different ones (found by a seed search
    with the oracle)"""
    from matchinglib_poselib_amd import synth

    s = synth.gms_scene("smooth", 120, seed=21)
    exp = S.oracle(s, True, True)
    first = (exp["scale"], exp["rotation"])
    tied = [k for k, c in exp["counts"].items() if c == exp["n_keep"] and k != first and (exp["masks"][k] != exp["keep"]).any()]
    assert exp["n_keep"] > 0 and tied and all(k > first for k in tied)
    check(ctx, s, True, True, exp)


@pytest.mark.parametrize("use_scale", [False, True])
@pytest.mark.parametrize("ka,kb,winner", [(5, 5, 2), (4, 5, 6), (5, 4, 2)])
def test_tie_between_rotation_types_of_one_scale_level(ctx, ka, kb, winner, use_scale):
    """two blocks of 9 ka and 9 kb matches, one consistent at rotation type 2 only, the other at type 6 only: at ka = kb the runs (0, 2) and
    (0, 6) tie on 45 matches with different masks and the first wins (with the scale switch, level 2 ties as well); otherwise the larger"""
    s = S.rotation_tie_scene(ka, kb)
    exp = S.oracle(s, use_scale, True)
    c = exp["counts"]
    assert (c[(0, 0)], c[(0, 2)], c[(0, 6)]) == (0, 9 * ka, 9 * kb) and (exp["masks"][(0, 2)] != exp["masks"][(0, 6)]).any()
    assert (exp["scale"], exp["rotation"], exp["n_keep"]) == (0, winner, 9 * max(ka, kb))
    assert not use_scale or c[(2, 2)] == c[(0, 2)]                           # a later scale level reaches the same count and must not win
    got, _ = check(ctx, s, use_scale, True, exp)
    assert got["keep"][s["A" if winner == 2 else "B"]].all() and not got["keep"][s["B" if winner == 2 else "A"]].any()


# ---- 3. the carried-over drop

def test_a_match_dropped_at_one_grid_type_stays_dropped(ctx):
    s = S.carry_over_scene()
    exp, off = S.oracle(s), S.oracle(s, carry=False)
    assert exp["keep"].tobytes() != off["keep"].tobytes()                     # the scene depends on the carry-over
    assert exp["keep"][s["A"]].all() and not exp["keep"][s["B"]].any() and off["keep"][s["B"]].all()
    got, _ = check(ctx, s, exp=exp)
    assert got["keep"][s["A"]].all()                                          # the flag earned at grid type 1 survives the drop at type 2


# ---- 4. boundary arithmetic

def test_cell_boundaries_with_separate_rounding(ctx):
    s = S.boundary_scene()
    exp, fused = S.oracle(s), S.oracle(s, fused=True)
    flips = int((exp["keep"] != fused["keep"]).sum())
    print(f"{flips} of {len(s['matches'])} matches flip under a contracted multiply-add")
    assert flips >= len(s["flip"]) > 0
    check(ctx, s, exp=exp)
    check(ctx, s, True, True)
    u = S.unit_edge_scene()
    assert (G.normalise(u["kp2"], u["size2"])[0] == 1.0).any()                # x just below the width normalises to 1.0f
    check(ctx, u)
    check(ctx, u, True, False)


# ---- 5. threshold ties

def test_threshold_ties(ctx):
    s = S.tie_threshold_scene()
    got, exp = check(ctx, s)
    assert all(got["keep"][g].all() for g in s["groups"].values()) and got["n_keep"] == 37
    check(ctx, s, True, True)


# ---- 6. deviations from the reference and argument checks

def _with_extra(base, p1, p2):
    s = dict(base)
    n1, n2 = len(base["kp1"]), len(base["kp2"])
    s["kp1"] = np.concatenate([base["kp1"], np.asarray([p1], np.float32)])
    s["kp2"] = np.concatenate([base["kp2"], np.asarray([p2], np.float32)])
    m = np.zeros(1, S.DMATCH)
    m["queryIdx"], m["trainIdx"] = n1, n2
    s["matches"] = np.concatenate([base["matches"], m])
    return s


def test_out_of_bounds_cases_are_dropped_and_counted(ctx):
    from matchinglib_poselib_amd import synth

    w, h = 1920, 480
    base = synth.gms_scene("smooth", 500, seed=3, width=w, height=h)
    ref, _ = check(ctx, base)
    assert ref["dropped"] == 0 and ref["n_keep"] > 100
    inside = (5.25 * w / 20, 5.25 * h / 20)
    cases = {
        "right index past the table": (inside, (S.ulps(w, -1), 19.5 * h / 20)),
        "NaN on the left": ((float("nan"), 100.0), inside),
        "1e30 on the right": (inside, (100.0, 1e30)),
        "infinity on the left": ((float("inf"), 100.0), inside),
    }
    for name, (p1, p2) in cases.items():
        s = _with_extra(base, p1, p2)
        got, _ = check(ctx, s)
        assert got["dropped"] == 1 and not got["keep"][-1], name
        assert got["keep"][:-1].tobytes() == ref["keep"].tobytes() and got["n_keep"] == ref["n_keep"], name   # nothing else moves
    # a negative x on the left is not checked by the reference: column -1 of row 6 is the last cell of row 5
    s = _with_extra(base, (-10.0, 6.25 * h / 20), inside)
    got, exp = check(ctx, s)
    assert got["dropped"] == 0
    xn, yn = G.normalise(s["kp1"], s["size1"])
    assert G.left_codes(xn[-1:], yn[-1:], 1)[0] == 20 * 6 - 1
    check(ctx, s, True, True)


def test_bad_arguments(ctx):
    from matchinglib_poselib_amd import matching, synth

    s = synth.gms_scene("smooth", 64, seed=0)
    for size1, size2 in (((0, 720), (1280, 720)), ((1280, -1), (1280, 720)), ((1280, 720), (0, 720)), ((1280, 720), (1280, 0))):
        bad_input(lambda: matching.gms_filter(s["kp1"], size1, s["kp2"], size2, s["matches"], ctx=ctx))
    for field, value in (("queryIdx", 64), ("queryIdx", -1), ("trainIdx", 64), ("trainIdx", -1)):
        m = s["matches"].copy()
        m[field][10] = value
        bad_input(lambda: matching.gms_filter(s["kp1"], s["size1"], s["kp2"], s["size2"], m, ctx=ctx))
    n, out = matching.filter_matches_gms(s["kp1"], s["size1"], s["kp2"], s["size2"], s["matches"][:0], ctx=ctx)
    assert n == 0 and len(out) == 0


# ---- 7. the batched device entry

@pytest.mark.parametrize("rule", [False, True])
def test_batch_is_byte_identical_to_the_single_entry(ctx, rule):
    """seven lists of 0, 1, 64, 65, 1025, 2000 and match_stride matches in one launch: the last one is the output of match_hamming_device
    on a synth.stereo_pair (no ratio test: one match per query), the others crafted scenes"""
    import torch
    from matchinglib_poselib_amd import matching, synth

    stride, size = 2048, (1280, 720)
    dev = torch.device("cuda:0")
    sp = synth.stereo_pair(stride, seed=20261801)
    mo = matching.match_hamming_device(torch.from_numpy(sp["desc1"]).to(dev), torch.from_numpy(sp["desc2"]).to(dev), ratio_test=False, ctx=ctx)
    torch.cuda.synchronize()
    assert int(mo["count"][0]) == stride
    counts = [0, 1, 64, 65, 1025, 2000, stride]
    B = len(counts)
    kp1, kp2 = np.zeros((B, stride, 2), np.float32), np.zeros((B, stride, 2), np.float32)
    m = np.zeros((B, stride), S.DMATCH)
    for b, n in enumerate(counts[:-1]):
        s = synth.gms_scene("smooth" if b % 2 else "rot90", n, seed=40 + b)
        kp1[b, :n], kp2[b, :n], m[b, :n] = s["kp1"], s["kp2"], s["matches"]
    kp1[-1], kp2[-1] = sp["kp1"] * 2.0, sp["kp2"] * 2.0   # the 640 x 480 pair spread over the 1280 x 720 grid
    m[-1] = mo["matches"][0].cpu().numpy().view(S.DMATCH).reshape(-1)
    d_m = torch.from_numpy(m.view(np.int32).reshape(B, stride, 4)).to(dev)
    d_n = torch.tensor(counts, dtype=torch.int32, device=dev)
    for use_scale, use_rotation in ((False, False), (True, True)):
        out = matching.gms_filter_matches_device(d_m, d_n, torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev), size, size, use_scale,
                                                 use_rotation, min_final_rule=rule, ctx=ctx)
        torch.cuda.synchronize()
        om, oc, oi = out["matches"].cpu().numpy(), out["count"].cpu().numpy(), out["inliers"].cpu().numpy()
        for b, n in enumerate(counts):
            g = matching.gms_filter(kp1[b], size, kp2[b], size, m[b, :n], use_scale, use_rotation, ctx=ctx)
            exp = m[b, :n][g["keep"]] if (not rule or g["n_keep"] >= 2) else m[b, :n]
            assert oi[b] == g["n_keep"] and oc[b] == len(exp), (b, n)
            assert om[b, :len(exp)].tobytes() == exp.view(np.int32).reshape(-1, 4).tobytes(), (b, n)
        print(f"rule {rule} scale {use_scale} rotation {use_rotation}: kept {oi.tolist()} of {counts}")


def test_min_final_rule_at_one_and_two_kept(ctx):
    """correspondences.cpp:388-397: a filter count of 1 passes the list through, a count of 2 replaces it"""
    import torch
    from matchinglib_poselib_amd import matching

    dev = torch.device("cuda:0")
    scenes = [S.final_rule_scene(1), S.final_rule_scene(2)]
    n = len(scenes[0]["matches"])
    m = np.stack([s["matches"] for s in scenes])
    d_m = torch.from_numpy(m.view(np.int32).reshape(2, n, 4)).to(dev)
    d_n = torch.tensor([n, n], dtype=torch.int32, device=dev)
    k1 = torch.from_numpy(np.stack([s["kp1"] for s in scenes])).to(dev)
    k2 = torch.from_numpy(np.stack([s["kp2"] for s in scenes])).to(dev)
    for rule in (False, True):
        out = matching.gms_filter_matches_device(d_m, d_n, k1, k2, (S.W, S.H), (S.W, S.H), min_final_rule=rule, ctx=ctx)
        torch.cuda.synchronize()
        om, oc, oi = out["matches"].cpu().numpy(), out["count"].cpu().numpy(), out["inliers"].cpu().numpy()
        assert oi.tolist() == [1, 2]
        assert oc.tolist() == ([n, 2] if rule else [1, 2])
        for b, s in enumerate(scenes):
            g, _ = check(ctx, s)
            exp = s["matches"] if (rule and b == 0) else s["matches"][g["keep"]]
            assert om[b, :len(exp)].tobytes() == exp.view(np.int32).reshape(-1, 4).tobytes()


# ---- 8. the C++ drop-in

@pytest.mark.parametrize("kind,switches", [("smooth", (0, 0)), ("scale2", (1, 1)), ("rot90", (0, 0))])
def test_cpp_facade_equals_python(ctx, tmp_path, kind, switches):
    """both overloads of filterMatchesGMS; rot90 without the rotation switch keeps nothing: the mask handed in stays as it was and the list
    comes back empty"""
    from matchinglib_poselib_amd import synth

    assert os.path.exists(FACADE_EXE), "run __graft_entry__.build() first"
    s = synth.gms_scene(kind, 1000, seed=2)
    g = device(ctx, s, *switches)
    n = len(s["matches"])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<7i", n, n, n, s["size1"][0], s["size1"][1], *switches))
        f.write(s["kp1"].tobytes() + s["kp2"].tobytes() + s["matches"].tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "matchinglib_poselib_amd", "lib") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([FACADE_EXE, str(fin), str(fout)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout
    blob = open(fout, "rb").read()
    c_mask, n_mask = struct.unpack_from("<2i", blob, 0)
    mask = np.frombuffer(blob, np.uint8, n_mask, 8)
    c_list, n_list = struct.unpack_from("<2i", blob, 8 + n_mask)
    lst = np.frombuffer(blob, S.DMATCH, n_list, 16 + n_mask)
    assert c_mask == c_list == g["n_keep"] == n_list
    if g["n_keep"]:
        assert mask.astype(bool).tobytes() == g["keep"].tobytes()
        assert lst.tobytes() == s["matches"][g["keep"]].tobytes()
    else:
        assert kind == "rot90" and mask.tolist() == [1, 0, 1]
    assert (g["n_keep"] == 0) == (kind == "rot90")
