"""CPU-only: the two restatements of the GMS match filter in tests/gms_oracle.py (the literal dense-table one and the bucket one) agree on every
synthetic scene kind, with and without the scale and rotation switches, and the crafted scenes of tests/gms_scenes.py have the properties the
GPU tests rely on.  The reference itself needs OpenCV and is not compiled: parity at this boundary rests on these two restatements."""
import numpy as np
import pytest

import gms_oracle as G
import gms_scenes as S

SIZES = [0, 1, 4, 63, 64, 65, 257, 1025, 4096]
KINDS = ["smooth", "rot90", "scale2", "sparse"]


def both(s, use_scale, use_rotation):
    a = G.gms_oracle(s["kp1"], s["size1"], s["kp2"], s["size2"], s["matches"], use_scale, use_rotation)
    b = G.gms_buckets(s["kp1"], s["size1"], s["kp2"], s["size2"], s["matches"], use_scale, use_rotation)
    assert a["keep"].tobytes() == b["keep"].tobytes()
    assert [a[k] for k in ("n_keep", "scale", "rotation", "dropped")] == [b[k] for k in ("n_keep", "scale", "rotation", "dropped")]
    return a


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_restatements_agree(kind, n):
    from matchinglib_poselib_amd import synth

    s = synth.gms_scene(kind, n, seed=n % 7)
    for use_scale in (False, True):
        for use_rotation in (False, True):
            a = both(s, use_scale, use_rotation)
            assert a["n_keep"] == int(a["keep"].sum()) and (a["n_keep"] > 0) == (a["scale"] >= 0) == (a["rotation"] >= 0)


def test_rotation_patterns_are_rotations():
    """every pattern is a permutation with the centre fixed; type r is type 1 applied r times"""
    step = G.PATTERN[1]
    cur = np.arange(9)
    for r in range(8):
        assert sorted(G.PATTERN[r]) == list(range(9)) and G.PATTERN[r][4] == 4
        assert G.PATTERN[r].tolist() == cur.tolist()
        cur = cur[step]
    assert G.RIGHT_SIZE == (20, 10, 14, 28, 40)
    assert G._bucket_pattern() == G.PATTERN.tolist()   # the second restatement's table, derived from angles


def test_scene_kinds_exercise_the_switches():
    from matchinglib_poselib_amd import synth

    r = both(synth.gms_scene("rot90", 2000, 0), True, True)
    assert r["rotation"] != 0 and r["n_keep"] > 1000
    assert both(synth.gms_scene("rot90", 2000, 0), False, True)["rotation"] != 0
    r = both(synth.gms_scene("scale2", 2000, 0), True, True)
    assert r["scale"] == 1 and r["n_keep"] > 1000
    assert both(synth.gms_scene("scale2", 2000, 0), True, False)["scale"] == 1


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("ratio,level", [(2.0, 1), (2.0 ** 0.5, 2), (0.5 ** 0.5, 3), (0.5, 4)])
def test_scaled_scenes_win_at_their_scale_level(ratio, level, rotate):
    r = both(S.scaled_scene(ratio, 2000, 0, rotate), True, True)
    assert (r["scale"], r["rotation"]) == (level, 6 if rotate else 0) and r["n_keep"] > 1000


@pytest.mark.parametrize("ka,kb,winner", [(5, 5, 2), (4, 5, 6), (5, 4, 2)])
def test_rotation_tie_scene(ka, kb, winner):
    s = S.rotation_tie_scene(ka, kb)
    for use_scale in (False, True):
        r = both(s, use_scale, True)
        assert (r["scale"], r["rotation"], r["n_keep"]) == (0, winner, 9 * max(ka, kb))
        assert (r["counts"][(0, 2)], r["counts"][(0, 6)]) == (9 * ka, 9 * kb)


def test_crafted_scenes_agree_and_hold_their_properties():
    s = S.carry_over_scene()
    a, off = both(s, False, False), S.oracle(s, carry=False)
    assert a["keep"][s["A"]].all() and not a["keep"][s["B"]].any() and off["keep"][s["B"]].all()
    s = S.boundary_scene()
    a, fused = both(s, False, False), S.oracle(s, fused=True)
    assert a["keep"][s["flip"]].all() and not fused["keep"][s["flip"]].any()
    both(s, True, True)
    s = S.unit_edge_scene()
    a = both(s, False, False)
    assert (G.normalise(s["kp2"], s["size2"])[0] == 1.0).any() and (G.normalise(s["kp2"], s["size2"])[1] == 1.0).any() and a["keep"][s["U1"]].all()
    s = S.tie_threshold_scene()
    a = both(s, False, False)
    assert all(a["keep"][g].all() for g in s["groups"].values()) and a["n_keep"] == 37   # every tie evaluates to "kept" in float64
    for k in (1, 2):
        assert both(S.final_rule_scene(k), False, False)["n_keep"] == k
