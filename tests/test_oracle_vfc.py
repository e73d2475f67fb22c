"""CPU-only: the numpy restatement of the VFC match filter (vfc_oracle.py) against itself -- the reference's float32 arithmetic against
float64, and float64 against float64 in the reverse summation order.  What these tests establish is what the GPU tests rely on:

* on separable ("clean") scenes the posterior P is bimodal, both arithmetics keep the same matches and no P comes within 0.2 of the
  threshold 0.75;
* on "graded" scenes the two float64 orders still keep the same matches; their largest |dP| is the oracle's own spread, recorded in
  tests/golden/vfc_spread.json (the GPU test's band is ten times that).

The m x m system of SparseVFC is numerically singular, and at n = 40 the reference's float LU hits cv::solve's singular rule in several
of its 50 solves.  When that happens late, the float32 run ends on garbage (C = 0 one iteration before the end) while float64 does not:
vfc_scene's generator constant was chosen among twenty tried so that none of the twelve clean scenes below ends that way (the others
failed on one or two of the n = 40 scenes).  That is a property of the reference's arithmetic, not of the device code, which these
tests do not touch.
"""
import json
import os

import numpy as np
import pytest

import vfc_oracle as VO
from matchinglib_poselib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD_JSON = os.path.join(ROOT, "tests", "golden", "vfc_spread.json")
GRADED = [(n, seed) for n in (257, 1025) for seed in range(4)]


def random_scene(n, seed):
    """matches between unrelated points: the scenes on which fewer than 10 % survive (rc = -2)"""
    rng = np.random.default_rng(500 + seed)
    return (rng.random((n, 2)) * [1280, 720]).astype(np.float32), (rng.random((n, 2)) * [1280, 720]).astype(np.float32)


MINUS2 = [(100, 0), (300, 1)]   # found by a search over seeds 0-11: both arithmetics answer -2 with every P at least 0.19 from 0.75


@pytest.mark.parametrize("n", [40, 300, 2000])
@pytest.mark.parametrize("seed", range(4))
def test_clean_scenes_both_arithmetics_agree(n, seed):
    s = synth.vfc_scene("clean", n, seed)
    a = VO.vfc(s["x1"], s["x2"], 1, "float32_serial")
    b = VO.vfc(s["x1"], s["x2"], 1, "float64")
    print(f"n={n} seed={seed}: kept {a['n_keep']} / {b['n_keep']}, margins {a['margin']:.4f} / {b['margin']:.4f}, iterations "
          f"{a['iterations']} / {b['iterations']}, singular solves {a['singular']} / {b['singular']}, max|dP| {np.abs(a['P'] - b['P']).max():.2e}")
    assert a["rc"] == b["rc"] == 0 and a["m"] == b["m"] == 16
    assert (a["keep"] == b["keep"]).all()
    assert a["margin"] >= 0.2 and b["margin"] >= 0.2
    assert (b["keep"] == s["inlier"]).all()


def graded_spread():
    spread, rows = 0.0, []
    for n, seed in GRADED:
        s = synth.vfc_scene("graded", n, seed)
        f = VO.vfc(s["x1"], s["x2"], 1, "float64", "forward")
        r = VO.vfc(s["x1"], s["x2"], 1, "float64", "reverse")
        d = float(np.abs(f["P"] - r["P"]).max())
        rows.append(dict(kind="graded", n=n, seed=seed, same_keep=bool((f["keep"] == r["keep"]).all()), dP=d,
                         iterations=[f["iterations"], r["iterations"]]))
        spread = max(spread, d)
    return spread, rows


def test_graded_scenes_orders_agree_and_spread_is_recorded():
    """The recorded value is data: it is rewritten only when VFC_WRITE_SPREAD=1 (or when the file is missing); otherwise the test checks that
    what it computes now is the recorded value up to a factor of two (exp and the summation of another numpy build may differ in the last
    bits, and the spread is a maximum over few iteration counts)."""
    spread, rows = graded_spread()
    for r in rows:
        print(r)
        assert r["same_keep"], r
    if os.environ.get("VFC_WRITE_SPREAD") == "1" or not os.path.exists(SPREAD_JSON):
        with open(SPREAD_JSON, "w") as f:
            json.dump(dict(spread=spread, theta=0.75, seed=1, scenes=rows), f, indent=1)
            f.write("\n")
    rec = json.load(open(SPREAD_JSON))
    assert [(r["n"], r["seed"]) for r in rec["scenes"]] == GRADED
    assert 0.5 * rec["spread"] <= spread <= 2.0 * rec["spread"], (spread, rec["spread"])


def test_fewer_than_five():
    s = synth.vfc_scene("clean", 4, 0)
    for mode in ("float32_serial", "float64"):
        assert VO.vfc(s["x1"], s["x2"], 1, mode)["rc"] == -1


def test_small_scale_keeps_all():
    rng = np.random.default_rng(3)
    x1 = (np.array([600.0, 300.0]) + rng.random((50, 2)) * 0.1).astype(np.float32)    # RMS radius below 0.1 px: normalize() refuses
    x2 = (rng.random((50, 2)) * [1280, 720]).astype(np.float32)
    for mode in ("float32_serial", "float64"):
        r = VO.vfc(x1, x2, 1, mode)
        assert r["rc"] == 0 and r["refused"] and r["keep"].all() and r["iterations"] == 0 and r["m"] == 0


def test_pure_translation_keeps_all_without_iterating():
    s = synth.vfc_scene("clean", 100, 0)
    x2 = (s["x1"] + np.float32([32.0, -16.0])).astype(np.float32)    # exact in float32 for these magnitudes: Y = 0 up to rounding
    for mode in ("float32_serial", "float64"):
        r = VO.vfc(s["x1"], x2, 1, mode)
        assert r["rc"] == 0 and not r["refused"] and r["iterations"] == 0 and r["keep"].all() and r["sigma2"] <= 1e-8


def test_duplicated_points_give_fewer_control_points():
    s = synth.vfc_scene("clean", 8, 0)
    x1, x2 = np.tile(s["x1"], (8, 1)), np.tile(s["x2"], (8, 1))     # 64 matches on 8 distinct points
    for mode in ("float32_serial", "float64"):
        r = VO.vfc(x1, x2, 1, mode)
        assert r["rc"] in (0, -2) and 1 <= r["m"] <= 8


@pytest.mark.parametrize("n,seed", MINUS2)
def test_minus_two(n, seed):
    x1, x2 = random_scene(n, seed)
    a, b = VO.vfc(x1, x2, 1, "float32_serial"), VO.vfc(x1, x2, 1, "float64")
    assert a["rc"] == b["rc"] == -2
    assert a["n_keep"] / n < 0.1 and b["n_keep"] / n < 0.1
    assert a["margin"] >= 0.19 and b["margin"] >= 0.19


def test_getmatches_rule():
    assert VO.getmatches_rule(0, 9, 24) and VO.getmatches_rule(0, 9, 23)
    assert not VO.getmatches_rule(0, 8, 24)
    assert VO.getmatches_rule(0, 8, 23)
    assert not VO.getmatches_rule(-2, 9, 24) and not VO.getmatches_rule(-2, 0, 23) and not VO.getmatches_rule(-1, 3, 3)
    # through the list filter: 23 and 24 matches of which the filter keeps eight or nine
    s = synth.vfc_scene("clean", 24, 5)
    m = np.zeros(24, dtype=[("queryIdx", np.int32), ("trainIdx", np.int32), ("imgIdx", np.int32), ("distance", np.float32)])
    m["queryIdx"] = m["trainIdx"] = np.arange(24)
    for n in (23, 24):
        r = VO.vfc(s["x1"][:n], s["x2"][:n], 1)
        rc, out = VO.filter_matches(s["x1"], s["x2"], m[:n], 1, rule=True)
        assert rc == r["rc"] and len(out) == (r["n_keep"] if VO.getmatches_rule(r["rc"], r["n_keep"], n) else n)


def test_glibc_rand_known_values():
    """srand(1): the first values every glibc prints"""
    assert VO.glibc_rand(1, 3).tolist() == [1804289383, 846930886, 1681692777]
    assert VO.glibc_rand(0, 3).tolist() == VO.glibc_rand(1, 3).tolist()
