"""CPU tests of the sequential restatement of computeHomographyArrsac / estimateMultHomographys (tests/cpp/homography_oracle.cpp): every
committed scene is admissible (tests/homography_scenes.py says what that means), S_MAX holds, the planted planes are found, the fixture
is reproduced, the streams carry over, and the special paths (n = 4, a scene on which every sample fails) behave as the reference's."""
import os

import numpy as np
import pytest

import homography_oracle as ho
import homography_scenes as hs

FRESH = np.array(ho.RNG_FRESH, np.uint64)


def same_decisions(a, b, keys):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)


@pytest.mark.parametrize("name", [c[0] for c in hs.SINGLE])
def test_single_scene_is_admissible_and_finds_the_plane(name):
    p1, p2, H_true, planted, th = hs.single(name)
    a, b = ho.homography_arrsac(p1, p2, th), ho.homography_arrsac(p1, p2, th, variant=1)
    assert a["ok"] and same_decisions(a, b, ("ok", "stats", "rng_state", "mask", "n_inliers"))
    s = hs.h_dist(a["H"], b["H"])
    margin, need = min(a["margin"], b["margin"]), 1000 * hs.TOL_H * hs.max_coord(p1, p2) / th
    print(f"{name}: s = {s:.3e} (S_MAX {hs.S_MAX:.3e}), margin = {margin:.3e} (needs {need:.3e})")
    assert s <= hs.S_MAX
    assert margin >= need
    assert max(a["doubt"], b["doubt"]) <= hs.TOL_H   # no step the refinement rejected could have moved H by more than the tolerance
    # the planted plane: its points map within a few noise sigmas under the estimate, and the mask finds them
    sigma = hs._units([c for c in hs.SINGLE if c[0] == name][0][3])[3]
    err = np.linalg.norm(hs.apply_h(a["H"], p1[planted]) - p2[planted], axis=1)
    assert np.median(err) < 3 * sigma
    if len(p1) >= 99:
        assert a["mask"][planted].mean() >= 0.9 and a["mask"][~planted].sum() <= 3
    assert a["n_inliers"] == int(a["mask"].sum())


def test_generation_scene_reaches_the_generation_branch():
    assert hs.TOL_H == 64 * hs.S_MAX and hs.TOL_H < 1e-7   # the project's bar for ARRSAC models (tests/test_gpu_arrsac.py)
    p1, p2, _, _, th = hs.single("n1200_gen")
    assert ho.homography_arrsac(p1, p2, th)["stats"][5] > 0
    p1, p2, _, _, th = hs.single("n1500_ext")
    r = ho.homography_arrsac(p1, p2, th)
    assert r["stats"][5] > 0 and r["stats"][6] > 1024       # the preemptive stage runs past the rows every model is tested on


@pytest.mark.parametrize("name,kw", hs.MULTI_CASES)
def test_multi_scene_is_admissible(name, kw):
    p1, p2, Hs, label, th = hs.multi(name)
    a, b = ho.mult_homographies(p1, p2, th, **kw), ho.mult_homographies(p1, p2, th, variant=1, **kw)
    assert same_decisions(a, b, ("rc", "n_planes", "num_inl", "th_used", "strength", "masks", "rng_state"))
    s = max([hs.h_dist(x, y) for x, y in zip(a["H"], b["H"])], default=0.0)
    # every call inside runs at 1.5 th or more, and the margin is relative to the threshold of its call
    margin, need = min(a["margin"], b["margin"]), 1000 * hs.TOL_H * hs.max_coord(p1, p2) / (1.5 * th)
    print(f"{name} {kw}: s = {s:.3e}, margin = {margin:.3e} (needs {need:.3e})")
    assert s <= hs.S_MAX and margin >= need and max(a["doubt"], b["doubt"]) <= hs.TOL_H


def test_multi_planes_are_the_planted_ones():
    for name, counts in (("two", (260, 140)), ("three", (380, 220, 120))):
        p1, p2, Hs, label, th = hs.multi(name)
        r = ho.mult_homographies(p1, p2, th, min_pts_per_plane=30)
        assert r["rc"] == 0 and r["n_planes"] == len(counts)
        assert list(r["num_inl"]) == sorted(r["num_inl"], reverse=True)
        for k in range(len(counts)):   # planted in descending size, reported in descending size
            assert r["masks"][k][label == k].mean() > 0.85 and r["masks"][k].sum() == r["num_inl"][k]
            assert r["strength"][k] == th * 1.5 * float(r["num_inl"][k]) / (r["th_used"][k] * float(len(p1)))
        assert (r["masks"].sum(axis=0) <= 1).all()
    p1, p2, _, _, th = hs.multi("varth")
    r = ho.mult_homographies(p1, p2, th, min_pts_per_plane=30)
    assert r["rc"] == 0 and r["th_used"][0] == th * 1.5 * 1.5
    assert ho.mult_homographies(p1, p2, th, min_pts_per_plane=30, var_th=False)["rc"] == -1
    p1, p2, _, _, th = hs.multi("noise")
    assert ho.mult_homographies(p1, p2, th, var_th=False)["rc"] == -1


def test_fixture_is_reproduced():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "homography_trace.npz"))
    assert list(g["cases"]) == hs.FIXTURE
    for i, name in enumerate(hs.FIXTURE):
        p1, p2, _, _, th = hs.single(name)
        assert np.array_equal(p1, g[f"c{i}_p1"]) and np.array_equal(p2, g[f"c{i}_p2"]) and th == g[f"c{i}_th"][0]
        r = ho.homography_arrsac(g[f"c{i}_p1"], g[f"c{i}_p2"], th)
        assert r["ok"] == bool(g[f"c{i}_ok"][0]) and np.array_equal(r["stats"], g[f"c{i}_stats"]) and np.array_equal(r["rng_state"], g[f"c{i}_rng"])
        assert np.array_equal(np.packbits(r["mask"]), g[f"c{i}_mask"]) and hs.h_dist(r["H"], g[f"c{i}_H"]) <= hs.S_MAX


def test_streams_carry_over():
    p1, p2, _, _, th = hs.single("n1024")
    st = FRESH.copy()
    first = ho.homography_arrsac(p1, p2, th, rng_state=st)
    assert not np.array_equal(st, FRESH) and np.array_equal(st, first["rng_state"])
    second = ho.homography_arrsac(p1, p2, th, rng_state=st)
    assert second["ok"] and not np.array_equal(second["rng_state"], first["rng_state"])
    assert second["stats"].tolist() != first["stats"].tolist()   # other samples, other turns
    st2 = FRESH.copy()
    for _ in range(2):
        again = ho.homography_arrsac(p1, p2, th, rng_state=st2)
    assert np.array_equal(st2, st) and again["stats"].tolist() == second["stats"].tolist()


def test_four_points_take_the_direct_path():
    p1, p2, H_true, _, th = hs.single("n4")
    st = FRESH.copy()
    r = ho.homography_arrsac(p1, p2, th, rng_state=st)
    assert r["ok"] and np.array_equal(st, FRESH) and r["stats"].tolist() == [0] * 8
    assert r["mask"].tolist() == [1, 1, 1, 1] and r["n_inliers"] == 4
    assert np.abs(hs.apply_h(r["H"], p1) - p2).max() < 1e-8
    ok, H = ho.sample_model(p1, p2, [0, 1, 2, 3])
    assert ok and np.array_equal(H, r["H"])
    assert not ho.homography_arrsac(p1[:3], p2[:3], th)["ok"]


def test_every_sample_failing_ends_after_500_prosac_turns():
    p1, p2, th = hs.failing_scene()
    outs = [ho.homography_arrsac(p1, p2, th, variant=v) for v in (0, 1)]
    for r in outs:
        assert not r["ok"] and r["stats"].tolist() == [0, 0, 500, 0, 0, 0, 0, 0]
        assert r["rng_state"][1] == FRESH[1] and r["rng_state"][0] != FRESH[0]   # only the PROSAC stream moved
    assert np.array_equal(outs[0]["rng_state"], outs[1]["rng_state"])


def test_polish_of_a_twelve_point_sample_matters():
    p1, p2, lists = hs.sample_cases()
    ok0, H0 = ho.sample_model(p1, p2, lists["m12"], polish=False)
    ok1, H1 = ho.sample_model(p1, p2, lists["m12"], polish=True)
    assert ok0 and ok1 and hs.h_dist(H0, H1) > 1000 * hs.TOL_H
    assert not ho.sample_model(p1, p2, lists["flat"])[0]
    for name, idx in lists.items():
        if name != "flat":
            a, b = ho.sample_model(p1, p2, idx), ho.sample_model(p1, p2, idx, variant=1)
            assert a[0] and b[0] and hs.h_dist(a[1], b[1]) <= hs.S_MAX, name
