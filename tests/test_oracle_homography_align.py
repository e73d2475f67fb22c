"""CPU-only: the sequential restatement of the homography alignment (tests/cpp/homography_align_oracle.cpp) against itself, numpy and
the golden trace -- the yardstick S_A, the admissibility of every scene the device tests use, the convention guard, the defined
failures, and the two numerical building blocks (cyclic Jacobi 3 x 3, the equilibrated LU)."""
import os

import numpy as np
import pytest

import homography_align_oracle as hao
import homography_pose_scenes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "homography_align_trace.npz")
ALL = [c[0] for c in S.SCENES + S.GUARD]
_cache = {}


def both(name):
    if name not in _cache:
        sc = S.scene(name)
        _cache[name] = (sc, [hao.alignment(sc["p1"], sc["p2"], sc["labels"], sc["P"], sc["H0"], sc["th"], v) for v in (0, 1)])
    return _cache[name]


@pytest.mark.parametrize("name", ALL)
def test_variants_agree_and_scene_is_admissible(name):
    sc, (a, b) = both(name)
    assert a["code"] == 0 and b["code"] == 0
    d = S.variant_distance(a, b)
    print(f"{name}: S = {d:.3e}, stop margin {min(a['margin_stop'], b['margin_stop']):.3e}, q margin {min(a['margin_q'], b['margin_q']):.3e}, "
          f"rounds {a['rounds'].tolist()}")
    assert d <= S.S_A, f"{name}: variants differ by {d:.3e} > S_A"
    assert 64 * d <= S.tol_of(S.units_of(name)) <= S.TOL_A < 1e-6                                    # the allowance covers this scene and stays below the project's bar
    assert S.same_decisions(a, b)
    assert min(a["margin_stop"], b["margin_stop"]) >= S.MARGIN
    assert min(a["margin_q"], b["margin_q"]) >= S.MARGIN


def test_scenes_cover_both_stop_tests_and_the_round_limit():
    _, (a, _) = both("exact")
    assert a["e1"][a["q"]] < S.scene("exact")["th"] and a["rounds"][a["q"], 0] == 4 and a["rounds"][a["q"], 1] == 0      # e1 < tol at iter 3
    sc, (a, _) = both("slow")
    assert (a["e1"] > sc["th"]).all() and a["rounds"].max() < 40                                                      # the |e1 - e2| test
    _, (a, _) = both("forty")
    assert (a["rounds"][0] == 40).all()                                                                               # neither


@pytest.mark.parametrize("name", [c[0] for c in S.GUARD])
def test_convention_guard(name):
    """R is the planted rotation (camera 1 -> camera 2), t is minus the planted position of camera 2 in camera 1's frame: catches a
    swapped or transposed R and a sign error in t.  Noise-free, well separated normals, baseline >= 10 % of the depth."""
    sc, (a, _) = both(name)
    normals = [m / np.linalg.norm(m) for m in sc["normals"]]
    for i in range(sc["P"]):
        for j in range(i):
            assert S.angle_deg_vec(normals[i], normals[j]) >= 30.0
    depth = min(1.0 / m[2] for m in sc["normals"])
    assert np.linalg.norm(sc["t"]) >= 0.1 * depth
    assert S.angle_deg_rot(a["R"], sc["R"]) < 0.5
    assert S.angle_deg_rot(a["R"], sc["R"].T) > 1.0
    assert S.angle_deg_vec(a["t"], -sc["t"]) < 0.5
    assert abs(np.linalg.norm(a["t"]) - 1.0) < 1e-12
    # the sign that puts the points in front: P2 = R (P1 - t'), t' = -|t| a["t"], has positive depth for every plane point
    scale = np.linalg.norm(sc["t"])
    on = sc["labels"] >= 0
    ray = np.c_[sc["p1"][on], np.ones(on.sum())]
    z = 1.0 / np.einsum("ij,ij->i", ray, sc["normals"][sc["labels"][on]])
    P2 = (ray * z[:, None] + scale * a["t"]) @ a["R"].T
    assert (P2[:, 2] > 0).all()
    # The planes' homographies under the common motion are the planted ones -- plane 0 always; the further planes only when the first
    # candidate (q = 0) won, because the reference combines the chosen motion with the plane offsets of the FIRST candidate's run
    # (dn2.rowRange(0, num_patches), HomographyAlignment.cpp:336) and the restatement follows it.
    for k in range(sc["P"] if a["q"] == 0 else 1):
        assert np.abs(a["Hs"][k] - sc["Hs"][k]).max() < 1e-6


def test_golden_trace():
    g = np.load(GOLDEN)
    for name in S.FIXTURE:
        _, (a, _) = both(name)
        gi = g[name + "_info"]
        assert (gi[:10] == a["info"][:10]).all() and (gi[16:18] == a["info"][16:18]).all()      # the decisions: exactly
        assert np.abs(gi[10:16] - a["info"][10:16]).max() <= S.S_A                              # the recorded errors: as the other keys
        for key in ("R", "t", "E", "norms", "Hs"):
            assert np.abs(g[f"{name}_{key}"] - a[key]).max() <= S.S_A, (name, key)


def test_defined_failures():
    sc = S.scene("p2_n63")
    # one plane only: the reference's defined answer
    one = np.where(sc["labels"] == 0, 0, -1).astype(np.int32)
    r = hao.alignment(sc["p1"], sc["p2"], one, 1, sc["H0"], sc["th"])
    assert (r["code"], r["reason"]) == (-3, 5)
    # a pure rotation: the degenerate branch is followed as written; the two rays of every correspondence are parallel, so
    # Check_motion_error counts nothing (and t = 0 could not be normalised either)
    Rz = S.rodrigues([0.2, -0.1, 1.0], 0.05)
    p2 = np.c_[sc["p1"], np.ones(len(sc["p1"]))] @ Rz.T
    r = hao.alignment(sc["p1"], p2[:, :2] / p2[:, 2:3], sc["labels"], 2, Rz, sc["th"])
    assert (r["code"], r["reason"]) == (-3, 3)
    # an H0 the decomposition refuses: the two largest eigenvalues of H^T H are equal, the third is not (d0 > 1 fails)
    r = hao.alignment(sc["p1"], sc["p2"], sc["labels"], 2, np.diag([1.0, 1.0, 0.5]), sc["th"])
    assert (r["code"], r["reason"]) == (-3, 1)
    # a plane without correspondences
    lab = np.where(sc["labels"] == 1, -1, sc["labels"]).astype(np.int32)
    r = hao.alignment(sc["p1"], sc["p2"], lab, 2, sc["H0"], sc["th"])
    assert (r["code"], r["reason"]) == (-3, 6)
    # every ray pair parallel: Check_motion_error counts nothing
    same = hao.alignment(sc["p1"], sc["p1"], sc["labels"], 2, sc["H0"], sc["th"])
    assert same["code"] == -3 and same["reason"] in (3, 4)


def test_jacobi33_against_numpy():
    rng = np.random.default_rng(7)
    for _ in range(200):
        M = rng.normal(size=(3, 3))
        A = M.T @ M
        for variant in (0, 1):
            ok, d, v = hao.jacobi33(A, variant)
            assert ok == 1
            w = np.linalg.eigvalsh(A)[::-1]
            assert (np.diff(d) <= 0).all()
            # the sweeps end at an off-diagonal sum of 1e-6: eigenvalues to ~1e-12 relative to the gap, vectors orthonormal to rounding
            assert np.abs(d - w).max() <= 1e-9 * max(1.0, w[0])
            assert np.abs(v.T @ v - np.eye(3)).max() < 1e-13
            assert np.abs(v.T @ A @ v - np.diag(np.diag(v.T @ A @ v))).max() < 2e-6


def test_equilibrated_lu_against_numpy():
    rng = np.random.default_rng(8)
    for n in (3, 11, 32):
        for _ in range(50):
            M = rng.normal(size=(n + 5, n))
            A = M.T @ M * np.exp(rng.uniform(-6, 6, n))[:, None]     # badly scaled rows: what the equilibration is for
            b = rng.normal(size=n)
            ok, m = hao.solve_by_inverse(A, b)
            assert ok == 1
            x = np.linalg.solve(A, b)
            assert np.abs(m - x).max() <= 1e-9 * np.linalg.cond(A) * np.abs(x).max() * 1e-3 + 1e-12
    A = np.ones((11, 11))
    assert hao.solve_by_inverse(A, np.ones(11))[0] == 0                # singular
    A = np.eye(11)
    A[4, :] = 0
    assert hao.solve_by_inverse(A, np.ones(11))[0] == 0                # a zero column of the transposed system


# ---- the whole function: the composition of the two restatements -------------------------------------------------------------------------
FULL_CASES = [(c[0], False) for c in S.FULL] + [("full_two", True)]


@pytest.mark.parametrize("name,masked", FULL_CASES)
def test_full_scene_is_admissible(name, masked):
    import homography_scenes as hs

    sc = S.full_scene(name)
    mask = S.full_mask(len(sc["p1"])) if masked else None
    a, b = [hao.pose_homographies(sc["p1"], sc["p2"], sc["th"], mask=mask, variant=v) for v in (0, 1)]
    assert a["result"] == 0 and b["result"] == 0
    assert a["n_planes"] == b["n_planes"] >= 2 and (a["num_inl"] == b["num_inl"]).all() and (a["rng_state"] == b["rng_state"]).all()
    assert (a["labels"] == b["labels"]).all() and (a["mask"] == b["mask"]).all()
    assert max(a["doubt"], b["doubt"]) <= hs.TOL_H
    assert min(a["margin_planes"], b["margin_planes"]) >= 1000 * hs.TOL_H * hs.max_coord(sc["p1"], sc["p2"]) / sc["th"]
    assert S.same_decisions(a["align"], b["align"])
    d = max(S.variant_distance(a["align"], b["align"]), np.abs(a["E"] - b["E"]).max())
    m = min(a["margin_mask"], b["margin_mask"], a["align"]["margin_stop"], b["align"]["margin_stop"], a["align"]["margin_q"], b["align"]["margin_q"])
    print(f"{name} masked={masked}: S = {d:.3e}, closest comparison {m:.3e}, planes {a['num_inl'].tolist()}, inliers {a['n_inliers']}")
    assert d <= S.S_A and m >= S.FULL_MARGIN


def test_full_defined_results():
    sc = S.full_scene("full_one")
    assert hao.pose_homographies(sc["p1"], sc["p2"], sc["th"])["result"] == -3
    sc = S.full_scene("full_weak")
    r = hao.pose_homographies(sc["p1"], sc["p2"], sc["th"], check_plane_strength=True)
    assert r["result"] == -2 and r["n_planes"] >= 1 and r["strength"].sum() <= 0.5
    p1, p2, th = S.noise_scene()
    assert hao.pose_homographies(p1, p2, th)["result"] == -1
    assert hao.pose_homographies(p1[:3], p2[:3], th)["result"] == -3                                   # fewer than 4 rows: no plane, no pose
    assert hao.pose_homographies(p1[:3], p2[:3], th, check_plane_strength=True)["result"] == -2
