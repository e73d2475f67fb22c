"""Seed sweeps at the REFERENCE's RANSAC settings (1000 iterations, confidence 0.999: findEssentialMat as estimateEssentialMat("RANSAC") drives
it, pose_estim.cpp:870-873), with and without the least-squares refit, at the library's default options: iteration count, inlier count and
mask identical to the CPU oracle on every seed, E to 1e-7.  The same with the solver's safeguard off (A/B)."""
import numpy as np
import pytest

from matchinglib_poselib_amd import pose, synth
from option_guard import options

pytestmark = pytest.mark.gpu


def constraint_residual(E):
    E = np.asarray(E, np.float64).reshape(3, 3)
    E = E / np.linalg.norm(E)
    return max(np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max(), abs(np.linalg.det(E)))


def e_dist(a, b):
    a, b = np.ravel(a) / np.linalg.norm(a), np.ravel(b) / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


CASES = [(1500, 1000 + i, 50 + i) for i in range(120)] + [(5000, 20260103 + i, 12345 + i) for i in range(6)]


@pytest.mark.parametrize("refit", [False, True])
def test_reference_settings_over_120_seeds(ctx, oracle, refit):
    """120 (scene, seed) pairs of C3 shape (50 % inliers, 0.3 px noise; 1500 correspondences so that the CPU side stays within a minute)
    plus 6 at the full 5000, at the library's DEFAULT options (no option is touched): identical (iterations, inliers, mask) on EVERY
    seed, E to 1e-7 (measured: 1.8e-9)."""
    assert ctx.get_option("solver_polish") == 1
    diverged = []
    for n, scene_seed, seed in CASES:
        p1, p2, R, t, truth, th = synth.pose_scene(n, 0.5, seed=scene_seed)
        o = oracle.ransac_essential(p1, p2, th, confidence=0.999, max_iters=1000, lesqu=refit, seed=seed)
        g = pose.ransac_essential(p1, p2, th, confidence=0.999, max_iters=1000, refit=refit, seed=seed, ctx=ctx)
        assert g["ok"] == o["ok"]
        flips = int(np.count_nonzero(g["mask"] != o["mask"]))
        if g["iters"] == o["iters"] and g["n_inliers"] == o["n_inliers"] and flips == 0:
            assert e_dist(g["E"], o["E"]) < 1e-7, (n, scene_seed, seed, e_dist(g["E"], o["E"]))
            continue
        diverged.append((n, scene_seed, seed, g["iters"], o["iters"], g["n_inliers"], o["n_inliers"], flips))
    for d in diverged:
        print("n %d scene %d seed %d: iters %d/%d inliers %d/%d mask flips %d" % d)
    if not refit:
        assert not diverged, diverged                     # every run IS the CPU path's run
    else:
        # the refit solves an n-point system whose four smallest singular vectors come from different decompositions (Jacobi SVD of the
        # n x 9 matrix on the CPU, eigenvectors of the 9 x 9 Gram matrix on the device): a correspondence exactly at the threshold may
        # change sides.  At most 2 flips per run, on at most 5 % of the runs, and never a different iteration count.
        assert len(diverged) <= 6, diverged
        for d in diverged:
            assert d[3] == d[4] and d[7] <= 2 and abs(d[5] - d[6]) <= 2, d


def test_plain_root_path_ab_over_the_same_seeds(ctx, oracle):
    """A/B, solver_polish = 0 (the plain elimination + root path): the same 126 runs are identical to the CPU path's as well -- the safeguard
    decides nothing at the level of a RANSAC run on these seeds; what it does decide is measured per model (tools/polish_default_ab.py,
    tests/test_gpu_baseline_configs.py)."""
    with options(ctx, solver_polish=0):
        for n, scene_seed, seed in CASES:
            p1, p2, R, t, truth, th = synth.pose_scene(n, 0.5, seed=scene_seed)
            o = oracle.ransac_essential(p1, p2, th, confidence=0.999, max_iters=1000, lesqu=False, seed=seed)
            g = pose.ransac_essential(p1, p2, th, confidence=0.999, max_iters=1000, refit=False, seed=seed, ctx=ctx)
            assert g["iters"] == o["iters"] and g["n_inliers"] == o["n_inliers"] and np.array_equal(g["mask"], o["mask"]), (n, scene_seed, seed)
            assert e_dist(g["E"], o["E"]) < 1e-7


def test_refit_mask_flips_are_correspondences_at_the_threshold(ctx, oracle):
    """Where a refit run's mask differs from the CPU path's, the flipped correspondences sit within 1e-9 (relative) of the threshold under
    either model: named, printed."""
    found = 0
    for i in range(40):
        p1, p2, R, t, truth, th = synth.pose_scene(3000, 0.5, seed=4000 + i)
        o = oracle.ransac_essential(p1, p2, th, confidence=0.999, max_iters=1000, lesqu=True, seed=70 + i)
        g = pose.ransac_essential(p1, p2, th, confidence=0.999, max_iters=1000, refit=True, seed=70 + i, ctx=ctx)   # default options
        assert g["iters"] == o["iters"]
        idx = np.nonzero(g["mask"] != o["mask"])[0]
        assert len(idx) <= 2
        for j in idx:
            found += 1
            errs = [oracle.sampson_err(p1[j:j + 1], p2[j:j + 1], E)[0] for E in (o["E"], g["E"])]
            rel = [abs(float(e) - th * th) / (th * th) for e in errs]
            print("scene %d: correspondence %d flips; Sampson error / threshold^2 - 1 = %.2e (CPU model), %.2e (device model)" % (4000 + i, j, rel[0], rel[1]))
            assert min(rel) < 1e-6, (i, j, rel)
    print("flipped correspondences over 40 refit runs:", found)


def test_non_integer_float_descriptors_c4_size(ctx, oracle):
    """C4-size (4096 x 4096 x 128) RootSIFT-like descriptors -- L1-normalised, square-rooted: not integer-valued, so the exact fp32 kernel
    serves them -- through getMatches("LINEAR"): the match list of cvflann's L2<float> order, bit-exact."""
    import matchinglib_poselib_amd as mpa

    q, t = synth.sift_pair(4096, 4096, seed=20260104)
    root = lambda d: np.sqrt(d / np.maximum(d.sum(axis=1, keepdims=True), 1e-12)).astype(np.float32)  # noqa: E731
    q, t = root(q), root(t)
    assert not np.array_equal(q, np.rint(q))
    err, m = mpa.getMatches([None] * 4096, [None] * 4096, q, t, matcher_name="LINEAR", ctx=ctx)
    rc, o = oracle.get_matches_linear(4096, 4096, q, t)
    assert err == rc == 0 and len(m) > 1000
    assert m.tobytes() == o.tobytes()
