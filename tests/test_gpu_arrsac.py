"""GPU parity tests for ARRSAC (estimateEssentialMat's default method): the device batches + host control flow of
mlpl_arrsac_essential against the sequential CPU restatement (oracle/arrsac_oracle.cpp)."""
import numpy as np
import pytest

from matchinglib_poselib_amd import pose, synth
from option_guard import options

pytestmark = pytest.mark.gpu


def e_dist(a, b):
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


SCENES = [(5000, 0.5, 20260103), (5000, 0.3, 20260104), (5000, 0.8, 20260105), (2000, 0.95, 20260106), (300, 0.6, 20260107),
          (80, 0.7, 20260108), (150, 0.5, 20260109), (1000, 0.9, 20260110), (5000, 0.15, 20260111), (8192, 0.4, 20260112)]


@pytest.mark.parametrize("polish", [0, 1])
@pytest.mark.parametrize("n,frac,seed", SCENES)
def test_arrsac_equals_the_sequential_oracle(ctx, oracle, n, frac, seed, polish):
    p1, p2, R, t, truth, th = synth.pose_scene(n, frac, seed=seed)
    with options(ctx, solver_polish=polish):
        for refine in (False, True):
            st_g = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
            g = pose.arrsac_essential(p1, p2, th, refine=refine, rng_state=st_g, ctx=ctx)
            o = oracle.arrsac_essential(p1, p2, th, refine=refine)
            assert g["ok"] == o["ok"], (g["stats"], o["stats"])
            # the control flow took the same turns: same sample counts, same stage ends, same stream positions
            assert g["stats"][:8].tolist() == o["stats"].tolist(), (g["stats"], o["stats"])
            assert st_g.tolist() == o["rng_state"].tolist()
            assert g["n_inliers"] == o["n_inliers"]
            if g["n_inliers"]:
                assert np.array_equal(g["mask"], o["mask"])
            if g["ok"]:
                assert e_dist(g["E"], o["E"]) < 1e-7, e_dist(g["E"], o["E"])   # with and without the solver's safeguard


@pytest.mark.parametrize("polish", [1, 0])
def test_arrsac_fixture_on_the_device(ctx, polish):
    """The committed oracle fixture (tests/golden/arrsac_trace.npz): result, statistics, stream positions and the first 60 turns."""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "arrsac_trace.npz"))
    with options(ctx, solver_polish=polish):
        for ci in range(len(g["cases"])):
            buf = np.zeros(20 * 4000, np.int32)
            ctx.lib.mlpl_debug_arrsac_trace(ctx.handle, buf.ctypes.data, len(buf))
            st = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
            r = pose.arrsac_essential(g[f"c{ci}_p1"], g[f"c{ci}_p2"], float(g[f"c{ci}_th"][0]), refine=True, rng_state=st, ctx=ctx)
            ln = ctx.lib.mlpl_debug_arrsac_trace(ctx.handle, None, 0)
            assert r["ok"] == bool(g[f"c{ci}_ok"][0]) and np.array_equal(r["stats"][:8], g[f"c{ci}_stats"])
            assert np.array_equal(st, g[f"c{ci}_rng"]) and np.array_equal(np.packbits(r["mask"]), g[f"c{ci}_mask"])
            assert e_dist(r["E"], g[f"c{ci}_E"]) < 1e-7
            assert np.array_equal(buf[:ln].reshape(-1, 20)[:60], g[f"c{ci}_turns"])


@pytest.mark.parametrize("polish", [1, 0])
def test_arrsac_streams_carry_over_and_default_method(ctx, oracle, polish):
    """Second call of a process = the reference's second call (static cv::RNGs); estimateEssentialMat's default method is ARRSAC."""
    p1, p2, R, t, truth, th = synth.pose_scene(1500, 0.5, seed=6)
    with options(ctx, solver_polish=polish):
        st_g, st_o = np.array(pose.ARRSAC_RNG_FRESH, np.uint64), np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
        for call in range(3):
            g = pose.arrsac_essential(p1, p2, th, refine=False, rng_state=st_g, ctx=ctx)
            o = oracle.arrsac_essential(p1, p2, th, refine=False, rng_state=st_o)
            assert g["ok"] == o["ok"] and np.array_equal(st_g, st_o) and g["stats"][:8].tolist() == o["stats"].tolist(), call
            assert np.array_equal(g["mask"], o["mask"])
        pose._arrsac_rng_state[:] = pose.ARRSAC_RNG_FRESH
        ok, E, mask = pose.estimateEssentialMat(p1, p2, threshold=th, refine=True, ctx=ctx)
        o = oracle.arrsac_essential(p1, p2, th, refine=True)
        assert ok and o["ok"] and np.array_equal(mask, o["mask"]) and e_dist(E, o["E"]) < 1e-7
        assert np.array_equal(pose._arrsac_rng_state, o["rng_state"])


@pytest.mark.parametrize("polish", [1, 0])
def test_arrsac_generation_in_the_preemptive_stage(ctx, oracle, polish):
    """Scenes whose first block is almost all inliers make the preemptive stage generate more hypotheses (uniform sampler over ALL
    correspondences, sequential test over the first i+1): large device batches, scores that double-count, the n == 1 exit."""
    hit = 0
    with options(ctx, solver_polish=polish):
        for seed in range(40, 60):
            p1, p2, R, t, truth, th = synth.pose_scene(1200, 0.97, seed=seed)
            o = oracle.arrsac_essential(p1, p2, th, refine=False)
            if o["stats"][5] == 0:
                continue
            hit += 1
            st = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
            g = pose.arrsac_essential(p1, p2, th, refine=False, rng_state=st, ctx=ctx)
            assert g["ok"] == o["ok"] and g["stats"][:8].tolist() == o["stats"].tolist() and np.array_equal(st, o["rng_state"])
            assert np.array_equal(g["mask"], o["mask"])
            if hit == 4:
                break
        assert hit >= 1, "no scene reached the generation branch"


def test_arrsac_bad_arguments_and_failure(ctx):
    p1, p2, R, t, truth, th = synth.pose_scene(300, 0.5, seed=8)
    from matchinglib_poselib_amd._lib import MlplError
    with pytest.raises(MlplError):
        pose.arrsac_essential(p1[:5], p2[:5], th, ctx=ctx)                # runARRSAC is never reached with 5 correspondences
    with pytest.raises(MlplError):
        pose.arrsac_essential(p1, p2, 0.0, ctx=ctx)
    rng = np.random.default_rng(0)                                         # pure noise: a winner with too few inliers -> not ok
    r = pose.arrsac_essential(rng.uniform(-0.4, 0.4, (400, 2)), rng.uniform(-0.4, 0.4, (400, 2)), th, rng_state=np.array(pose.ARRSAC_RNG_FRESH, np.uint64), ctx=ctx)
    assert not r["ok"]


@pytest.mark.parametrize("polish", [0, 1])
def test_arrsac_forty_scenes_on_one_stream_pair(ctx, oracle, polish):
    """One process-like run: 40 random scenes (60-4000 correspondences, 20-100 % inliers, three noise levels) through ONE pair of
    streams.  Results (ok, mask, stream positions, stage ends) must agree on every scene.  The hypothesis COUNT of the first stage may
    differ by one or two on the rare sample whose 5-point system is ill conditioned: there the CPU elimination returns a model off the
    essential-matrix constraints or none at all (tools/arrsac_stress_trace.py) -- a low-support hypothesis that never wins."""
    rng = np.random.default_rng(99)
    st_g = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
    st_o = st_g.copy()
    exact = 0
    with options(ctx, solver_polish=polish):
        for it in range(40):
            n = int(rng.choice([60, 99, 100, 101, 150, 250, 600, 1500, 4000]))
            frac = float(rng.choice([0.2, 0.35, 0.5, 0.7, 0.85, 0.95, 1.0]))
            noise = float(rng.choice([0.0, 0.3, 1.0]))
            p1, p2, R, t, truth, th = synth.pose_scene(n, frac, seed=1000 + it, noise_px=noise)
            g = pose.arrsac_essential(p1, p2, th, refine=bool(it & 1), rng_state=st_g, ctx=ctx)
            o = oracle.arrsac_essential(p1, p2, th, refine=bool(it & 1), rng_state=st_o)
            assert g["ok"] == o["ok"] and np.array_equal(st_g, st_o) and np.array_equal(g["mask"], o["mask"]), it
            gs, os_ = g["stats"][:8].tolist(), o["stats"].tolist()
            assert gs[2:7] == os_[2:7] and abs(gs[0] - os_[0]) <= 2 and abs(gs[1] - os_[1]) <= 2, (it, gs, os_)
            exact += gs == os_
            if g["ok"]:
                assert e_dist(g["E"], o["E"]) < 1e-7, it
        assert exact >= 36, exact


def test_arrsac_device_variant_equals_host_api(ctx):
    import torch
    p1, p2, R, t, truth, th = synth.pose_scene(2500, 0.45, seed=77)
    a = pose.arrsac_essential(p1, p2, th, refine=True, rng_state=np.array(pose.ARRSAC_RNG_FRESH, np.uint64), ctx=ctx)
    st = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
        b = pose.arrsac_essential_device(d1, d2, th, refine=True, rng_state=st, ctx=ctx)
    stream.synchronize()
    assert a["ok"] and b["ok"] and a["n_inliers"] == b["n_inliers"] and np.array_equal(a["E"], b["E"])
    assert np.array_equal(b["mask"].cpu().numpy(), a["mask"])


@pytest.mark.parametrize("n", [6, 7, 8, 10, 14, 20, 37])
@pytest.mark.parametrize("polish", [1, 0])
def test_arrsac_tiny_inputs(ctx, oracle, n, polish):
    """Fewer correspondences than one block: the first stage alone decides (arrsac.h:388-401); the result fails the final
    plausibility test below 15 inliers (modelest.cpp:275-278) -- both sides must say so alike."""
    p1, p2, R, t, truth, th = synth.pose_scene(n, 0.9, seed=500 + n)
    with options(ctx, solver_polish=polish):
        st = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
        g = pose.arrsac_essential(p1, p2, th, refine=True, rng_state=st, ctx=ctx)
        o = oracle.arrsac_essential(p1, p2, th, refine=True)
        assert g["ok"] == o["ok"] and g["n_inliers"] == o["n_inliers"] and np.array_equal(st, o["rng_state"])
        assert g["stats"][:8].tolist() == o["stats"].tolist()
        if g["n_inliers"]:
            assert np.array_equal(g["mask"], o["mask"])
        if g["ok"]:
            assert e_dist(g["E"], o["E"]) < 1e-7


def test_robust_essential_refine_on_the_device(ctx, oracle):
    """poselib::robustEssentialRefine (pose_estim.cpp:337-792): rounds, result and the < 50 points rule against the CPU restatement."""
    p1, p2, R, t, truth, th = synth.pose_scene(3000, 0.6, seed=71)
    o = oracle.ransac_essential(p1, p2, th, confidence=0.999, max_iters=300, lesqu=False, seed=5)
    mask = o["mask"]
    sel = mask.astype(bool)
    for scale in (50.0, 10.0, 2.0):
        it_o, E_o, err = oracle.robust_essential_refine(p1[sel], p2[sel], o["E"], th / scale)
        E_g, it_g, status = pose.robust_essential_refine(p1, p2, o["E"], th / scale, mask=mask, ctx=ctx)
        assert status == 0 and it_g == it_o and e_dist(E_g, E_o) < 1e-9, (scale, it_g, it_o, e_dist(E_g, E_o))
        s = np.linalg.svd(E_g, compute_uv=False)
        assert s[2] < 1e-12 * s[0]
    E_g, it_g, status = pose.robust_essential_refine(p1[:40], p2[:40], o["E"], th / 10, ctx=ctx)      # too few points: returned as is
    assert status == 2 and np.array_equal(E_g, o["E"])


def _cubic_residual(E):
    E = E / np.linalg.norm(E)
    return max(np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max(), abs(np.linalg.det(E)))


@pytest.mark.parametrize("polish", [1, 0])
def test_arrsac_estimators_on_single_samples(ctx, oracle, polish):
    """The estimators ARRSAC's inner RANSAC uses, sample by sample: the 5-point solver on 6 and 7 correspondences (cv::SVD's four last
    right singular vectors of an m x 9 system there, the Gram matrix's four smallest eigenvectors here) and the 8-point fit on 8..14.
    Every oracle solution that IS an essential matrix (cubic constraints to 1e-9) must be reproduced; where the CPU elimination is ill
    conditioned its solutions are off the constraints by up to 1e-2 (tools/arrsac_sample_check.py 600 0.7 1436 0 1.0 9,2,28,3,65,94)
    while the device's stay on them -- those are counted, not compared."""
    p1, p2, R, t, truth, th = synth.pose_scene(400, 0.8, seed=91, noise_px=1.0)
    rng = np.random.default_rng(7)
    with options(ctx, solver_polish=polish):
        compared = off = 0
        for trial in range(60):
            m = 6 + (trial & 1)
            idx = rng.choice(100, m, replace=False).astype(np.int32)
            Eg, vg = pose.arrsac_sample_models(p1, p2, idx, 0, ctx=ctx)
            Eo = [np.asarray(e).reshape(3, 3) for e in oracle.run5point(p1[idx], p2[idx])]
            A = np.array([[a[0] * b[0], a[1] * b[0], b[0], a[0] * b[1], a[1] * b[1], b[1], a[0], a[1], 1.0] for a, b in zip(p1[idx], p2[idx])])
            N = np.linalg.svd(A)[2][-4:].T
            for e in Eg:   # every device model lies in the reference's subspace and on the constraints
                v = e.reshape(9) / np.linalg.norm(e)
                assert np.linalg.norm(v - N @ (N.T @ v)) < 1e-9 and _cubic_residual(e) < 1e-6
            for e in Eo:
                if _cubic_residual(e) > 1e-9:
                    off += 1
                    continue
                compared += 1
                j = int(np.argmin([e_dist(e, x) for x in Eg]))
                assert e_dist(e, Eg[j]) < 1e-6, (trial, e_dist(e, Eg[j]))
                s = 1.0 if np.abs(e / np.linalg.norm(e) - Eg[j] / np.linalg.norm(Eg[j])).max() < 1e-6 else -1.0
                assert vg[j] == oracle.valid_model(p1[idx], p2[idx], s * e), trial      # same verdict for the same signed matrix
        assert compared > 100, (compared, off)
        for m in range(8, 15):
            for trial in range(6):
                idx = rng.choice(100, m, replace=False).astype(np.int32)
                Eg, vg = pose.arrsac_sample_models(p1, p2, idx, 1, ctx=ctx)
                ok, F = oracle.cv_fm_8point(p1[idx], p2[idx])
                assert ok and len(Eg) == 1 and np.abs(Eg[0] - F).max() < 1e-8 * np.abs(F).max(), (m, trial)
                assert vg[0] == oracle.valid_model(p1[idx], p2[idx], F)


def test_arrsac_preemptive_stage_past_the_up_front_rows(ctx, oracle):
    """Inlier ratios above ~0.9: the preemptive stage takes its GENERATION branch (k grows, nothing halves) and can walk past the 1024
    correspondences every hypothesis is tested on up front (the reference keeps going there); the survivors' remaining bits are then
    computed on demand (arrsac_extend_kernel).  Scenes that get past 1024 are rare (none in 1500 tried: the longest stage ended at 819),
    so the test lowers the up-front row length to 256 and 128 (option arrsac_flag_points) on scenes whose stage ends at 419..819:
    statistics (stats[6] = where the stage ended), stream positions, inlier counts and masks equal to the oracle's, refinement on and off."""
    past = 0
    for frac, noise, seed in ((0.9808375976373475, 0.3, 1218), (0.9937940121440533, 0.3, 1743), (0.9953357108295809, 0.01, 3073),
                              (0.9948514566031564, 0.05, 3193), (0.9881629620106517, 1.5, 1010), (0.9942391333394867, 0.02, 3152)):
        p1, p2, R, t, truth, th = synth.pose_scene(2500, frac, seed=seed, noise_px=noise)
        for refine in (False, True):
            o = oracle.arrsac_essential(p1, p2, th, refine=refine)
            for fp in (256, 128, 0):
                with options(ctx, arrsac_flag_points=fp):
                    st_g = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
                    g = pose.arrsac_essential(p1, p2, th, refine=refine, rng_state=st_g, ctx=ctx)
                    assert g["ok"] == o["ok"] and g["stats"][:8].tolist() == o["stats"].tolist(), (frac, noise, fp, g["stats"], o["stats"])
                    assert st_g.tolist() == o["rng_state"].tolist() and g["n_inliers"] == o["n_inliers"] and np.array_equal(g["mask"], o["mask"])
            past += int(o["stats"][6] >= 256)
    assert past >= 8, past      # the scenes do run past the shortened rows
