"""StereoRefine with the linear refinement solvers -- after the robust estimation (refineMethod, kneipInsteadBA) and on the correspondence
pool between robust estimations (refineMethod_CorrPool, kneipInsteadBA_CorrPool, checkPoolPoseRobust != 1): the C++ drop-in
(tests/cpp/stereo_refine_linear_driver.cpp) against the CPU restatement (tests/stereo_refine_linear_oracle.py), frame by frame, with the
frame generator, the poses and the rules of tests/test_gpu_stereo_refine.py."""
import os
import subprocess

import numpy as np
import pytest

from stereo_refine_linear_oracle import LinearCfg, StereoRefineLinearOracle
from test_gpu_stereo_refine import IMG_SIZE, K, POSE_A, POSE_B, constraint_residual, drifted, frame, same_up_to_sign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "stereo_refine_linear_driver")

DRIFT = [(450, "A", 0.2)] * 2 + [(450, 1.5 * k, 0.2) for k in range(1, 9)] + [(450, 12.0, 0.2)] * 2

# name -> (rng seed, configuration, frames as (count, pose, outlier fraction)); `want` = (branch, pose source) pairs the sequence must reach
SEQUENCES = {
    # the struct's defaults: the pool pose refined with Stewenius + pseudo-Huber weights between robust estimations
    "pool_stewenius": dict(seed=21, cfg=dict(checkPoolPoseRobust=3, refineMethod_CorrPool=0x23), frames=[(400, "A", 0.2)] * 12,
                           want=[("pool+refined", 1), ("pool+robust", 1)]),
    # the harness' value: Kneip's eigensolver from the last pose, then triangPts3D with the pose it returns
    "pool_kneip": dict(seed=22, cfg=dict(checkPoolPoseRobust=3, refineMethod_CorrPool=0x24), frames=[(400, "A", 0.2)] * 12,
                       want=[("pool+refined", 2), ("pool+robust", 1)]),
    "pool_8pt_torr": dict(seed=23, cfg=dict(checkPoolPoseRobust=3, refineMethod_CorrPool=0x11), frames=[(400, "A", 0.2)] * 10,
                          want=[("pool+refined", 1)]),
    "post_stewenius": dict(seed=24, cfg=dict(checkPoolPoseRobust=1, refineMethod=0x23), frames=[(450, "A", 0.25)] * 5, want=[("init", 1), ("pool", 1)]),
    # R passed empty: the 12 perturbed starts drawn from the run's seed
    "post_kneip": dict(seed=25, cfg=dict(checkPoolPoseRobust=1, refineMethod=0x24), frames=[(450, "A", 0.25)] * 5, want=[("init", 2), ("pool", 2)]),
    "kneip_instead_of_ba": dict(seed=26, cfg=dict(checkPoolPoseRobust=3, kneipInsteadBA=True, kneipInsteadBA_CorrPool=True),
                                frames=[(400, "A", 0.2)] * 8, want=[("init", 4), ("pool+refined", 4)]),
    # the pose drifts away from the identity the pool was started near: Kneip's solver, started from the last rotation, loses more than
    # 15 % of the pool at its first step -> refineEssentialLinear returns false, twice in a row
    "drift_fails_the_refinement": dict(seed=33, cfg=dict(checkPoolPoseRobust=3, refineMethod_CorrPool=0x24, relInlRatThLast=0.6), frames=DRIFT, want=[]),
    # the same drift with Kneip's solver in the place of bundle adjustment: its failure path, whose fallback refinement (Stewenius with
    # pseudo-Huber weights) SUCCEEDS and therefore -- the reference's inverted test -- ends the refinement with -1
    "kneip_instead_of_ba_fails_on_the_pool": dict(seed=33, cfg=dict(checkPoolPoseRobust=3, kneipInsteadBA_CorrPool=True, relInlRatThLast=0.6),
                                                  frames=DRIFT, want=[]),
    # ... and after the robust estimation: robustPoseEstimation returns -1 and leaves refineMethod at the fallback's value, so that every
    # later estimation fails the same way
    "kneip_instead_of_ba_fails_after_the_estimate": dict(seed=33, cfg=dict(checkPoolPoseRobust=3, kneipInsteadBA=True, kneipInsteadBA_CorrPool=True,
                                                                           relInlRatThLast=0.6), frames=DRIFT[:8], want=[]),
}


def sequence(name):
    spec = SEQUENCES[name]
    rng = np.random.default_rng(spec["seed"])
    cfg = LinearCfg(**spec["cfg"])
    pose = lambda p: POSE_A if p == "A" else POSE_B if p == "B" else drifted(p)  # noqa: E731
    frames = [frame(rng, n, pose(p), out) for n, p, out in spec["frames"]]
    assert len(frames) <= 12 and all(len(f[2]) <= 500 for f in frames) and cfg.RobMethod == "RANSAC"
    return cfg, frames


_oracle_runs = {}


def run_oracle(oracle, name, seed=777):
    if name in _oracle_runs:
        return _oracle_runs[name]
    cfg, frames = sequence(name)
    sr = StereoRefineLinearOracle(oracle, cfg, K, K, np.zeros(8), np.zeros(8), seed)
    sr.img_size = IMG_SIZE
    out = []
    for kp1, kp2, dd in frames:
        rc = sr.add(kp1, kp2, dd)
        out.append(dict(rc=rc, inl=sr.nr_inliers, corrs=sr.nr_corrs, pool=len(sr.pool), est=sr.nr_est, skip=sr.skip, stable=int(sr.stable),
                        ml=int(sr.ml_stable), hist=len(sr.poses), src=sr.source, branch=sr.branch,
                        E=None if sr.E is None else sr.E.copy(), R=None if sr.R is None else sr.R.copy(),
                        t=None if sr.t is None else sr.t.copy(), Eml=None if sr.E_ml is None else sr.E_ml.copy()))
    _oracle_runs[name] = (out, sr.log)
    return _oracle_runs[name]


def run_gpu(name, tmp_path, seed=777):
    cfg, frames = sequence(name)
    fin, fout = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    with open(fin, "wb") as f:
        np.array([len(frames), 0], np.int32).tofile(f)
        np.array([seed], np.uint32).tofile(f)
        K.tofile(f)
        K.tofile(f)
        np.zeros(16).tofile(f)
        cfg.as_doubles().tofile(f)
        cfg.linear_ints().tofile(f)
        for kp1, kp2, dd in frames:
            np.array([len(dd)], np.int32).tofile(f)
            kp1.tofile(f)
            kp2.tofile(f)
            dd.tofile(f)
    subprocess.run([EXE, str(fin), str(fout)], check=True, timeout=300, stdout=subprocess.DEVNULL)
    rec = np.dtype([("st", np.int32, 10), ("E", np.float64, 9), ("R", np.float64, 9), ("t", np.float64, 3), ("Eml", np.float64, 9)])
    return np.frombuffer(fout.read_bytes(), rec)


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_oracle_reaches_the_refinement_branches(oracle, name):
    """CPU only: the restated state machine takes the branches each sequence is built for."""
    out, log = run_oracle(oracle, name)
    seen = [(o["branch"], o["src"]) for o in out]
    for w in SEQUENCES[name]["want"]:
        assert w in seen, (w, seen)
    if name == "pool_kneip":      # the refinement starts from the last pose: no perturbed starts
        assert any(k == "kneip" and ok and steps >= 1 and attempts == 0 for k, ok, steps, attempts in log), log
    elif name == "post_kneip":    # R passed empty: the seeded starts
        assert all(k == "kneip" and ok and attempts >= 1 for k, ok, steps, attempts in log) and len(log) >= 5, log
    elif name == "pool_8pt_torr" or name == "pool_stewenius" or name == "post_stewenius":
        assert any(k == "linear" and ok and steps >= 1 for k, ok, steps, _ in log), log
    elif name in ("drift_fails_the_refinement", "kneip_instead_of_ba_fails_on_the_pool"):
        rcs = [o["rc"] for o in out]
        first = rcs.index(-3)
        assert seen[first][0] == "pool+refined" and ("kneip", False, 0, 0) in log, (seen, log)
        assert 0 < out[first]["pool"] == out[first - 1]["pool"] and out[first]["est"] == out[first - 1]["est"], "the new pool entries are deleted again"
        assert out[first]["skip"] == out[first - 1]["skip"] + 1 and np.array_equal(out[first]["E"], out[first - 1]["E"]), "the old pose is kept"
        assert rcs[first + 1] == -3 and out[first + 1]["pool"] == 0 and out[first + 1]["est"] == 0, "the second failure clears the pool"
        assert rcs[first + 2] == 0 and seen[first + 2][0] == "init"
        if name == "kneip_instead_of_ba_fails_on_the_pool":
            assert log.count(("kneip_ba_fallback", "refined->fail")) == 2 and ("kneip_ba_fallback", "not refined->proceed") not in log, log
            assert ("pool+refined", 4) in seen
    elif name == "kneip_instead_of_ba_fails_after_the_estimate":
        rcs = [o["rc"] for o in out]
        first = rcs.index(-1)
        assert ("init", 4) in seen and first >= 2 and all(rc == -1 for rc in rcs[first:]) and len(rcs) - first >= 2, rcs
        assert log.count(("kneip_ba_fallback", "refined->fail")) == len(rcs) - first, log


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_sequence_matches_the_cpu_state_machine(oracle, tmp_path, name):
    """Frame by frame: identical decisions and pose sources, identical counts (a drift of <= 5 only once the CPU solver's model is itself
    off the essential-matrix constraints, the rule of test_gpu_stereo_refine.py), poses within 1e-6."""
    assert os.path.exists(EXE), "run __graft_entry__.build()"
    want, _ = run_oracle(oracle, name)
    got = run_gpu(name, tmp_path)
    assert len(got) == len(want)
    cpu_off = False
    unit = lambda a: a / np.linalg.norm(a)  # noqa: E731
    for i, (g, w) in enumerate(zip(got, want)):
        st = dict(zip(["rc", "inl", "corrs", "pool", "est", "skip", "stable", "ml", "hist", "src"], g["st"].tolist()))
        if w["E"] is not None and constraint_residual(w["E"]) > 1e-9:
            cpu_off = True
        for k in ("rc", "est", "skip", "stable", "ml", "hist", "src"):
            assert st[k] == w[k], (name, i, k, st, {k: w[k] for k in st})
        for k in ("inl", "corrs", "pool"):
            assert abs(st[k] - w[k]) <= (5 if cpu_off else 0), (name, i, k, st, {k: w[k] for k in st})
        if w["E"] is not None:
            assert same_up_to_sign(unit(g["E"].reshape(3, 3)), unit(w["E"]), 1e-6), (name, i)
            assert np.abs(g["R"].reshape(3, 3) - w["R"]).max() < 1e-6 and np.abs(g["t"] - w["t"]).max() < 1e-6, (name, i)
        if w["Eml"] is not None:
            assert same_up_to_sign(unit(g["Eml"].reshape(3, 3)), unit(w["Eml"]), 1e-6), (name, i)
