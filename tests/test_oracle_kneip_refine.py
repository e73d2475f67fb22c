"""The float64 restatement of refineEssentialLinear with PR_KNEIP (tests/kneip_refine_oracle.py): its solver against the reference's OpenGV
(tests/golden/kneip_eigensolver.npz, written by tests/golden/make_kneip_eigensolver.py) and the reference's quirks, one case each.  CPU only."""
import ctypes
import os

import numpy as np
import pytest

import kneip_refine_oracle as KRO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solver_equals_the_reference_built_eigensolver_on_every_kept_problem():
    """Every problem the generator kept (0.80 of the near-truth and 0.54 of the retry starts at 300 entries; the rest is where the
    reference's own arithmetic decides between minima): R and t / |t| within 1e-8, nothing left out."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "kneip_eigensolver.npz"))
    assert len(g["n"]) >= 400 and set(g["n"].tolist()) == {6, 64, 65, 300} and set(g["family"].tolist()) == {0, 1}
    worst = 0.0
    for s, n, R0, Rr, tr in zip(g["scene"], g["n"], g["R0"], g["R"], g["t"]):
        R, t = KRO.eigensolver(np.ascontiguousarray(g["scenes"][s]), np.arange(n, dtype=np.int32), R0)
        worst = max(worst, np.abs(R - Rr).max(), np.abs(t / np.linalg.norm(t) - tr / np.linalg.norm(tr)).max())
    assert worst < 1e-8, worst


def test_rand_restatement_equals_libc():
    libc = ctypes.CDLL("libc.so.6")
    for seed in (1, 7, 20260103, 0x80000001):
        libc.srand(ctypes.c_uint(seed))
        assert [libc.rand() for _ in range(36)] == KRO.glibc_rand(seed, 36)


@pytest.fixture(scope="module")
def scene():
    return KRO.make_scene(300, seed=41)


def _same(a, b):
    return (a["rc"] == b["rc"] and a["E"].tobytes() == b["E"].tobytes() and a["mask"].tobytes() == b["mask"].tobytes()
            and a["rt_valid"] == b["rt_valid"] and (not a["rt_valid"] or (a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes())))


def test_refines_from_a_start_rotation_and_from_none(scene):
    p1, p2, E0, m0, Rt, th = scene
    a = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x24, R=Rt, th=th)
    b = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x24, R=None, th=th, seed=3)
    for r in (a, b):
        assert r["rc"] == 0 and r["steps_done"] >= 1 and r["rt_valid"] and r["margin"] > 1e-9
        assert np.abs(r["R"] - Rt).max() < 5e-3 and abs(np.linalg.norm(r["t"]) - 1) < 1e-12
        assert r["E"].tobytes() == KRO.essential_from_pose(r["R"], r["t"]).tobytes()
        assert set(np.unique(r["mask"]).tolist()) <= {0, 1} and r["n_inliers"] == int(r["mask"].sum())
    assert a["attempts_used"] == 0 and 1 <= b["attempts_used"] <= 12
    # a passed R that is no rotation is the same as none
    c = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x24, R=2.0 * np.eye(3), th=th, seed=3)
    assert _same(b, c) and c["attempts_used"] == b["attempts_used"]


def test_weight_bits_do_not_change_a_result(scene):
    p1, p2, E0, m0, Rt, th = scene
    for R in (Rt, None):
        ref = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x04, R=R, th=th)
        for w in (0x10, 0x20, 0x30, 0x40):
            assert _same(ref, KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x04 | w, R=R, th=th))


def test_twelve_failed_attempts_return_true_with_E_unchanged_and_R_cleared():
    rng = np.random.default_rng(5)
    p1, p2 = rng.uniform(-0.4, 0.4, (200, 2)), rng.uniform(-0.4, 0.4, (200, 2))  # no geometry: no attempt keeps 85 % at th^2
    E0 = KRO.essential_from_pose(np.eye(3), [1.0, 0, 0])
    m0 = (rng.random(200) < 0.7).astype(np.uint8) * 9
    r = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x24, R=None, th=0.001)
    assert r["rc"] == 0 and r["attempts_used"] == 12 and r["steps_done"] == 0 and not r["rt_valid"] and r["R"] is None
    assert r["E"].tobytes() == E0.tobytes() and r["mask"].tobytes() == (m0 != 0).astype(np.uint8).tobytes()
    assert r["n_inliers"] == int(np.count_nonzero(m0))


def test_translation_sign_follows_the_first_list_entry(scene):
    p1, p2, E0, m0, Rt, th = scene
    pts = np.ascontiguousarray(np.concatenate([p1, p2], axis=1))
    f1, f2 = KRO.LRO.bearing(p2), KRO.LRO.bearing(p1)  # adapter view 1 = image 2
    idx = np.flatnonzero(m0)
    R, t = KRO.eigensolver(pts, idx, Rt)
    flow = f1 - f2 @ R.reshape(3, 3).T
    assert flow[idx[0]] @ t >= 0
    # the same set with another first entry whose flow opposes t: the same minimum, the translation negated
    flipped = 0
    for k in np.flatnonzero(m0 == 0):
        Ra, ta = KRO.eigensolver(pts, np.concatenate([idx, [k]]), Rt)
        Rb, tb = KRO.eigensolver(pts, np.concatenate([[k], idx]), Rt)
        fl = f1 - f2 @ Ra.reshape(3, 3).T
        assert fl[idx[0]] @ ta >= 0
        if fl[k] @ ta < 0 and np.abs(Ra - Rb).max() < 1e-6:
            assert np.abs(tb / np.linalg.norm(tb) + ta / np.linalg.norm(ta)).max() < 1e-4
            flipped += 1
    assert flipped >= 1


def test_step_zero_failure_paths(scene):
    p1, p2, E0, m0, Rt, th = scene
    few = np.zeros_like(m0)
    few[np.flatnonzero(m0)[:5]] = 1
    r = KRO.refine_essential_linear_rt(p1, p2, E0, few, 0x24, R=Rt, th=th)
    assert r["rc"] == KRO.MLPL_E_FAILED and r["mask"].tobytes() == few.tobytes() and r["E"].tobytes() == E0.tobytes()
    # every point flagged: the first step loses too many -> false, from a rotation and from the retry loop
    q1, q2, F0, _, Rq, thq = KRO.make_scene(120, seed=43, extra=1.0)
    allm = np.ones(q1.shape[0], np.uint8)
    r = KRO.refine_essential_linear_rt(q1, q2, F0, allm, 0x24, R=Rq, th=thq)
    assert r["rc"] == KRO.MLPL_E_FAILED and r["mask"].tobytes() == allm.tobytes() and r["E"].tobytes() == F0.tobytes() and r["attempts_used"] == 0
    # the solver rejects step 0 from a given rotation: the loop is left, true with E unchanged and no pose
    nan_solver = lambda pts, idx, R0: (np.full(9, np.nan), np.ones(3))  # noqa: E731
    r = KRO.refine_essential_linear_rt(p1, p2, E0, m0 * 3, 0x24, R=Rt, th=th, solver=nan_solver)
    assert r["rc"] == 0 and r["steps_done"] == 0 and not r["rt_valid"] and r["E"].tobytes() == E0.tobytes()
    assert r["mask"].tobytes() == (m0 != 0).astype(np.uint8).tobytes()
    # ... and in the retry loop all twelve times
    r = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x24, R=None, th=th, solver=nan_solver)
    assert r["rc"] == 0 and r["attempts_used"] == 12 and not r["rt_valid"] and r["E"].tobytes() == E0.tobytes()
    # a translation that is zero to 1e-3 in every component cannot come out of a normalised vector; a non-rotation is rejected
    skew_solver = lambda pts, idx, R0: (1.01 * np.eye(3).reshape(9), np.ones(3))  # noqa: E731
    r = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x24, R=Rt, th=th, solver=skew_solver)
    assert r["rc"] == 0 and r["steps_done"] == 0 and not r["rt_valid"]
    # no steps: true, the mask made 0 / 1, no pose (t_out stays zero)
    r = KRO.refine_essential_linear_rt(p1, p2, E0, m0 * 3, 0x24, R=Rt, th=th, steps=0)
    assert r["rc"] == 0 and not r["rt_valid"] and r["mask"].tobytes() == (m0 != 0).astype(np.uint8).tobytes()


def test_other_solvers_pass_through(scene):
    p1, p2, E0, m0, Rt, th = scene
    a = KRO.refine_essential_linear_rt(p1, p2, E0, m0, 0x21, R=Rt, th=th)
    b = KRO.LRO.refine_essential_linear(p1, p2, E0, m0, 0x21, th=th)
    assert a["rc"] == b["rc"] == 0 and a["E"].tobytes() == b["E"].tobytes() and not a["rt_valid"]
