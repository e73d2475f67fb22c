"""CPU checks of the refineEssentialLinear restatement (linear_refine_oracle.py) and of the library's exported symbols."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import linear_refine_oracle as LRO
import oracle_lib

SYMBOLS = ("mlpl_refine_essential_linear", "mlpl_refine_essential_linear_batch_dev", "mlpl_recover_pose_batch_dev")


def _true_E(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return E / np.linalg.norm(E)


def _close_up_to_sign(A, B, tol):
    a = np.asarray(A).reshape(9) / np.linalg.norm(A)
    b = np.asarray(B).reshape(9) / np.linalg.norm(B)
    return min(np.abs(a - b).max(), np.abs(a + b).max()) <= tol


def test_library_exports_symbols():
    import ctypes as C

    import matchinglib_poselib_amd as mpa

    lib = C.CDLL(mpa._lib.library_path())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert all(name in mpa._lib._SIGNATURES for name in SYMBOLS)


@pytest.mark.parametrize("method", [s | w for s in (0x1, 0x2, 0x3) for w in (0x10, 0x20, 0x30)])
def test_noise_free_recovers_true_E(method):
    from matchinglib_poselib_amd import synth

    ora = oracle_lib.load()
    p1, p2, R, t, _, th = synth.pose_scene(600, 0.7, seed=3, noise_px=0.0)
    r = ora.ransac_essential(p1, p2, th, seed=5)
    # start from a perturbed model so that every refit has work to do (and pseudo-Huber weights do not vanish)
    E0 = r["E"] + 1e-4 * np.random.default_rng(1).normal(size=(3, 3))
    o = LRO.refine_essential_linear(p1, p2, E0, r["mask"], method, th=th)
    assert o["rc"] == 0 and o["steps_done"] >= 1
    assert _close_up_to_sign(o["E"], _true_E(R, t), 1e-9)
    assert o["n_inliers"] == 420


def _scene(n=1500, frac=0.6, seed=21):
    from matchinglib_poselib_amd import synth

    p1, p2, _, _, _, th = synth.pose_scene(n, frac, seed=seed, noise_px=0.3)
    r = oracle_lib.load().ransac_essential(p1, p2, th, seed=2)
    return p1, p2, r["E"], r["mask"], th


def test_control_flow():
    p1, p2, E0, m0, th = _scene()
    few = np.zeros_like(m0)
    few[np.flatnonzero(m0)[:5]] = 1
    o = LRO.refine_essential_linear(p1, p2, E0, few, 0x21, th=th)
    assert o["rc"] == LRO.MLPL_E_FAILED and o["mask"].tobytes() == few.tobytes()
    o = LRO.refine_essential_linear(p1, p2, E0, np.ones_like(m0), 0x21, th=th)   # the first step loses more than 15 %
    assert o["rc"] == LRO.MLPL_E_FAILED
    for method, steps in [(0x21, 0), (0x00, 4), (0x05, 4), (0x35, 4)]:
        o = LRO.refine_essential_linear(p1, p2, E0, m0 * 3, method, th=th, steps=steps)
        assert o["rc"] == 0 and o["steps_done"] == 0 and np.array_equal(o["E"], E0)
        assert o["mask"].tobytes() == (m0 != 0).astype(np.uint8).tobytes()
    assert LRO.refine_essential_linear(p1, p2, E0, m0, 0x24, th=th)["rc"] == LRO.MLPL_E_UNSUPPORTED
    assert LRO.refine_essential_linear(p1, p2, E0, m0, 0x04, th=th)["rc"] == LRO.MLPL_E_UNSUPPORTED


def test_weight_bits():
    p1, p2, E0, m0, th = _scene()
    for w in (0x00, 0x40):
        assert LRO.refine_essential_linear(p1, p2, E0, m0, 0x1 | w, th=th)["rc"] == LRO.MLPL_E_BAD_INPUT
        for solver in (0x2, 0x3):
            a = LRO.refine_essential_linear(p1, p2, E0, m0, solver | w, th=th)
            b = LRO.refine_essential_linear(p1, p2, E0, m0, solver | 0x30, th=th)
            assert a["rc"] == b["rc"] == 0 and np.array_equal(a["E"], b["E"]) and np.array_equal(a["mask"], b["mask"])


@pytest.mark.ref
def test_plain_nister_refit_matches_opengv():
    """The plain PR_NISTER refit's solution set (OpenGV fivept_nister on all listed points) against the reference's own OpenGV.  On some
    systems OpenGV's Sturm bracketing leaves a root unconverged (1e-7 .. 1e-5; the exact-solver deviation DESIGN 8 records for USAC),
    so the pin uses a system where all of its roots converge."""
    exe = oracle_lib.ref_tool("opengv_5pt")
    if exe is None:
        pytest.skip("oracle/_ref/opengv_5pt is built only where the reference sources exist")
    p1, p2, _, m0, _ = _scene(n=800, frac=0.6, seed=6)
    idx = np.flatnonzero(m0)[:200]
    sols = LRO.run5point_rows(LRO.rows(LRO.bearing(p1[idx]), LRO.bearing(p2[idx])))
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        pts = np.concatenate([p1[idx], p2[idx]], axis=1)
        with open(src, "wb") as f:
            f.write(struct.pack("<ii", 1, len(idx)) + np.ascontiguousarray(pts).tobytes())
        subprocess.run([exe, src, dst], check=True, timeout=120)
        raw = open(dst, "rb").read()
    cnt = struct.unpack_from("<i", raw, 0)[0]
    ref = np.frombuffer(raw, np.float64, 90, 4).reshape(10, 3, 3)[:cnt]
    assert cnt == len(sols) >= 1
    for E in sols:
        assert any(_close_up_to_sign(E, R, 1e-8) for R in ref)


# ---- the edge scenes (linear_refine_scenes.py): the restatement's trace shows what each scene is there for, and each is decidable ----
import linear_refine_scenes as LRS  # noqa: E402


def test_trace_records():
    p1, p2, E0, m0, th = _scene()
    o = LRO.refine_essential_linear(p1, p2, E0, m0, 0x22, th=th)
    assert o["rc"] == 0 and len(o["trace"]) == 4 and o["end"] == "steps" and o["trace"][-1]["end"] == "steps"
    for t in o["trace"]:
        assert t["verdict"] == "accepted" and t["wn"] > 0 and t["n_sols"] >= 1 and 0 <= t["chosen"] < t["n_sols"]
        assert (t["exit"] is None) == (t["n_sols"] == 1)
    assert [t["n_list"] for t in o["trace"][1:]] == [t["count"] for t in o["trace"][:-1]] and o["n_inliers"] == o["trace"][-1]["count"]
    o8 = LRO.refine_essential_linear(p1, p2, E0, m0, 0x31, th=th)
    assert all(t["n_sols"] == 1 and t["exit"] is None and t["wn"] is None for t in o8["trace"])
    rej = LRO.refine_essential_linear(p1, p2, E0, np.ones_like(m0), 0x21, th=th)
    assert rej["rc"] == LRO.MLPL_E_FAILED and rej["end"] == "rejected" and rej["trace"][0]["verdict"] == "rejected" and len(rej["trace"]) == 1
    none = LRO.refine_essential_linear(p1, p2, E0, m0, 0x05, th=th)
    assert none["end"] == "no fit: solver" and none["trace"][0]["n_sols"] is None
    assert LRO.refine_essential_linear(p1, p2, E0, m0, 0x21, th=th, steps=0)["trace"] == []


def test_choice_is_the_reference_loop():
    """pick_trace against the loop as the reference writes it (sums, the test at i > 3 and i % 4 == 0, break), on an ordered scene."""
    s = LRS.scene("exit68")
    t = LRS.expected("exit68")["trace"][0]
    errs = t["errs"]
    sums, at = np.zeros(errs.shape[0]), -1
    for i in range(errs.shape[1]):
        sums += errs[:, i]
        if i > 3 and i % 4 == 0 and np.sort(sums)[0] < 0.66 * np.sort(sums)[1]:
            at = i
            break
    assert at == t["exit"] == 68 and int(np.argmin(sums)) == t["chosen"] and t["fires"][0] == (68, t["chosen"])
    assert s["mask"].sum() == errs.shape[1]


def test_equal_sums_follow_a_nudge():
    """Two copies of one solution's errors: the sums tie and a relative 1e-8 decides the index -- the kind of choice stable() is there to
    refuse.  Built on the choice alone: the five-point solver returns no duplicates."""
    s = LRS.scene("none64")
    at = np.flatnonzero(s["mask"])
    f, fp = LRO.bearing(s["p1"])[at], LRO.bearing(s["p2"])[at]
    E = s["E0"] / np.linalg.norm(s["E0"])
    rng = np.random.default_rng(0)
    picks = {LRO.pick_trace([LRO._nudge(rng, E, 1e-8), LRO._nudge(rng, E, 1e-8)], f, fp)[0] for _ in range(40)}
    assert picks == {0, 1}


def _case(name, seed, **over):
    s = LRS.make(seed=seed, **{k: v for k, v in LRS.TABLE[name].items() if k != "claim"})
    kw = dict(LRS.oracle_kw(s["kw"]), th=s["th"], **over)
    return s, kw


def test_stable_refuses_a_decision_on_a_threshold():
    """The unweighted 8-point fit does not depend on th, so th can be put where the first step's threshold 1.75 th^2 lies a relative 2e-9
    above the largest error of a listed row: past the margin bar of 1e-9, and a relative 1e-8 on the model moves that row across."""
    s, kw = _case("cnt64_31", 0)
    at = np.flatnonzero(s["mask"])
    f, fp = LRO.bearing(s["p1"]), LRO.bearing(s["p2"])
    err = LRO.sampson_l2(LRO.fit_8pt(LRO.rows(f[at], fp[at])), f, fp)
    kw["th"] = float(np.sqrt(err[at].max() * (1 + 2e-9) / 1.75))
    o = LRO.refine_essential_linear(s["p1"], s["p2"], s["E0"], s["mask"], s["method"], **kw)
    assert o["rc"] == 0 and o["trace"][0]["count"] >= 64 and 1e-9 < o["margin"] < 1e-8
    assert not LRO.stable(s["p1"], s["p2"], s["E0"], s["mask"], s["method"], **kw)
    kw["th"] = s["th"]
    assert LRO.stable(s["p1"], s["p2"], s["E0"], s["mask"], s["method"], **kw)


def test_stable_refuses_a_model_the_restatement_does_not_reproduce():
    """`loss_mid_plane` at a seed the search passed over: every decision survives the 1e-8 / 1e-12 reruns, the margin is 2e-2, and the
    restatement's own E moves by more than 1e-9 when its solver's rows move by 1e-15 (the device differed from it by 7.6e-7 there)."""
    s, kw = _case("loss_mid_plane", 3)
    args = (s["p1"], s["p2"], s["E0"], s["mask"], s["method"])
    o = LRO.refine_essential_linear(*args, **kw)
    assert o["rc"] == 0 and o["margin"] > 1e-3
    rng = np.random.default_rng(0)
    assert all(LRO._decisions(LRO.refine_essential_linear(*args, _rng=rng, **kw)) == LRO._decisions(o) for _ in range(5))
    assert not LRO.stable(*args, **kw)


@pytest.mark.parametrize("name", LRS.NAMES)
def test_scene_shows_its_branch_and_is_decidable(name):
    o = LRS.expected(name)
    print(f"{name}: {LRS.TABLE[name]['why']}; rc {o['rc']} steps {o['steps_done']} end '{o['end']}' margin {o['margin']:.3g} "
          f"first step: {[(k, o['trace'][0][k]) for k in ('n_list', 'n_sols', 'exit', 'chosen', 'count', 'verdict')] if o['trace'] else None}")
    assert LRS.broken_claims(name) == []
    assert o["margin"] > LRS.MARGIN, "an error lies on a step threshold: pick another seed"
    assert LRS.is_stable(name), "a decision changes under a relative 1e-8 on the candidates / 1e-12 on the solver's rows: pick another seed"


def test_scene_set_covers_the_branches():
    first = {n: (LRS.expected(n)["trace"] or [None])[0] for n in LRS.NAMES}
    exits = {n: t["exit"] for n, t in first.items() if t is not None and t["exit"] is not None}
    reached = sorted({e for e in exits.values() if e >= 0})
    never = sorted({first[n]["n_list"] for n, e in exits.items() if e == -1})
    margins = {n: LRS.expected(n)["margin"] for n in LRS.NAMES}
    worst = min(margins, key=margins.get)
    print(f"exit positions reached: {reached}; no exit at list lengths {never}; smallest margin {margins[worst]:.3g} ({worst}); "
          f"{len(LRS.NAMES)} scenes")
    assert {4, 8, 60, 64, 68, 128} <= set(reached) and any(e >= 132 for e in reached)
    assert {64, 65, 129} <= set(never) and any(c >= 200 for c in never)
    assert all(first[n]["n_list"] <= 300 for n in exits)
    sols = {t["n_sols"] for t in first.values() if t is not None and t["n_sols"] is not None}
    assert {2, 10} <= sols
    ends = {LRS.expected(n)["end"] for n in LRS.NAMES}
    assert {"steps", "loss", "rejected", "too few", "no fit: rows", "no fit: weights"} <= ends
    assert any(LRS.expected(n)["end"] == "loss" and 0 < LRS.expected(n)["steps_done"] < 4 for n in LRS.NAMES)
    o = LRS.expected("cnt8_accept")
    assert o["rc"] == 0 and o["steps_done"] >= 1 and o["trace"][0]["n_list"] == 8 and LRS.scene("cnt8_accept")["method"] & 0xF == 1
    for c in LRS.COUNTS:
        for m in LRS.METHODS:
            assert int(np.count_nonzero(LRS.scene(f"cnt{c}_{m:02x}")["mask"])) == c
    # every listed count, and the scenes with default parameters, appear under every method (the batch tests group them by method)
    assert all(len([n for n in LRS.NAMES if LRS.TABLE[n]["method"] == m and not LRS.TABLE[n].get("kw")]) >= len(LRS.COUNTS) for m in LRS.METHODS)
