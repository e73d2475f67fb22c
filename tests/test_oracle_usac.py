"""CPU tests of the USAC oracle (oracle/usac_oracle.cpp) against the REFERENCE's control flow: tests/golden/usac_trace.npz holds decision
traces of the reference's own include/usac/estimators/USAC.h + usac/utils compiled in place (oracle/_ref/usac_ref, generator
tests/golden/make_golden.py usac).  Event records: see include/mlpl_c.h (mlpl_debug_usac_trace)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import make_golden  # noqa: E402  (scene generator of the fixture)
import usac_compare  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def fixture_cases(name="usac_trace.npz"):
    g = np.load(os.path.join(GOLD, name))
    for k in range(int(g["n_cases"][0])):
        n, frac, seed, prosac, usac_seed, agree = g[f"k{k}_meta"]
        yield g, k, int(n), float(frac), int(seed), int(prosac), int(usac_seed), int(agree)


def check_against_fixture(run, g, k, n, frac, seed, prosac, usac_seed, e_tol=1e-8, e5_max=1e-8, kept=make_golden.USAC_EVENTS_KEPT):
    """run(p1, p2, th, usac_seed, sorted_idx, event_cap) -> dict(events, final, flags, E).  Asserts the reference's decisions.
    e5_max: bound on the largest difference of a MINIMAL model (the device polishes every 5-point solution on the cubic constraints; on
    the ~1 % of samples whose elimination is ill conditioned the CPU root path is off by up to 1e-5); 98 % within e_tol."""
    p1, p2, th, truth, order = make_golden.usac_scene(n, frac, seed)
    o = run(p1, p2, th, usac_seed, order if prosac else None, 200000)
    ref_ev = g[f"k{k}_events"]
    assert o["n_events"] == int(g[f"k{k}_n_events"][0])
    first, d = usac_compare.compare(ref_ev, o["events"][:kept])
    assert first is None, (k, first, ref_ev[first][:12] if first < len(ref_ev) else None, o["events"][first][:12])
    assert d.get("sprt", 0) < 1e-12 and d.get("E3", 0) < e_tol and d.get("E5_q98", 0) < e_tol and d.get("E5", 0) < e5_max, d
    assert np.array_equal(o["final"][:8], g[f"k{k}_final"][:8])          # counts: hypotheses, models, rejections, inliers, verifications, LOs
    assert np.abs(o["final"][8:] - g[f"k{k}_final"][8:]).max() < 1e-12   # SPRT delta / epsilon handed back
    assert np.array_equal(np.packbits(o["flags"]), g[f"k{k}_flags"])
    Er, Eo = g[f"k{k}_E"] / np.linalg.norm(g[f"k{k}_E"]), o["E"] / np.linalg.norm(o["E"])
    assert min(np.abs(Er - Eo).max(), np.abs(Er + Eo).max()) < e_tol


def test_fixture_is_the_intended_one():
    g = np.load(os.path.join(GOLD, "usac_trace.npz"))
    assert int(g["n_cases"][0]) == 4 * len(make_golden.USAC_CASES)
    assert np.array_equal(g["cases"], np.array(make_golden.USAC_CASES, np.float64))
    agree = [c[-1] for c in fixture_cases()]
    assert sum(agree) >= len(agree) - 2      # two cases hit ccmath's early stop (make_golden.usac_case docstring)


@pytest.mark.parametrize("half", [0, 1])
def test_oracle_follows_the_references_usac_decision_by_decision(oracle, half):
    """USAC.h's samplers, sequential tests, history, stopping rules and local optimisation, restated: every sample, every evaluation
    (start position, inliers seen, points tested, verdict, delta, epsilon, threshold), every refit and every stored model as in the
    reference-built trace."""
    cases = list(fixture_cases())
    for g, k, n, frac, seed, prosac, usac_seed, agree in cases[half::2]:
        if not agree:
            continue
        check_against_fixture(lambda p1, p2, th, s, si, cap: oracle.usac_essential(p1, p2, th, s, sorted_idx=si, event_cap=cap), g, k, n, frac,
                              seed, prosac, usac_seed)


def test_where_ccmath_stops_early_the_runs_part_at_a_refit_and_end_alike(oracle):
    """The two recorded cases: the first differing decision is the evaluation right after a refined model (record type 3) whose
    reference version (ccmath svdu1v / svduv) is not the smallest singular vector; the final inlier counts agree within 2."""
    seen = 0
    for g, k, n, frac, seed, prosac, usac_seed, agree in fixture_cases():
        if agree:
            continue
        seen += 1
        p1, p2, th, truth, order = make_golden.usac_scene(n, frac, seed)
        o = oracle.usac_essential(p1, p2, th, usac_seed, sorted_idx=order if prosac else None, event_cap=200000)
        ref_ev = g[f"k{k}_events"]
        first, _ = usac_compare.compare(ref_ev, o["events"][:len(ref_ev)])
        assert first is not None and int(ref_ev[first - 1][0]) == 3 and int(ref_ev[first][0]) == 2
        a, b = ref_ev[first - 1][5:14], o["events"][first - 1][5:14]
        a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
        assert min(np.abs(a - b).max(), np.abs(a + b).max()) > 1e-3      # a different matrix, not rounding
        assert ref_ev[first][4] < o["events"][first][4]                   # ... which explains fewer correspondences (the oracle's: more)
        assert abs(int(o["final"][5]) - int(g[f"k{k}_final"][5])) <= 2
    assert seen == 2


def test_with_the_references_own_solver_the_results_agree(oracle):
    """OpenGV's fivept_nister in the reference-built USAC (fixture `opengv_*`): unconverged roots change individual models, so traces
    part, but the estimates agree: same hypothesis count within 10 %, inlier sets equal up to a handful of correspondences."""
    for g, k, n, frac, seed, prosac, usac_seed, agree in fixture_cases():
        p1, p2, th, truth, order = make_golden.usac_scene(n, frac, seed)
        o = oracle.usac_essential(p1, p2, th, usac_seed, sorted_idx=order if prosac else None)
        gf = g[f"k{k}_opengv_final"]
        flags = np.unpackbits(g[f"k{k}_opengv_flags"])[:n]
        assert abs(o["final"][1] - gf[1]) <= max(2, 0.1 * gf[1]), (k, o["final"][1], gf[1])
        assert np.count_nonzero(flags != o["flags"]) <= max(3, 0.01 * n), (k, np.count_nonzero(flags != o["flags"]))


def stewenius_run(f):
    """POSE_STEWENIUS as estimateEssentialMatUsac configures it on a process' first call: mS = 6, tM = 2736 (usac_estimations.cpp:323, 412, 422)."""
    return lambda p1, p2, th, s, si, cap: f(p1, p2, th, s, sorted_idx=si, event_cap=cap, sprt_ms=6.0, sprt_tm=2736.0)


def test_oracle_follows_the_reference_running_its_default_stewenius_solver(oracle):
    """tests/golden/usac_stewenius_trace.npz: the reference-built USAC.h with the reference's DEFAULT estimator, OpenGV's
    fivept_stewenius (`usac_ref --stewenius`) -- the reference's own solver, nothing swapped in.  The oracle's five-point solver gives the
    same real solutions (98 % of the minimal models within 1e-8; the ill-conditioned samples up to 5e-3) and the run takes the same
    decisions, event by event, in 21 of the 24 runs."""
    g0 = np.load(os.path.join(GOLD, "usac_stewenius_trace.npz"))
    assert np.array_equal(g0["cases"], np.array(make_golden.USAC_STEWENIUS_CASES, np.float64))
    cases = list(fixture_cases("usac_stewenius_trace.npz"))
    assert len(cases) == 4 * len(make_golden.USAC_STEWENIUS_CASES) and sum(c[-1] for c in cases) >= len(cases) - 3
    for g, k, n, frac, seed, prosac, usac_seed, agree in cases:
        if agree:
            check_against_fixture(stewenius_run(oracle.usac_essential), g, k, n, frac, seed, prosac, usac_seed, e5_max=5e-3,
                                  kept=make_golden.USAC_STEWENIUS_EVENTS_KEPT)


def test_stewenius_runs_that_part_do_so_at_a_named_place_and_end_alike(oracle):
    """The three other runs: two part right after a refit where ccmath's svdu1v stops early (as in usac_trace.npz), one at a minimal
    sample so ill conditioned that the two solvers' models differ by 1e-5 and the oriented-constraint verdict with them.  Same estimate
    at the end: inlier counts within 1 %."""
    seen = 0
    for g, k, n, frac, seed, prosac, usac_seed, agree in fixture_cases("usac_stewenius_trace.npz"):
        if agree:
            continue
        seen += 1
        p1, p2, th, truth, order = make_golden.usac_scene(n, frac, seed)
        o = stewenius_run(oracle.usac_essential)(p1, p2, th, usac_seed, order if prosac else None, 200000)
        ref_ev = g[f"k{k}_events"]
        first, _ = usac_compare.compare(ref_ev, o["events"][:len(ref_ev)])
        if first is not None:     # inside the kept head: right after a refit
            assert int(ref_ev[first - 1][0]) == 3 and int(ref_ev[first][0]) == 2, (k, first)
        assert abs(int(o["final"][5]) - int(g[f"k{k}_final"][5])) <= max(2, 0.01 * g[f"k{k}_final"][5]), (k, o["final"][5], g[f"k{k}_final"][5])
    assert seen == 3


def test_live_against_the_reference_build(oracle):
    """oracle/_ref/usac_ref on six random scenes (PROSAC on every other one): its traces are recorded in tests/golden/ref_live.npz
    (make_golden.py ref_live); where the tool exists it runs again and must reproduce the recording."""
    import usac_ref_tool as u
    g = np.load(os.path.join(GOLD, "ref_live.npz"))
    for trial, n, frac, seed in make_golden.live_usac_trials():
        r = {k: g[f"usac{trial}_{k}"] for k in ("events", "final", "flags", "pool")}
        if u.available():
            live = make_golden.live_usac_run(trial, n, frac, seed)
            assert all(np.array_equal(live[k], r[k]) for k in r), trial
        p1, p2, th, truth, order = make_golden.usac_scene(n, frac, seed)
        si = order if trial % 2 else None
        o = oracle.usac_essential(p1, p2, th, 1000 + trial, sorted_idx=si, event_cap=200000)
        first, d = usac_compare.compare(r["events"], o["events"])
        if first is not None:   # only ever at a refit where ccmath stopped early
            assert int(r["events"][first - 1][0]) == 3
            continue
        assert np.array_equal(r["flags"], o["flags"]) and np.array_equal(r["final"][:8], o["final"][:8])
        assert np.array_equal(r["pool"][:5], np.asarray(r["pool"][:5]))


def test_too_few_correspondences(oracle):
    p1, p2, th, truth, order = make_golden.usac_scene(64, 0.8, 18)
    assert not oracle.usac_essential(p1[:4], p2[:4], th, 1)["ok"]
    assert not oracle.usac_essential(p1[:12], p2[:12], th, 1, sorted_idx=np.arange(12, dtype=np.uint32))["ok"]   # PROSAC: < 20
    assert oracle.usac_essential(p1[:12], p2[:12], th, 1)["ok"]


def refine_fixture_cases():
    g = np.load(os.path.join(GOLD, "usac_refine_trace.npz"))
    for k in range(int(g["n_cases"][0])):
        n, frac, seed, prosac, usac_seed, agree, refine = g[f"k{k}_meta"]
        yield g, k, int(n), float(frac), int(seed), int(prosac), int(usac_seed), int(agree), int(refine)


@pytest.mark.parametrize("refine", [5, 4, 7, 6])
def test_oracle_follows_the_reference_with_the_five_point_refinements(oracle, refine):
    """tests/golden/usac_refine_trace.npz: the inner refinements of the 5-point family (poselib::RefineAlg 4..7;
    EssentialMatEstimator.h:640-850, findWeights :2404-2428, weightingEssential.cpp:56-206).  ConfigUSAC's default is refine 5,
    REF_STEWENIUS_WEIGHTS, with POSE_STEWENIUS -- for 5 and 4 the fixture is the reference-built USAC.h running OpenGV's
    fivept_stewenius as minimal and as refinement solver (nothing swapped in); for 7 and 6 the control flow with the solver swapped
    (OpenGV's Nister returns unconverged roots).  The oracle takes the same decisions event by event in every run, refined models to 1e-8."""
    g0 = np.load(os.path.join(GOLD, "usac_refine_trace.npz"))
    assert np.array_equal(g0["cases"], np.array(make_golden.USAC_REFINE_CASES, np.float64))
    cases = [c for c in refine_fixture_cases() if c[-1] == refine]
    assert len(cases) == (4 if refine in (5, 7) else 2) * len(make_golden.USAC_REFINE_CASES) and all(c[-2] for c in cases)
    for g, k, n, frac, seed, prosac, usac_seed, agree, rf in cases:
        run = stewenius_run(lambda *a, **kw: oracle.usac_essential(*a, refine=rf, **kw))
        check_against_fixture(run, g, k, n, frac, seed, prosac, usac_seed, e5_max=5e-3, kept=make_golden.USAC_REFINE_EVENTS_KEPT)


def test_nister_refinement_with_the_references_own_solver_ends_alike(oracle):
    """refine 7 / 6 with OpenGV's fivept_nister (fixture `opengv_*`): individual models differ (unconverged roots), the estimates agree."""
    for g, k, n, frac, seed, prosac, usac_seed, agree, rf in refine_fixture_cases():
        if rf not in (6, 7):
            continue
        p1, p2, th, truth, order = make_golden.usac_scene(n, frac, seed)
        o = oracle.usac_essential(p1, p2, th, usac_seed, refine=rf, sorted_idx=order if prosac else None, sprt_ms=6.0, sprt_tm=2736.0)
        flags = np.unpackbits(g[f"k{k}_opengv_flags"])[:n]
        # (one fixture run of the reference's solver ends 7 % short of the inliers: 998 of 1067, an unconverged refinement model)
        assert np.count_nonzero(flags != o["flags"]) <= max(4, 0.08 * n), (k, np.count_nonzero(flags != o["flags"]))


def test_the_solver_on_scaled_rows_is_the_solver_on_the_points(oracle):
    """oracle_run5point_rows: with rows x2 (x) x1 of homogeneous points it is oracle_run5point; scaling a row of a minimal (exactly
    solvable) system changes nothing; for more than five rows the weights matter."""
    import ctypes as C
    rng = np.random.default_rng(5)
    p1, p2, th, truth, order = make_golden.usac_scene(64, 1.0, 3)
    lib = oracle.lib
    lib.oracle_run5point_rows.restype = C.c_int
    lib.oracle_run5point_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

    def rows_of(idx, w=None):
        a = np.concatenate([p1[idx], np.ones((len(idx), 1))], 1)
        b = np.concatenate([p2[idx], np.ones((len(idx), 1))], 1)
        r = (b[:, :, None] * a[:, None, :]).reshape(len(idx), 9)
        return np.ascontiguousarray(r if w is None else r * w[:, None])

    def solve_rows(r):
        out = np.zeros(90)
        ns = lib.oracle_run5point_rows(r.ctypes.data, len(r), out.ctypes.data)
        return out[:9 * ns].reshape(ns, 9)

    def same(A, B, tol):
        if len(A) != len(B):
            return False
        return all(min(min(np.abs(a - b).max(), np.abs(a + b).max()) for b in B) < tol for a in A)

    idx = rng.choice(64, 5, replace=False)
    E0 = oracle.run5point(p1[idx], p2[idx]).reshape(-1, 9)
    assert len(E0) > 0 and same(E0, solve_rows(rows_of(idx)), 1e-12)
    assert same(E0, solve_rows(rows_of(idx, rng.uniform(0.2, 3.0, 5))), 1e-8)
    idx = rng.choice(64, 12, replace=False)
    p1[idx] += rng.normal(0, 1e-3, (12, 2))
    A, B = solve_rows(rows_of(idx)), solve_rows(rows_of(idx, rng.uniform(0.2, 3.0, 12)))
    assert len(A) > 0 and not same(A, B, 1e-9)
