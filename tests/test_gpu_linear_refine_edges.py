"""refineEssentialLinear on the MI355X over the edge scenes of linear_refine_scenes.py: list lengths on either side of 8 rows and of a 64-entry
chunk, the choice among five-point solutions with its early exit at list positions 4 .. 136 and without one, the stops of the loop, the
parameters, scaled starting models, other motions and mask patterns -- the single entry against the restatement (linear_refine_oracle.py),
the batch entry byte for byte against the single one.  test_oracle_linear_refine.py shows on the CPU that every scene reaches the branch it
is named for and is decidable (margin > 1e-9, stable())."""
import numpy as np
import pytest

import linear_refine_oracle as LRO
import linear_refine_scenes as LRS
from test_gpu_linear_refine import _single

pytestmark = pytest.mark.gpu

_diff = {}   # method -> the largest |E device - E restatement| (Frobenius-normalised, up to sign) seen by this process


def _e_diff(A, B):
    a = np.asarray(A).reshape(9) / np.linalg.norm(A)
    b = np.asarray(B).reshape(9) / np.linalg.norm(B)
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


@pytest.mark.parametrize("name", LRS.NAMES)
def test_scene_matches_restatement(ctx, name):
    s, o = LRS.scene(name), LRS.expected(name)
    g = _single(ctx, s["p1"], s["p2"], s["E0"], s["mask"], s["method"], s["th"], **s["kw"])
    assert g["ok"] == (o["rc"] == 0)
    assert g["steps_done"] == o["steps_done"] and g["n_inliers"] == o["n_inliers"]
    assert g["mask"].tobytes() == o["mask"].tobytes()
    if not g["ok"] or o["steps_done"] == 0:   # refused, or no step accepted: the model comes back as it went in
        assert g["E"].tobytes() == np.asarray(s["E0"], np.float64).tobytes()
    if not g["ok"]:
        assert g["mask"].tobytes() == s["mask"].tobytes()
        return
    d = _e_diff(g["E"], o["E"])
    _diff[s["method"]] = max(_diff.get(s["method"], 0.0), d)
    print(f"{name}: method 0x{s['method']:02x} |E - restatement| = {d:.3g}")
    assert d <= 1e-8


@pytest.fixture(scope="module", autouse=True)
def _report_differences():
    """After the module's tests: the largest difference per method among the scenes that ran (the 1e-8 bar is asserted per scene)."""
    yield
    for m in sorted(_diff):
        print(f"method 0x{m:02x}: largest |E - restatement| = {_diff[m]:.3g}")


def _batch_of(method, kw):
    """The scenes of one method with one set of parameters (a launch has one), and a problem without rows in the middle."""
    names = [n for n in LRS.NAMES if LRS.TABLE[n]["method"] == method and (LRS.TABLE[n].get("kw") or {}) == kw]
    names.insert(len(names) // 2, None)
    return names


def _check_batch(ctx, method, names, kw):
    """One launch over the scenes against the single entry, byte for byte, with NaN rows and sentinel mask bytes behind every count."""
    import torch
    from matchinglib_poselib_amd import pose

    scenes = [LRS.scene(n) if n else None for n in names]
    counts = np.array([s["p1"].shape[0] if s else 0 for s in scenes], np.int32)
    B, stride = len(names), int(counts.max()) + 9
    P1, P2 = np.full((B, stride, 2), np.nan), np.full((B, stride, 2), np.nan)   # a row read behind a count poisons the result
    M = np.full((B, stride), LRS.SENTINEL, np.uint8)
    E = np.zeros((B, 9))
    for b, s in enumerate(scenes):
        if s is None:
            E[b] = np.arange(1, 10)
            continue
        n = counts[b]
        P1[b, :n], P2[b, :n], M[b, :n], E[b] = s["p1"], s["p2"], s["mask"], s["E0"].reshape(9)
    d1, d2, dm = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda(), torch.from_numpy(M).cuda()
    res = pose.refine_essential_linear_batch(d1, d2, counts, E, dm, LRS.TH, method, ctx=ctx, **kw)
    torch.cuda.synchronize()
    masks = dm.cpu().numpy()
    assert d1.cpu().numpy().tobytes() == P1.tobytes() and d2.cpu().numpy().tobytes() == P2.tobytes()
    kinds = set()
    for b, s in enumerate(scenes):
        n = counts[b]
        assert masks[b, n:].tobytes() == M[b, n:].tobytes()
        if s is None:
            assert res["status"][b] == LRO.MLPL_E_FAILED and res["n_inliers"][b] == 0 and res["steps_done"][b] == 0
            assert res["E"][b].tobytes() == E[b].tobytes()
            continue
        g = _single(ctx, s["p1"], s["p2"], s["E0"], s["mask"], method, s["th"], **kw)
        assert (res["status"][b] == 0) == g["ok"] and (g["ok"] or res["status"][b] == LRO.MLPL_E_FAILED)
        assert res["E"][b].tobytes() == g["E"].tobytes()
        assert masks[b, :n].tobytes() == g["mask"].tobytes()
        assert res["n_inliers"][b] == g["n_inliers"] and res["steps_done"][b] == g["steps_done"]
        if not g["ok"]:
            assert res["E"][b].tobytes() == E[b].tobytes() and masks[b, :n].tobytes() == s["mask"].tobytes()
        kinds.add("refused" if not g["ok"] else ("refined" if g["steps_done"] else "unchanged"))
    return counts, kinds


@pytest.mark.parametrize("method", LRS.METHODS)
def test_batch_equals_single(ctx, method):
    names = _batch_of(method, {})
    counts, kinds = _check_batch(ctx, method, names, {})
    assert len(names) >= len(LRS.COUNTS) + 1 and len(set(counts.tolist())) > 5
    assert "refined" in kinds


@pytest.mark.parametrize("method", (0x12, 0x22, 0x32, 0x23))
def test_batch_equals_single_on_the_choice_scenes(ctx, method):
    """The one-step scenes of the choice (exits in the first, second and third chunk of the list, lists without exit) through the batch
    kernel's addressing; the single entry they are compared with is held to the restatement by test_scene_matches_restatement."""
    names = _batch_of(method, LRS.ONE_STEP)
    assert any(n and n.startswith("exit") for n in names) and any(n and n.startswith("none") for n in names)
    _, kinds = _check_batch(ctx, method, names, LRS.ONE_STEP)
    assert kinds == {"refined"}
