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
