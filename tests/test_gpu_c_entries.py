"""The host-pointer entries against their device-pointer twins, the rule by which each robust estimator hands its mask back, and the count
check of the batch entries (csrc/mlpl_internal.h: upload_points, download_mask, counts_in_range).

A host-pointer entry uploads the correspondences, runs the body of its `_dev` twin and brings the mask back: with the same inputs and the
same seed or RNG state both forms must return the same code, model, mask and counts, bit for bit.  Sizes: the smallest n the entry accepts
and 257, one past a 256-thread block."""
import ctypes as C

import numpy as np
import pytest
import torch

import ba_scenes
import homography_scenes as HS
from matchinglib_poselib_amd import _lib, pose, synth

pytestmark = pytest.mark.gpu

FRESH = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)


def _scene(n, seed=20260501):
    p1, p2, R, t, _, th = synth.pose_scene(max(n, 8), 0.7, seed=seed)
    return np.ascontiguousarray(p1[:n]), np.ascontiguousarray(p2[:n]), R, t, th


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [6, 257])
def test_ransac_essential_twins(ctx, n):
    p1, p2, _, _, th = _scene(n)
    for refit in (False, True):
        h = pose.ransac_essential(p1, p2, th, max_iters=300, refit=refit, seed=7, ctx=ctx)
        d = pose.ransac_essential_device(_dev(p1), _dev(p2), th, max_iters=300, refit=refit, seed=7, ctx=ctx)
        assert (h["ok"], h["n_inliers"], h["iters"]) == (d["ok"], d["n_inliers"], d["iters"])
        assert _same(h["E"], d["E"])
        if h["ok"]:
            assert _same(h["mask"], d["mask"])


@pytest.mark.parametrize("n", [6, 257])
def test_arrsac_essential_twins(ctx, n):
    p1, p2, _, _, th = _scene(n)
    st_h, st_d = FRESH.copy(), FRESH.copy()
    h = pose.arrsac_essential(p1, p2, th, rng_state=st_h, ctx=ctx)
    d = pose.arrsac_essential_device(_dev(p1), _dev(p2), th, rng_state=st_d, ctx=ctx)
    assert (h["ok"], h["n_inliers"]) == (d["ok"], d["n_inliers"]) and st_h.tolist() == st_d.tolist()
    assert _same(h["E"], d["E"])
    if h["ok"] or h["n_inliers"] > 0:
        assert _same(h["mask"], d["mask"])


def _planes(n):
    if n < 40:
        p1, p2, _, _, th = HS.planes_scene(40, [30], 11, units="cam")
        return np.ascontiguousarray(p1[:n]), np.ascontiguousarray(p2[:n]), th
    p1, p2, _, _, th = HS.planes_scene(n, [n // 2, n // 4], 11, units="cam", shuffled=True)
    return p1, p2, th


@pytest.mark.parametrize("n", [1, 257])
def test_homography_arrsac_twins(ctx, n):
    p1, p2, th = _planes(n)
    st_h, st_d = FRESH.copy(), FRESH.copy()
    h = pose.homography_arrsac(p1, p2, th, rng_state=st_h, ctx=ctx)
    d = pose.homography_arrsac_device(_dev(p1), _dev(p2), th, rng_state=st_d, ctx=ctx)
    assert (h["ok"], h["n_inliers"]) == (d["ok"], d["n_inliers"]) and st_h.tolist() == st_d.tolist()
    assert _same(h["H"], d["H"]) and _same(h["stats"], d["stats"])
    if h["ok"]:
        assert _same(h["mask"], d["mask"])


@pytest.mark.parametrize("n", [4, 257])
def test_mult_homographies_twins(ctx, n):
    p1, p2, th = _planes(n)
    st_h, st_d = FRESH.copy(), FRESH.copy()
    h = pose.mult_homographies(p1, p2, th, min_pts_per_plane=min(30, n), rng_state=st_h, ctx=ctx)
    d = pose.mult_homographies_device(_dev(p1), _dev(p2), th, min_pts_per_plane=min(30, n), rng_state=st_d, ctx=ctx)
    assert (h["rc"], h["n_planes"]) == (d["rc"], d["n_planes"]) and st_h.tolist() == st_d.tolist()
    for k in ("H", "num_inl", "strength", "th_used", "found_at"):
        assert _same(h[k], d[k]), k
    if h["n_planes"] > 0:
        assert _same(h["labels"], d["labels"]) and _same(h["masks"], d["masks"])


@pytest.mark.parametrize("n", [1, 257])
def test_pose_homographies_twins(ctx, n):
    p1, p2, th = _planes(n)
    st_h, st_d = FRESH.copy(), FRESH.copy()
    h = pose.pose_homographies(p1, p2, th, rng_state=st_h, ctx=ctx)
    d = pose.pose_homographies_device(_dev(p1), _dev(p2), th, rng_state=st_d, ctx=ctx)
    assert (h["result"], h["n_inliers"], h["n_planes"]) == (d["result"], d["n_inliers"], d["n_planes"]) and st_h.tolist() == st_d.tolist()
    for k in ("R", "t", "E", "H", "num_inl", "strength", "info"):
        assert _same(h[k], d[k]), k
    if h["result"] == 0:
        assert _same(h["mask"], d["mask"])
    if h["n_planes"] > 0:
        assert _same(h["labels"], d["labels"])


@pytest.mark.parametrize("n", [0, 12, 257])     # 0: accepted and answered before the device is touched; 12: the fewest points the optimiser takes
def test_refine_stereo_ba_twins(ctx, n):
    s = ba_scenes.make_scene(max(n, 1), seed=3)
    p1, p2, Q = s["p1"][:n], s["p2"][:n], s["Q"][:n]
    h = pose.refine_stereo_ba(p1, p2, s["R"], s["t"], Q, s["th"], ctx=ctx)
    dq = _dev(Q)
    d = pose.refine_stereo_ba_device(_dev(p1), _dev(p2), s["R"], s["t"], dq, s["th"], ctx=ctx)
    assert h["accepted"] == d["accepted"] and h["mu"] == d["mu"]
    assert _same(h["R"], d["R"]) and _same(h["t"], d["t"]) and _same(h["info"], d["info"]) and _same(h["Q"], dq)


@pytest.mark.parametrize("n", [1, 257])     # (the device form takes no empty tensor: its pointers are null)
def test_triang_pts3d_twins(ctx, n):
    p1, p2, R, t, _ = _scene(n)
    m = (np.arange(n) % 5 != 0).astype(np.uint8)
    gh, Qh, mh = pose.triangPts3D(R, t, p1, p2, m, ctx=ctx)
    dq, dm = torch.zeros((n, 3), dtype=torch.float64, device="cuda"), _dev(m)
    gd = pose.triangPts3D_device(R, t, _dev(p1), _dev(p2), dm, Q_out=dq, ctx=ctx)
    assert gh == gd and _same(Qh, dq) and _same(mh, dm)


@pytest.mark.parametrize("n", [0, 257])
def test_get_pose_triang_pts_twins(ctx, n):
    p1, p2, R, t, _ = _scene(n)
    t = np.asarray(t, np.float64).reshape(3)
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    m = (np.arange(n) % 5 != 0).astype(np.uint8)
    gh, Rh, th_, Qh, mh = pose.getPoseTriangPts(E, p1, p2, m, ctx=ctx)
    dq, dm = torch.zeros((n, 3), dtype=torch.float64, device="cuda"), _dev(m)
    gd, Rd, td = pose.getPoseTriangPts_device(E, _dev(p1), _dev(p2), dm, Q_out=dq, ctx=ctx)
    assert gh == gd and _same(Rh, Rd) and _same(th_, td) and _same(Qh, dq) and _same(mh, dm)


# ---- the three rules by which a mask comes back: each call goes through the raw C entry with the caller's mask pre-filled with 7 -------------------
def _noise(n, seed=0):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-0.4, 0.4, (n, 2))), np.ascontiguousarray(rng.uniform(-0.4, 0.4, (n, 2)))


def test_ransac_without_a_model_leaves_the_mask(ctx):
    """thresh = 1e-30: thresh^2 lies below the smallest float, so only an error of exactly zero would pass -- no model gathers an inlier."""
    p1, p2, _, _, _ = _scene(8)
    for refit in (0, 1):
        E, mask, ninl, iters = np.zeros(9), np.full(8, 7, np.uint8), C.c_int(0), C.c_int(0)
        rc = ctx.lib.mlpl_ransac_essential(ctx.handle, p1.ctypes.data, p2.ctypes.data, 8, 1e-30, 0.999, 50, refit, 3, E.ctypes.data, mask.ctypes.data,
                                           C.byref(ninl), C.byref(iters))
        assert rc == _lib.MLPL_E_FAILED and ninl.value == 0 and "no model found" in _lib.last_error()
        assert (mask == 7).all()


def test_lmeds_hands_the_mask_back_with_a_failure(ctx):
    """Every correspondence at the origin: no sample gives a model, LMedS ends with MLPL_E_FAILED before it writes a mask, and the entry
    still copies the device mask out.  That buffer holds what the call before left in it: here the mask of a run that succeeded."""
    q1, q2, _, _, _ = _scene(8)
    good = pose.lmeds_essential(q1, q2, max_iters=50, seed=3, ctx=ctx)
    assert good["ok"] and 0 < good["mask"].sum() <= 8
    z = np.zeros((8, 2))
    E, mask, ninl, med = np.zeros(9), np.full(8, 7, np.uint8), C.c_int(0), C.c_double(0)
    rc = ctx.lib.mlpl_lmeds_essential(ctx.handle, z.ctypes.data, z.ctypes.data, 8, 0.999, 50, 3, E.ctypes.data, mask.ctypes.data, C.addressof(ninl),
                                      C.addressof(med))
    assert rc == _lib.MLPL_E_FAILED and ninl.value == 0 and "no model found" in _lib.last_error()
    assert not (mask == 7).any() and np.array_equal(mask, good["mask"])


def _arrsac_raw(ctx, p1, p2, th):
    n = len(p1)
    E, mask, ninl, st = np.zeros(9), np.full(n, 7, np.uint8), C.c_int(0), FRESH.copy()
    rc = ctx.lib.mlpl_arrsac_essential(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, th, 1, st.ctypes.data, E.ctypes.data, mask.ctypes.data,
                                       C.addressof(ninl))
    return rc, mask, ninl.value


def test_arrsac_hands_the_mask_back_with_a_failure_that_has_inliers(ctx):
    p1, p2 = _noise(8)     # pure noise: a winner that only its own sample supports
    rc, mask, ninl = _arrsac_raw(ctx, p1, p2, 1e-3)
    assert rc == _lib.MLPL_E_FAILED and ninl > 0
    d = pose.arrsac_essential_device(_dev(p1), _dev(p2), 1e-3, rng_state=FRESH.copy(), ctx=ctx)
    assert not d["ok"] and d["n_inliers"] == ninl
    assert np.array_equal(mask, d["mask"].cpu().numpy()) and int(mask.sum()) == ninl


# ---- the count check of the batch entries ------------------------------------------------------------------------------------------------------------
STRIDE = 16
_pinned = []


def _zeros():
    """One zeroed block of pinned host memory, readable and writable by the host and by the device at the same address: it stands for
    every host and device array of an entry.  The count check refuses each call before any of them is touched; should it ever not, the
    call works on zeros inside this block and the test fails by its asserts."""
    if not _pinned:
        _pinned.append(torch.zeros(1 << 16, dtype=torch.float64).pin_memory())
    return _pinned[0]


# entry -> (lowest count it takes, its arguments behind ctx as a function of the addresses of counts, of a mlpl_usac_params and of _zeros())
BATCH_ENTRIES = {
    "mlpl_arrsac_essential_batch_dev": (6, lambda c, u, P: (1, P, P, STRIDE, c, 1e-3, 1, P, P, P, P, P, None)),
    "mlpl_homography_arrsac_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, 1e-3, P, P, P, P, P, P, None)),
    "mlpl_mult_homographies_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, 1e-3, 1, 0, 4, P, 4, P, P, P, P, P, P, P, P, None)),
    "mlpl_pose_homographies_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, 1e-3, 0, 0, P, P, P, P, P, P, P, 4, P, P, P, P, P, P, P, None)),
    "mlpl_ransac_essential_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, 1e-3, 100, 0.999, P, 0, 50.0, P, P, None)),
    "mlpl_usac_essential_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, u, P, P, P, P, P, None, 0, None, None)),
    "mlpl_refine_essential_linear_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, P, pose.PR_8PT | pose.PR_PSEUDOHUBER_WEIGHTS, 4, 1.0, 1.0, 1.0, P, P, P,
                                                             P, P, None)),
    "mlpl_refine_essential_linear_rt_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, P, pose.PR_KNEIP | pose.PR_PSEUDOHUBER_WEIGHTS, 4, 1.0, 1.0, 1.0, P,
                                                                P, P, P, P, P, P, P, P, P, None)),
    "mlpl_recover_pose_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, P, 50.0, P, P, P, P, None)),
    "mlpl_triang_pts3d_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, P, P, 50.0, P, P, P, None)),
    "mlpl_refine_stereo_ba_batch_dev": (0, lambda c, u, P: (1, P, P, STRIDE, c, P, P, P, P, P, 1.25, 0.05, P, P, None)),
    "mlpl_refine_multicam_ba_batch_dev": (0, lambda c, u, P: (1, P, P, 2, STRIDE, P, c, P, P, P, P, 1.25, 0.05, P, P, None)),
}


def _ws_grows(ctx):
    g = C.c_longlong(0)
    ctx.lib.mlpl_debug_hop_trace(ctx.handle, None, None, 0, C.byref(g))
    return g.value


@pytest.mark.parametrize("entry", sorted(BATCH_ENTRIES))
def test_counts_outside_the_range_are_refused(ctx, entry):
    lo, args = BATCH_ENTRIES[entry]
    usac = pose.UsacParams()
    ctx.lib.mlpl_usac_default_params(C.addressof(usac), 1e-3)
    zeros = _zeros()
    for bad in (STRIDE + 1, lo - 1):
        counts = np.array([bad], np.int32)
        grows = _ws_grows(ctx)
        rc = getattr(ctx.lib, entry)(ctx.handle, *args(counts.ctypes.data, C.addressof(usac), zeros.data_ptr()))
        assert rc == _lib.MLPL_E_BAD_INPUT, (entry, bad, rc, _lib.last_error())
        assert f"counts[0] = {bad} outside [{lo}, stride = {STRIDE}]" in _lib.last_error(), _lib.last_error()
        assert _ws_grows(ctx) == grows       # refused before a buffer was asked for ...
        torch.cuda.synchronize()
        assert not zeros.any()               # ... and no output, of the host or of a kernel, was written
