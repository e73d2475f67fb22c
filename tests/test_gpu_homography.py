"""GPU parity tests for computeHomographyArrsac / estimateMultHomographys: the device kernels + host control flow of
mlpl_homography_arrsac / mlpl_mult_homographies against the sequential CPU restatement (tests/cpp/homography_oracle.cpp).  Decisions
(ok, statistics, both stream positions, inlier count, mask) must be EQUAL; H within TOL_H (tests/homography_scenes.py: 64 times the
distance between the restatement's two variants, measured on the CPU -- never against the device)."""
import os
import subprocess

import numpy as np
import pytest

import homography_oracle as ho
import homography_scenes as hs
from matchinglib_poselib_amd import MlplError, _lib, pose

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRESH = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)


def assert_same_plane(g, o, st_g, what=""):
    assert g["ok"] == o["ok"], (what, g["stats"], o["stats"])
    assert g["stats"][:8].tolist() == o["stats"].tolist(), (what, g["stats"], o["stats"])
    assert st_g.tolist() == o["rng_state"].tolist(), what
    assert g["n_inliers"] == o["n_inliers"], what
    if g["ok"]:
        assert np.array_equal(g["mask"], o["mask"]), what
        d = hs.h_dist(g["H"], o["H"])
        print(f"{what}: |H_dev - H_ref| = {d:.3e} (TOL_H {hs.TOL_H:.3e})")
        assert d <= hs.TOL_H, (what, d)


def test_sample_kernel_alone(ctx):
    p1, p2, lists = hs.sample_cases()
    for name, idx in lists.items():
        H, ok = pose.homography_sample_models(p1, p2, idx, ctx=ctx)
        o_ok, o_H = ho.sample_model(p1, p2, idx)
        assert bool(ok[0]) == o_ok, name
        if o_ok:
            d = hs.h_dist(H[0], o_H)
            print(f"{name}: |H_dev - H_ref| = {d:.3e}")
            assert d <= hs.TOL_H, (name, d)
    assert not ho.sample_model(p1, p2, lists["flat"])[0]            # the zero-spread sample is refused by both
    _, before = ho.sample_model(p1, p2, lists["m12"], polish=False)  # and the polish of the 12-point sample is not a no-op
    H, ok = pose.homography_sample_models(p1, p2, lists["m12"], ctx=ctx)
    assert hs.h_dist(H[0], before) > 1000 * hs.TOL_H
    # several samples in one launch = each alone
    both = np.stack([lists["m4"], lists["m4b"]])
    Hb, okb = pose.homography_sample_models(p1, p2, both, ctx=ctx)
    for k, name in enumerate(("m4", "m4b")):
        H1, ok1 = pose.homography_sample_models(p1, p2, lists[name], ctx=ctx)
        assert okb[k] == ok1[0] == 1 and Hb[k].tobytes() == H1[0].tobytes()


@pytest.mark.parametrize("name", [c[0] for c in hs.SINGLE])
def test_single_plane_equals_the_restatement(ctx, name):
    p1, p2, _, _, th = hs.single(name)
    st = FRESH.copy()
    g = pose.homography_arrsac(p1, p2, th, rng_state=st, ctx=ctx)
    o = ho.homography_arrsac(p1, p2, th)
    assert_same_plane(g, o, st, name)
    if name == "n1500_ext":
        assert o["stats"][6] > 1024 and g["ok"]                       # past the 1024-bit rows: the bits beyond come on demand
    if name == "n1200_gen":
        assert o["stats"][5] > 0 and g["stats"][5] == o["stats"][5]   # the generation branch of the preemptive stage ran


def test_fixture_on_the_device(ctx):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "homography_trace.npz"))
    for i in range(len(g["cases"])):
        st = FRESH.copy()
        r = pose.homography_arrsac(g[f"c{i}_p1"], g[f"c{i}_p2"], float(g[f"c{i}_th"][0]), rng_state=st, ctx=ctx)
        assert r["ok"] == bool(g[f"c{i}_ok"][0]) and np.array_equal(r["stats"][:8], g[f"c{i}_stats"]) and np.array_equal(st, g[f"c{i}_rng"])
        assert np.array_equal(np.packbits(r["mask"]), g[f"c{i}_mask"]) and hs.h_dist(r["H"], g[f"c{i}_H"]) <= hs.TOL_H


@pytest.mark.parametrize("name", ["n4", "n200", "n5000_half"])
def test_host_and_device_entries_give_identical_bytes(ctx, name):
    import torch
    p1, p2, _, _, th = hs.single(name)
    st_h, st_d = FRESH.copy(), FRESH.copy()
    h = pose.homography_arrsac(p1, p2, th, rng_state=st_h, ctx=ctx)
    d = pose.homography_arrsac_device(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), th, rng_state=st_d, ctx=ctx)
    assert h["ok"] and d["ok"] and h["H"].tobytes() == d["H"].tobytes() and h["mask"].tobytes() == d["mask"].cpu().numpy().tobytes()
    assert st_h.tobytes() == st_d.tobytes() and h["n_inliers"] == d["n_inliers"] and h["stats"].tobytes() == d["stats"].tobytes()
    m, cnt = pose.homography_inliers(p1, p2, h["H"], th, ctx=ctx)
    om, ocnt = ho.homography_inliers(p1, p2, h["H"], th)
    assert np.array_equal(m, om) and cnt == ocnt


def test_three_consecutive_calls_carry_the_streams(ctx):
    p1, p2, _, _, th = hs.single("n1024")
    st_g, st_o = FRESH.copy(), FRESH.copy()
    for call in range(3):
        g = pose.homography_arrsac(p1, p2, th, rng_state=st_g, ctx=ctx)
        o = ho.homography_arrsac(p1, p2, th, rng_state=st_o)
        assert_same_plane(g, o, st_g, f"call {call}")
    # the reference-named mirror draws from the process-wide pair estimateEssentialMat uses
    pose._arrsac_rng_state[:] = FRESH
    ok, H, mask, f1, f2 = pose.computeHomographyArrsac(p1, p2, th, ctx=ctx)
    o = ho.homography_arrsac(p1, p2, th)
    assert ok and np.array_equal(pose._arrsac_rng_state, o["rng_state"]) and np.array_equal(mask, o["mask"])
    assert np.array_equal(f1, p1[o["mask"] == 1]) and np.array_equal(f2, p2[o["mask"] == 1])
    pose._arrsac_rng_state[:] = FRESH


def test_failing_scene_returns_not_ok_with_equal_streams(ctx):
    p1, p2, th = hs.failing_scene()
    st = FRESH.copy()
    g = pose.homography_arrsac(p1, p2, th, rng_state=st, ctx=ctx)
    o = ho.homography_arrsac(p1, p2, th)
    assert not g["ok"] and not o["ok"] and g["stats"][:8].tolist() == o["stats"].tolist() and st.tolist() == o["rng_state"].tolist()
    st3 = FRESH.copy()
    assert not pose.homography_arrsac(p1[:3], p2[:3], th, rng_state=st3, ctx=ctx)["ok"] and np.array_equal(st3, FRESH)   # n < 4


def test_bad_arguments_are_refused(ctx):
    p1, p2, _, _, th = hs.single("n99")
    H, mask, st, ninl = np.zeros(9), np.zeros(99, np.uint8), FRESH.copy(), np.zeros(1, np.int32)
    lib, h = ctx.lib, ctx.handle
    bad = _lib.MLPL_E_BAD_INPUT
    assert lib.mlpl_homography_arrsac(h, p1.ctypes.data, p2.ctypes.data, 99, 0.0, st.ctypes.data, H.ctypes.data, mask.ctypes.data, None, None) == bad
    assert lib.mlpl_homography_arrsac(h, p1.ctypes.data, p2.ctypes.data, 99, float("nan"), st.ctypes.data, H.ctypes.data, mask.ctypes.data, None, None) == bad
    assert lib.mlpl_homography_arrsac(h, p1.ctypes.data, p2.ctypes.data, 0, th, st.ctypes.data, H.ctypes.data, mask.ctypes.data, None, None) == bad
    assert lib.mlpl_homography_arrsac(h, None, p2.ctypes.data, 99, th, st.ctypes.data, H.ctypes.data, mask.ctypes.data, None, None) == bad
    assert lib.mlpl_homography_arrsac(h, p1.ctypes.data, p2.ctypes.data, 99, th, None, H.ctypes.data, mask.ctypes.data, None, None) == bad
    assert np.array_equal(st, FRESH)
    with pytest.raises(MlplError):
        pose.mult_homographies(p1[:3], p2[:3], th, ctx=ctx)
    with pytest.raises(MlplError):
        pose.mult_homographies(p1, p2, th, cap=0, ctx=ctx)
    with pytest.raises(MlplError):
        pose.homography_sample_models(p1, p2, [0, 1, 2, 99], ctx=ctx)      # an index outside the correspondences
    with pytest.raises(MlplError):
        pose.homography_sample_models(p1, p2, [0, 1, 2], ctx=ctx)          # fewer than four points
    with pytest.raises(MlplError):
        pose.homography_sample_models(p1, p2, list(range(13)), ctx=ctx)    # more than twelve


@pytest.mark.parametrize("name,kw", hs.MULTI_CASES)
def test_multi_plane_equals_the_restatement(ctx, name, kw):
    p1, p2, _, _, th = hs.multi(name)
    st = FRESH.copy()
    g = pose.mult_homographies(p1, p2, th, rng_state=st, ctx=ctx, **kw)
    o = ho.mult_homographies(p1, p2, th, **kw)
    assert g["rc"] == o["rc"] and g["n_planes"] == o["n_planes"], (g["rc"], o["rc"], g["n_planes"], o["n_planes"])
    assert st.tolist() == o["rng_state"].tolist()
    assert g["num_inl"].tolist() == o["num_inl"].tolist() and g["th_used"].tobytes() == o["th_used"].tobytes()
    assert g["strength"].tobytes() == o["strength"].tobytes()          # the same double expression on the host
    assert np.array_equal(g["masks"], o["masks"])                      # original indexing, order after the descending sort
    for k in range(o["n_planes"]):
        assert hs.h_dist(g["H"][k], o["H"][k]) <= hs.TOL_H, (k, hs.h_dist(g["H"][k], o["H"][k]))


def test_multi_plane_labels_order_of_discovery_and_capacity(ctx):
    p1, p2, _, _, th = hs.multi("three")
    st = FRESH.copy()
    m = pose.mult_homographies(p1, p2, th, min_pts_per_plane=30, rng_state=st, ctx=ctx)
    assert sorted(m["found_at"].tolist()) == [0, 1, 2] and m["labels"].min() == -1 and m["labels"].max() == 2
    for k in range(3):
        assert np.array_equal(m["labels"] == k, m["masks"][k] == 1)
    # the mask entry (cap masks of n bytes) says the same as the labels
    cap, npl = 4, np.zeros(1, np.int32)
    H, num, stg, thu, masks = np.zeros((cap, 9)), np.zeros(cap, np.int32), np.zeros(cap), np.zeros(cap), np.zeros((cap, len(p1)), np.uint8)
    st2 = FRESH.copy()
    rc = ctx.lib.mlpl_mult_homographies(ctx.handle, p1.ctypes.data, p2.ctypes.data, len(p1), th, 1, 0, 30, st2.ctypes.data, cap, npl.ctypes.data,
                                        H.ctypes.data, num.ctypes.data, stg.ctypes.data, thu.ctypes.data, masks.ctypes.data)
    assert rc == 0 and npl[0] == 3 and np.array_equal(masks[:3], m["masks"]) and H[:3].tobytes() == m["H"].tobytes() and np.array_equal(st2, st)
    # more planes than the arrays hold: refused, and the streams are where they were
    st3 = FRESH.copy()
    with pytest.raises(MlplError):
        pose.mult_homographies(p1, p2, th, min_pts_per_plane=30, cap=2, rng_state=st3, ctx=ctx)
    assert np.array_equal(st3, FRESH)


def test_multi_plane_device_entry_and_mirror(ctx):
    import torch
    p1, p2, _, _, th = hs.multi("three")
    st_h, st_d = FRESH.copy(), FRESH.copy()
    h = pose.mult_homographies(p1, p2, th, min_pts_per_plane=30, rng_state=st_h, ctx=ctx)
    d = pose.mult_homographies_device(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), th, min_pts_per_plane=30, rng_state=st_d, ctx=ctx)
    assert h["n_planes"] == d["n_planes"] == 3 and h["H"].tobytes() == d["H"].tobytes() and st_h.tobytes() == st_d.tobytes()
    assert np.array_equal(h["masks"], d["masks"].cpu().numpy()) and h["num_inl"].tolist() == d["num_inl"].tolist()
    nm = pose.mult_homographies(p1, p2, th, min_pts_per_plane=30, rng_state=FRESH.copy(), want_masks=False, ctx=ctx)
    assert nm["H"].tobytes() == h["H"].tobytes() and "masks" not in nm
    pose._arrsac_rng_state[:] = FRESH
    rc, masks, pts, Hs, num, strength = pose.estimateMultHomographys(p1, p2, th, minPtsPerPlane=30, ctx=ctx)
    assert rc == 0 and num == h["num_inl"].tolist() and np.array_equal(pose._arrsac_rng_state, st_h)
    assert all(np.array_equal(pts[k][0], p1[masks[k] == 1]) for k in range(3))
    pose._arrsac_rng_state[:] = FRESH


def test_streams_are_shared_with_the_essential_matrix_estimator(ctx, oracle):
    """An E-ARRSAC call between two homography calls moves the streams exactly as the restatements of both say."""
    from matchinglib_poselib_amd import synth
    p1, p2, _, _, th = hs.single("n200")
    e1, e2, R, t, truth, eth = synth.pose_scene(300, 0.6, seed=20260107)
    st_g, st_o = FRESH.copy(), FRESH.copy()
    g = pose.homography_arrsac(p1, p2, th, rng_state=st_g, ctx=ctx)
    assert_same_plane(g, ho.homography_arrsac(p1, p2, th, rng_state=st_o), st_g, "first")
    ge = pose.arrsac_essential(e1, e2, eth, refine=False, rng_state=st_g, ctx=ctx)
    oe = oracle.arrsac_essential(e1, e2, eth, refine=False, rng_state=st_o)
    assert ge["ok"] == oe["ok"] and np.array_equal(st_g, st_o) and np.array_equal(ge["mask"], oe["mask"])
    g = pose.homography_arrsac(p1, p2, th, rng_state=st_g, ctx=ctx)
    assert_same_plane(g, ho.homography_arrsac(p1, p2, th, rng_state=st_o), st_g, "second")


def test_cpp_facade_equals_the_c_entries(ctx, tmp_path):
    """tests/cpp/homography_facade.cpp: both functions through the reference's C++ signatures -- optional outputs omitted, vectors appended
    to in the sorted branch, the stream pair shared with estimateEssentialMat."""
    from matchinglib_poselib_amd import synth
    exe = os.path.join(ROOT, "tests", "cpp", "homography_facade")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    p1, p2, _, _, th = hs.multi("three")
    e1, e2, R, t, truth, eth = synth.pose_scene(300, 0.6, seed=20260107)
    n, ne = len(p1), len(e1)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.int32(n).tobytes() + np.float64(th).tobytes() + p1.tobytes() + p2.tobytes())
        f.write(np.int32(ne).tobytes() + np.float64(eth).tobytes() + np.ascontiguousarray(e1, np.float64).tobytes()
                + np.ascontiguousarray(e2, np.float64).tobytes() + np.uint32(30).tobytes())
    subprocess.run([exe, str(inp), str(out)], check=True, timeout=120)
    buf = open(out, "rb").read()
    at = [0]

    def take(dtype, count=1):
        a = np.frombuffer(buf, dtype, count, at[0])
        at[0] += a.nbytes
        return a

    st = FRESH.copy()
    a = pose.homography_arrsac(p1, p2, th, rng_state=st, ctx=ctx)                       # A
    assert take(np.int32)[0] == 1 and take(np.float64, 9).tobytes() == a["H"].tobytes() and take(np.uint8, n).tobytes() == a["mask"].tobytes()
    assert take(np.int32)[0] == a["n_inliers"] and take(np.uint64, 2).tobytes() == st.tobytes()
    e = pose.arrsac_essential(e1, e2, eth, refine=False, rng_state=st, ctx=ctx)         # B
    assert take(np.int32)[0] == int(e["ok"]) and take(np.uint64, 2).tobytes() == st.tobytes()
    c = pose.homography_arrsac(p1, p2, th, rng_state=st, ctx=ctx)                       # C
    assert take(np.int32)[0] == 1 and take(np.float64, 9).tobytes() == c["H"].tobytes() and take(np.uint64, 2).tobytes() == st.tobytes()
    st = FRESH.copy()
    m = pose.mult_homographies(p1, p2, th, min_pts_per_plane=30, rng_state=st, ctx=ctx)  # D
    assert take(np.int32)[0] == 0 and take(np.int32)[0] == m["n_planes"] == 3 and take(np.int32)[0] == 1
    for k in range(3):
        assert take(np.uint32)[0] == m["num_inl"][k] and take(np.float64)[0] == m["strength"][k]
        assert take(np.float64, 9).tobytes() == m["H"][k].tobytes() and take(np.uint8, n).tobytes() == m["masks"][k].tobytes()
        assert take(np.int32)[0] == m["num_inl"][k]
    assert take(np.uint64, 2).tobytes() == st.tobytes()
    one = pose.mult_homographies(p1, p2, th, min_pts_per_plane=30, max_planes=1, rng_state=FRESH.copy(), ctx=ctx)   # E
    assert take(np.int32)[0] == 0 and take(np.int32)[0] == 1 and take(np.float64, 9).tobytes() == one["H"][0].tobytes()
    disc = np.argsort(m["found_at"], kind="stable")                                     # F: without num_inl, the order of discovery
    assert take(np.int32)[0] == 0 and take(np.int32)[0] == 3
    for k in disc:
        assert take(np.float64, 9).tobytes() == m["H"][k].tobytes() and take(np.uint8, n).tobytes() == m["masks"][k].tobytes()
    assert take(np.int32)[0] == 1 and at[0] == len(buf)
