"""GPU parity tests for the pose-from-planes half of estimatePoseHomographies: the one-workgroup alignment kernel behind
mlpl_homography_alignment and the whole function mlpl_pose_homographies against the sequential CPU restatements
(tests/cpp/homography_align_oracle.cpp, composed with tests/cpp/homography_oracle.cpp for the plane search).  Decisions (code, chosen
candidate, rounds of every outer turn, candidate choices, plane counts, stream positions, masks) must be EQUAL; R, t, E, normals and
homographies within TOL_A (tests/homography_pose_scenes.py: 64 times the distance between the restatement's two variants, measured on
the CPU -- never against the device)."""
import ctypes as C

import numpy as np
import pytest

import homography_align_oracle as hao
import homography_pose_scenes as S
import homography_scenes as hs
from matchinglib_poselib_amd import MlplError, _lib, pose

pytestmark = pytest.mark.gpu

FRESH = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
_ref = {}


def ref_alignment(name):
    if name not in _ref:
        sc = S.scene(name)
        _ref[name] = (sc, hao.alignment(sc["p1"], sc["p2"], sc["labels"], sc["P"], sc["H0"], sc["th"], 0))
    return _ref[name]


def assert_same_alignment(g, o, what, tol=S.TOL_A):
    gi, oi = g["info"], o["info"]
    assert gi[:10].tolist() == oi[:10].tolist() and gi[16] == oi[16] and gi[17] == oi[17], (what, gi[:18], oi[:18])
    if o["code"] != 0:
        return
    d_err = float(np.abs(gi[10:16] - oi[10:16]).max())
    d = {k: float(np.abs(g[k] - o[k]).max()) for k in ("R", "t", "E", "norms", "Hs")}
    print(f"{what}: errors {d_err:.3e} " + " ".join(f"{k} {v:.3e}" for k, v in d.items()) + f" (tolerance {tol:.3e})")
    assert d_err <= tol and max(d.values()) <= tol, (what, d, d_err)


@pytest.mark.parametrize("name", [c[0] for c in S.SCENES])
def test_alignment_equals_the_restatement(ctx, name):
    sc, o = ref_alignment(name)
    g = pose.homography_alignment(sc["p1"], sc["p2"], sc["labels"], sc["P"], sc["num_inl"], sc["H0"], sc["th"], ctx=ctx)
    assert g["code"] == 0
    assert_same_alignment(g, o, name, S.tol_of(S.units_of(name)))
    if name == "forty":
        assert g["info"][2:6].tolist() == [40, 40, 40, 40]
    if name == "exact":
        assert g["info"][10 + int(g["info"][1])] < sc["th"]


def test_fixture_on_the_device(ctx):
    import os
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "homography_align_trace.npz"))
    for name in S.FIXTURE:
        sc = S.scene(name)
        g = pose.homography_alignment(sc["p1"], sc["p2"], sc["labels"], sc["P"], sc["num_inl"], sc["H0"], sc["th"], ctx=ctx)
        assert g["info"][:10].tolist() == gold[name + "_info"][:10].tolist()
        for key in ("R", "t", "E", "norms", "Hs"):
            assert np.abs(g[key] - gold[f"{name}_{key}"]).max() <= S.tol_of(S.units_of(name)), (name, key)


def _alignment_dev(ctx, sc):
    import torch
    d1, d2 = torch.from_numpy(sc["p1"]).cuda(), torch.from_numpy(sc["p2"]).cuda()
    dl = torch.from_numpy(sc["labels"]).cuda()
    P = sc["P"]
    R, t, E, info, norms, Hs = np.zeros(9), np.zeros(3), np.zeros(9), np.zeros(24), np.zeros((P, 3)), np.zeros((P, 9))
    H0 = np.ascontiguousarray(sc["H0"], np.float64)
    rc = ctx.lib.mlpl_homography_alignment_dev(ctx.handle, d1.data_ptr(), d2.data_ptr(), dl.data_ptr(), len(sc["p1"]), P, sc["num_inl"].ctypes.data,
                                               H0.ctypes.data, float(sc["th"]), R.ctypes.data, t.ctypes.data, E.ctypes.data, norms.ctypes.data,
                                               Hs.ctypes.data, info.ctypes.data, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    return R, t, E, norms, Hs, info


@pytest.mark.parametrize("name", ["p2_n38", "p3_n900", "p2_n4100"])
def test_alignment_host_and_device_entries_give_identical_bytes(ctx, name):
    sc = S.scene(name)
    g = pose.homography_alignment(sc["p1"], sc["p2"], sc["labels"], sc["P"], sc["num_inl"], sc["H0"], sc["th"], ctx=ctx)
    R, t, E, norms, Hs, info = _alignment_dev(ctx, sc)
    assert info.tobytes() == g["info"].tobytes()
    for a, b in ((R, g["R"]), (t, g["t"]), (E, g["E"]), (norms, g["norms"]), (Hs, g["Hs"])):
        assert a.tobytes() == np.ascontiguousarray(b).tobytes()
    # and a second run gives the same bytes: fixed-order sums
    g2 = pose.homography_alignment(sc["p1"], sc["p2"], sc["labels"], sc["P"], sc["num_inl"], sc["H0"], sc["th"], ctx=ctx)
    assert all(np.ascontiguousarray(g[k]).tobytes() == np.ascontiguousarray(g2[k]).tobytes() for k in ("R", "t", "E", "norms", "Hs", "info"))


def test_alignment_defined_failures(ctx):
    sc = S.scene("p2_n63")

    def run(p1, p2, labels, P, H0):
        labels = np.ascontiguousarray(labels, np.int32)
        num = np.array([(labels == k).sum() for k in range(P)], np.int32)
        g = pose.homography_alignment(p1, p2, labels, P, num, H0, sc["th"], ctx=ctx)
        o = hao.alignment(p1, p2, labels, P, H0, sc["th"], 0)
        assert_same_alignment(g, o, "failure")
        assert g["code"] == -3
        for k in ("R", "t", "E", "norms", "Hs"):   # outputs untouched
            assert not g[k].any()
        return int(g["info"][17])

    assert run(sc["p1"], sc["p2"], np.where(sc["labels"] == 0, 0, -1), 1, sc["H0"]) == 5          # one plane
    Rz = S.rodrigues([0.2, -0.1, 1.0], 0.05)
    p2 = np.c_[sc["p1"], np.ones(len(sc["p1"]))] @ Rz.T
    assert run(sc["p1"], np.ascontiguousarray(p2[:, :2] / p2[:, 2:3]), sc["labels"], 2, Rz) == 3   # a pure rotation
    assert run(sc["p1"], sc["p2"], np.where(sc["labels"] == 1, -1, sc["labels"]), 2, sc["H0"]) == 6   # an empty plane
    assert run(sc["p1"], sc["p2"], sc["labels"], 2, np.diag([1.0, 1.0, 0.5])) == 1                 # H0 refused by the decomposition


def test_alignment_malformed_calls(ctx):
    sc = S.scene("p2_n63")
    ok = dict(p1=sc["p1"], p2=sc["p2"], labels=sc["labels"], n_planes=2, num_inl=sc["num_inl"], H0=sc["H0"], tol=sc["th"])

    def refused(**kw):
        a = dict(ok, **kw)
        with pytest.raises(MlplError) as e:
            pose.homography_alignment(a["p1"], a["p2"], a["labels"], a["n_planes"], a["num_inl"], a["H0"], a["tol"], ctx=ctx)
        assert e.value.code == _lib.MLPL_E_BAD_INPUT

    for tol in (0.0, -1.0, float("inf"), float("nan")):
        refused(tol=tol)
    bad = sc["labels"].copy()
    bad[5] = 2
    refused(labels=bad)                                                  # a label >= P
    refused(num_inl=sc["num_inl"] + np.array([1, -1], np.int32))         # num_inl not matching the labels
    refused(n_planes=65, num_inl=np.zeros(65, np.int32))
    z = np.zeros(24)
    rc = ctx.lib.mlpl_homography_alignment(ctx.handle, None, sc["p2"].ctypes.data, sc["labels"].ctypes.data, len(sc["p1"]), 2, sc["num_inl"].ctypes.data,
                                           z.ctypes.data, 1e-3, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data)
    assert rc == _lib.MLPL_E_BAD_INPUT
    rc = ctx.lib.mlpl_homography_alignment(ctx.handle, sc["p1"].ctypes.data, sc["p2"].ctypes.data, sc["labels"].ctypes.data, 0, 2,
                                           sc["num_inl"].ctypes.data, z.ctypes.data, 1e-3, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                                           z.ctypes.data, z.ctypes.data)
    assert rc == _lib.MLPL_E_BAD_INPUT


# ---- the whole function ---------------------------------------------------------------------------------------------------------------------
def assert_same_pose(g, o, st_g, what):
    assert g["result"] == o["result"], (what, g["result"], o["result"])
    assert st_g.tolist() == o["rng_state"].tolist(), what
    assert g["n_planes"] == o["n_planes"], what
    if o["n_planes"] > 0:
        assert g["num_inl"].tolist() == o["num_inl"].tolist(), what
        assert np.array_equal(np.asarray(g["labels"]), o["labels"]), what
        for k in range(o["n_planes"]):
            assert hs.h_dist(g["H"][k], o["H"][k]) <= hs.TOL_H, (what, k)
    if o["result"] != 0:
        return
    assert g["n_inliers"] == o["n_inliers"] and np.array_equal(np.asarray(g["mask"]), o["mask"]), what
    assert_same_alignment(dict(info=g["info"], code=0, R=g["R"], t=g["t"], E=g["E"], norms=np.zeros(1), Hs=np.zeros(1)),
                          dict(o["align"], norms=np.zeros(1), Hs=np.zeros(1)), what, 64 * S.S_CAM)


@pytest.mark.parametrize("name,masked", [(c[0], False) for c in S.FULL] + [("full_two", True)])
def test_pose_homographies_equals_the_restatements(ctx, name, masked):
    sc = S.full_scene(name)
    mask = S.full_mask(len(sc["p1"])) if masked else None
    st, st_o = FRESH.copy(), FRESH.copy()
    g = pose.pose_homographies(sc["p1"], sc["p2"], sc["th"], mask=mask, rng_state=st, ctx=ctx)
    o = hao.pose_homographies(sc["p1"], sc["p2"], sc["th"], mask=mask, rng_state=st_o)
    assert o["result"] == 0
    assert_same_pose(g, o, st, f"{name} masked={masked}")


@pytest.mark.parametrize("masked", [False, True])
def test_pose_homographies_host_and_device_entries_give_identical_bytes(ctx, masked):
    import torch
    sc = S.full_scene("full_two")
    mask = S.full_mask(len(sc["p1"])) if masked else None
    st, st_d = FRESH.copy(), FRESH.copy()
    g = pose.pose_homographies(sc["p1"], sc["p2"], sc["th"], mask=mask, rng_state=st, ctx=ctx)
    d = pose.pose_homographies_device(torch.from_numpy(sc["p1"]).cuda(), torch.from_numpy(sc["p2"]).cuda(), sc["th"],
                                      mask=None if mask is None else torch.from_numpy(mask).cuda(), rng_state=st_d, ctx=ctx)
    assert g["result"] == d["result"] == 0 and st.tobytes() == st_d.tobytes()
    for k in ("R", "t", "E", "H", "num_inl", "strength", "info"):
        assert np.ascontiguousarray(g[k]).tobytes() == np.ascontiguousarray(d[k]).tobytes(), k
    assert g["n_inliers"] == d["n_inliers"] and np.array_equal(g["mask"], d["mask"].cpu().numpy())
    assert np.array_equal(g["labels"], d["labels"].cpu().numpy()[:len(g["labels"])])


def test_pose_homographies_defined_results(ctx):
    def run(p1, p2, th, **kw):
        st, st_o = FRESH.copy(), FRESH.copy()
        g = pose.pose_homographies(p1, p2, th, rng_state=st, ctx=ctx, **kw)
        o = hao.pose_homographies(p1, p2, th, rng_state=st_o, **kw)
        assert_same_pose(g, o, st, str(kw))
        assert not g["R"].any() and not g["t"].any() and not g["E"].any() and not g["mask"].any() and g["n_inliers"] == 0   # untouched
        return g["result"]

    sc = S.full_scene("full_weak")
    assert run(sc["p1"], sc["p2"], sc["th"], check_plane_strength=True) == -2
    sc = S.full_scene("full_one")
    assert run(sc["p1"], sc["p2"], sc["th"]) == -3
    p1, p2, th = S.noise_scene()
    assert run(p1, p2, th) == -1
    assert run(p1[:3], p2[:3], th) == -3                                  # fewer than 4 rows: the plane loop does not run
    assert run(p1[:3], p2[:3], th, check_plane_strength=True) == -2


def test_pose_homographies_carries_the_streams(ctx):
    st, st_o = FRESH.copy(), FRESH.copy()
    for name in ("full_two", "full_wide", "full_two"):
        sc = S.full_scene(name)
        g = pose.pose_homographies(sc["p1"], sc["p2"], sc["th"], rng_state=st, ctx=ctx)
        o = hao.pose_homographies(sc["p1"], sc["p2"], sc["th"], rng_state=st_o)
        assert g["result"] == o["result"] and st.tolist() == st_o.tolist() and g["num_inl"].tolist() == o["num_inl"].tolist(), name
    assert st.tolist() != FRESH.tolist()


def test_pose_homographies_malformed_calls(ctx):
    sc = S.full_scene("full_two")
    for th in (0.0, float("inf"), float("nan")):
        st = FRESH.copy()
        with pytest.raises(MlplError) as e:
            pose.pose_homographies(sc["p1"], sc["p2"], th, rng_state=st, ctx=ctx)
        assert e.value.code == _lib.MLPL_E_BAD_INPUT and st.tolist() == FRESH.tolist()
    z, i = np.zeros(16), C.c_int(0)
    rc = ctx.lib.mlpl_pose_homographies(ctx.handle, sc["p1"].ctypes.data, sc["p2"].ctypes.data, 0, None, 1e-3, 0, 0, FRESH.copy().ctypes.data,
                                        C.addressof(i), z.ctypes.data, z.ctypes.data, z.ctypes.data, C.addressof(i), z.ctypes.data, 0, None, None, None,
                                        None, None, None)
    assert rc == _lib.MLPL_E_BAD_INPUT
