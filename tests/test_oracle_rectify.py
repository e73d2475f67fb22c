"""CPU: stereo rectification.  mlpl_rectify_parameters is host arithmetic and runs here against the restatement tests/rectify_oracle.py;
the restatements of the maps and of the remap are checked on properties that do not depend on them (an epipolar test on projected points,
extended precision, an identity map, affine ramps).

Scene `strong` (k1 = -1.5 in `small`) runs all four reduction loops to reduction >= 0.25 (24 steps each) and takes the coefficient-free pass;
`strong_partial` (k1 = -0.9) is its counterpart whose loops end on their own (14, 18, 14, 16 steps)."""
import numpy as np
import pytest

import rectify_oracle as O
import rectify_scenes as S
from matchinglib_poselib_amd import pose
from matchinglib_poselib_amd._lib import MLPL_E_BAD_INPUT, MlplError

NAMES = sorted(S.SCENES)
DOUBLES = ("Rect1", "Rect2", "Knew", "P1", "P2")


@pytest.mark.parametrize("name", NAMES)
def test_epipolar_property(name):
    """independent of any restatement: points projected with (R, t) land on one row after Rect1 / Rect2 and Knew"""
    s = S.SCENES[name]
    g = pose.rectification_parameters(*S.call_args(name))
    rng = np.random.default_rng(5)
    X = np.stack([rng.uniform(-2, 2, 200), rng.uniform(-2, 2, 200), rng.uniform(4, 12, 200)], 1)
    X2 = X @ s["R"].T + s["t"]
    y = []
    for Xc, Rect in ((X, g["Rect1"]), (X2, g["Rect2"])):
        q = (Xc / Xc[:, 2:3]) @ Rect.T
        q = (q / q[:, 2:3]) @ g["Knew"].T
        y.append(q[:, 1])
    print(name, "max |y1 - y2| =", np.abs(y[0] - y[1]).max())
    assert np.abs(y[0] - y[1]).max() <= 1e-10
    for Rect in (g["Rect1"], g["Rect2"]):
        assert np.abs(Rect @ Rect.T - np.eye(3)).max() <= 1e-12
        assert abs(np.linalg.det(Rect) - 1.0) <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_parameters_against_restatement(name):
    """roi and the step counts are equal; the doubles lie within 64 times the distance between two evaluation orders of the restatement
    (its three inverses by cofactors against Gaussian elimination)"""
    g = pose.rectification_parameters(*S.call_args(name))
    o, l = S.oracle_parameters(name), S.oracle_parameters(name, "lu")
    assert g["roi"] == o["roi"] == l["roi"]
    assert np.array_equal(g["info"][4:], o["info"][4:]) and np.array_equal(l["info"][4:], o["info"][4:])
    for k in DOUBLES + ("info",):
        spread = np.abs(o[k] - l[k]).max()
        d = np.abs(g[k] - o[k]).max()
        print(name, k, "library - restatement", d, "cofactors - elimination", spread)
        assert d <= 64 * spread, (name, k, d, spread)


def test_scene_branches():
    """each scene takes the branch it is there for"""
    p = {n: S.oracle_parameters(n) for n in NAMES}
    sm = S.SCENES["small"]
    assert p["small"]["info"][0] < min(sm["K1"][1, 1], sm["K2"][1, 1])            # dk1 < 0 lowers the focal length
    assert abs(p["small"]["info"][3] - 1.086) < 1e-3 and p["small"]["roi"] == [3, 2, 94, 58]
    assert p["small_resized"]["Knew"][0, 2] < 0.9 * p["small"]["Knew"][0, 2]
    assert abs(S.SCENES["vertical"]["t"][1]) > abs(S.SCENES["vertical"]["t"][0])  # idx = 1
    assert p["vertical"]["info"][0] <= 70 and p["vertical"]["inner"][2] < 0 and p["vertical"]["roi"] == [0, 0, 0, 0]
    assert p["vertical"]["info"][3] == 1.0 and p["vertical"]["info"][1] == 0.0    # alpha < 0: no scaling
    assert list(p["strong"]["info"][4:]) == [24.0] * 4 and p["strong"]["info"][3] == 1.0      # the pass without coefficients; s clamped
    assert all(0 < v < 24 for v in p["strong_partial"]["info"][4:]) and 0.5 < p["strong_partial"]["info"][3] < 2.0
    assert p["strong_partial"]["info"][3] != 1.0
    for n in ("small", "kitti", "vertical"):
        assert list(p[n]["info"][4:]) == [0.0] * 4


@pytest.mark.parametrize("name", NAMES)
def test_roi_arguments_are_well_conditioned(name):
    """no ceil / floor argument of the ROI lies within 1e-3 of an integer, so 1e-13 of arithmetic noise cannot move it"""
    for a in S.oracle_parameters(name)["roi_args"]:
        assert abs(a - round(a)) > 1e-3, (name, a)


def test_parameters_optional_outputs_and_bad_input():
    from matchinglib_poselib_amd import _lib

    lib = _lib.load_library()
    s = S.SCENES["small"]
    a = [np.ascontiguousarray(np.asarray(s[k], np.float64).reshape(-1)) for k in ("R", "t", "K1", "K2", "dist1", "dist2")]
    r1, r2, kn = np.zeros(9), np.zeros(9), np.zeros(9)

    def call(R=a[0], t=a[1], K1=a[2], n1=5, w=97, h=61, alpha=0.2, nw=0, nh=0):
        return lib.mlpl_rectify_parameters(R.ctypes.data, t.ctypes.data, K1.ctypes.data, a[3].ctypes.data, a[4].ctypes.data, n1, a[5].ctypes.data, 8,
                                           w, h, alpha, nw, nh, r1.ctypes.data, r2.ctypes.data, kn.ctypes.data, None, None, None, None)

    assert call() == 0                                            # roi, P1, P2 and info are optional
    o = S.oracle_parameters("small")
    assert np.array_equal(r1.reshape(3, 3), o["Rect1"]) and np.array_equal(kn.reshape(3, 3), o["Knew"])
    bad = a[0].copy()
    bad[4] = np.nan
    inf_t = a[1].copy()
    inf_t[0] = np.inf
    for kw in (dict(R=bad), dict(t=np.zeros(3)), dict(t=inf_t), dict(w=0), dict(h=-3), dict(n1=3), dict(alpha=float("nan")), dict(nw=-1)):
        assert call(**kw) == MLPL_E_BAD_INPUT, kw
    with pytest.raises(MlplError):
        pose.rectification_parameters(s["R"], s["t"], s["K1"], s["K2"], [0.1, 0.2, 0.3], None, s["size"])
    # t is normalised: a scaled t gives the same result up to the rounding of the division
    g1 = pose.rectification_parameters(*S.call_args("small"))
    args = list(S.call_args("small"))
    args[1] = 7.5 * args[1]
    g2 = pose.rectification_parameters(*args)
    assert np.abs(g1["Rect2"] - g2["Rect2"]).max() < 1e-13 and g1["roi"] == g2["roi"]
    # n_dist = 0 is eight zeros
    args = list(S.call_args("kitti"))
    args[4], args[5] = np.zeros(8), np.zeros(4)
    g3, g4 = pose.rectification_parameters(*args), pose.rectification_parameters(*S.call_args("kitti"))
    assert all(np.array_equal(g3[k], g4[k]) for k in DOUBLES) and g3["roi"] == g4["roi"]


@pytest.mark.parametrize("name", ["small", "small_resized", "strong", "kitti"])
def test_map_restatement_against_extended_precision(name):
    """the double formula, rounded to float32, stays within 1 float32 ulp of the same formula in numpy.longdouble"""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "the yardstick needs a numpy.longdouble wider than double"
    w, h = S.out_size(name)
    for side in (0, 1):
        ir, k, f = O.map_matrix(*S.map_args(name, side))
        u = np.arange(w, dtype=np.longdouble)[None, :].repeat(h, 0)
        v = np.arange(h, dtype=np.longdouble)[:, None].repeat(w, 1)
        ex, ey = O.map_formula(u, v, ir, k, f, xp=np.longdouble)
        mx, my = S.oracle_maps(name, side)
        for m, e in ((mx, ex), (my, ey)):
            ok = np.isfinite(e) & (np.abs(e) < 1e30)
            ulp = np.spacing(np.abs(m[ok]).astype(np.float32)).astype(np.longdouble)
            err = np.abs(m[ok].astype(np.longdouble) - e[ok]) / ulp
            print(name, side, "max error in float32 ulps", float(err.max()))
            assert err.max() <= 1.0


def test_maps_of_identity_rectification():
    """no distortion, Rect = I, Knew = K: every pixel maps to itself"""
    K = np.array([[100.0, 0, 31.5], [0, 100.0, 20.25], [0, 0, 1]])
    mx, my = O.maps(K, None, np.eye(3), K, 64, 40)
    assert np.abs(mx - np.arange(64)[None, :]).max() <= 4e-6 and np.abs(my - np.arange(40)[:, None]).max() <= 4e-6


def test_remap_restatement_identity_and_ramps():
    img = S.image(97, 61, 1)
    h, w = img.shape
    x = np.arange(w, dtype=np.float32)[None, :].repeat(h, 0)
    y = np.arange(h, dtype=np.float32)[:, None].repeat(w, 1)
    assert np.array_equal(O.remap(img, x, y), img)                       # an identity map copies the image
    # affine ramps with a slope of at most 4 levels per pixel: within 1 grey level of the exact bilinear value of the byte image (the map
    # position is rounded to 1 / 32: at most (4 + 4) / 64 levels; the result is rounded to a byte: at most 1 / 2)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(2)
    for (a, b, c) in ((1.0, 0.5, 3.0), (-2.0, 1.5, 250.0), (4.0, 0.0, 0.0), (0.0, -4.0, 255.0), (4.0, 4.0, -300.0), (0.25, 0.125, 17.0)):
        ramp = a * xx + b * yy + c
        ok_img = (ramp >= 0) & (ramp <= 255)
        rimg = np.clip(np.rint(ramp), 0, 255).astype(np.uint8)
        mx = rng.uniform(0, w - 1.001, (50, 70)).astype(np.float32)
        my = rng.uniform(0, h - 1.001, (50, 70)).astype(np.float32)
        got = O.remap(rimg, mx, my).astype(np.float64)
        x0, y0 = np.floor(mx).astype(int), np.floor(my).astype(int)
        fx, fy = mx.astype(np.float64) - x0, my.astype(np.float64) - y0
        p = rimg.astype(np.float64)
        exact = (p[y0, x0] * (1 - fx) + p[y0, x0 + 1] * fx) * (1 - fy) + (p[y0 + 1, x0] * (1 - fx) + p[y0 + 1, x0 + 1] * fx) * fy
        inside = ok_img[y0, x0] & ok_img[y0 + 1, x0] & ok_img[y0, x0 + 1] & ok_img[y0 + 1, x0 + 1]      # the four taps are unclipped ramp values
        assert inside.sum() > 300
        print("ramp", (a, b, c), "max |fixed point - exact bilinear| =", np.abs(got - exact)[inside].max())
        assert np.abs(got - exact)[inside].max() <= 1.0


def test_remap_restatement_hostile_values():
    img = S.image(97, 61, 1)
    mx, my = S.hostile_maps(97, 61)
    out = O.remap(img, mx, my)
    bad = ~np.isfinite(mx) | ~np.isfinite(my) | (np.abs(mx) > 1e6) | (np.abs(my) > 1e6)
    assert bad.sum() > 20 and not out[bad].any()                         # outside: 0
    full = np.full((4, 5), -7.0, np.float32)
    assert not O.remap(img, full, full).any()                            # an all-outside map
    # a tie of the x 32 rounding goes to the even side: 1 / 64 -> sx = 0 (not 1), 3 / 64 -> sx = 2
    r = np.zeros((1, 4), np.uint8)
    r[0] = (0, 64, 128, 192)
    t = O.remap(r, np.float32([[1 / 64, 3 / 64, 1 + 1 / 64, 1 + 3 / 64]]), np.zeros((1, 4), np.float32))
    assert list(t[0]) == [0, 4, 64, 68]
