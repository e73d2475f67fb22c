"""ctypes wrapper over tests/cpp/libhomography_oracle.so, the sequential restatement of computeHomographyArrsac /
estimateMultHomographys (tests/cpp/homography_oracle.cpp; built by csrc/facade/Makefile, or here when it is missing)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG_FRESH = (0xFFFFFFFF, 0xFFFFFFFF)   # cv::RNG's default state, both samplers
_lib = None


def load():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "cpp", "homography_oracle.cpp")
        so = os.path.join(ROOT, "tests", "cpp", "libhomography_oracle.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src], check=True)
        _lib = C.CDLL(so)
        for f in ("ho_homography_arrsac", "ho_sample_model", "ho_homography_inliers", "ho_mult_homographies"):
            getattr(_lib, f).restype = C.c_int
        _lib.ho_last_refine_doubt.restype = C.c_double
    return _lib


def _pts(p):
    return np.ascontiguousarray(np.asarray(p, np.float64).reshape(-1, 2))


def _p(a):
    return C.c_void_p(a.ctypes.data)


def homography_arrsac(p1, p2, th, rng_state=None, variant=0):
    """rng_state (uint64[2]) is advanced in place; a fresh pair is used when None."""
    lib = load()
    p1, p2 = _pts(p1), _pts(p2)
    n = len(p1)
    st = np.array(RNG_FRESH, np.uint64) if rng_state is None else rng_state
    H, mask, ninl = np.zeros(9), np.zeros(max(n, 1), np.uint8), C.c_int(0)
    stats, margin = np.zeros(8, np.int64), C.c_double(0)
    ok = lib.ho_homography_arrsac(_p(p1), _p(p2), n, C.c_double(th), _p(st), int(variant), _p(H), _p(mask), C.byref(ninl), _p(stats),
                                  C.byref(margin))
    return {"ok": bool(ok), "H": H.reshape(3, 3), "mask": mask[:n], "n_inliers": ninl.value, "stats": stats, "rng_state": st.copy(),
            "margin": margin.value, "doubt": lib.ho_last_refine_doubt()}


def sample_model(p1, p2, idx, variant=0, polish=True):
    lib = load()
    p1, p2 = _pts(p1), _pts(p2)
    idx = np.ascontiguousarray(idx, np.int32)
    H = np.zeros(9)
    ok = lib.ho_sample_model(_p(p1), _p(p2), _p(idx), len(idx), int(variant), int(bool(polish)), _p(H))
    return bool(ok), H.reshape(3, 3)


def homography_inliers(p1, p2, H, th):
    lib = load()
    p1, p2 = _pts(p1), _pts(p2)
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    mask = np.zeros(len(p1), np.uint8)
    cnt = lib.ho_homography_inliers(_p(p1), _p(p2), len(p1), _p(H), C.c_double(th), _p(mask))
    return mask, cnt


def mult_homographies(p1, p2, th, var_th=True, max_planes=0, min_pts_per_plane=4, rng_state=None, variant=0, cap=16):
    lib = load()
    p1, p2 = _pts(p1), _pts(p2)
    n = len(p1)
    st = np.array(RNG_FRESH, np.uint64) if rng_state is None else rng_state
    npl, margin = C.c_int(0), C.c_double(0)
    H, num, strength, thu = np.zeros((cap, 9)), np.zeros(cap, np.int32), np.zeros(cap), np.zeros(cap)
    masks = np.zeros((cap, max(n, 1)), np.uint8)
    rc = lib.ho_mult_homographies(_p(p1), _p(p2), n, C.c_double(th), int(bool(var_th)), C.c_uint(max_planes), C.c_uint(min_pts_per_plane), _p(st),
                                  int(variant), cap, C.byref(npl), _p(H), _p(num), _p(strength), _p(thu), _p(masks), C.byref(margin))
    k = min(npl.value, cap)
    return {"rc": rc, "n_planes": npl.value, "H": H[:k].reshape(k, 3, 3), "num_inl": num[:k], "strength": strength[:k], "th_used": thu[:k],
            "masks": masks[:k, :n], "rng_state": st.copy(), "margin": margin.value,
            "doubt": lib.ho_last_refine_doubt()}
