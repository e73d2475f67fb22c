"""ctypes wrapper over tests/cpp/libhomography_align_oracle.so, the sequential restatement of the pose-from-planes half of
estimatePoseHomographies (tests/cpp/homography_align_oracle.cpp; built by csrc/facade/Makefile, or here when it is missing)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_LEN = 24
_lib = None


def load():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "cpp", "homography_align_oracle.cpp")
        so = os.path.join(ROOT, "tests", "cpp", "libhomography_align_oracle.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src], check=True)
        _lib = C.CDLL(so)
        for f in ("hao_alignment", "hao_jacobi33", "hao_solve_by_inverse"):
            getattr(_lib, f).restype = C.c_int
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def parse_info(info):
    """The info block both the restatement and the library write (24 doubles) as a dict."""
    info = np.asarray(info, np.float64)
    return {"code": int(info[0]), "q": int(info[1]), "rounds": info[2:10].astype(int).reshape(2, 4), "e1": info[10:12].copy(),
            "motion_errors": info[12:16].copy(), "choices": int(info[16]), "reason": int(info[17]), "margin_stop": float(info[18]),
            "margin_q": float(info[19])}


def alignment(p1, p2, labels, n_planes, H0, tol, variant=0):
    lib = load()
    p1 = np.ascontiguousarray(np.asarray(p1, np.float64).reshape(-1, 2))
    p2 = np.ascontiguousarray(np.asarray(p2, np.float64).reshape(-1, 2))
    labels = np.ascontiguousarray(labels, np.int32)
    H0 = np.ascontiguousarray(H0, np.float64).reshape(9)
    P = int(n_planes)
    R, t, E = np.zeros(9), np.zeros(3), np.zeros(9)
    norms, Hs, info = np.zeros((max(P, 1), 3)), np.zeros((max(P, 1), 9)), np.zeros(INFO_LEN)
    code = lib.hao_alignment(_p(p1), _p(p2), _p(labels), len(p1), P, _p(H0), C.c_double(tol), int(variant), _p(R), _p(t), _p(E), _p(norms),
                             _p(Hs), _p(info))
    out = parse_info(info)
    out.update(code=code, R=R.reshape(3, 3), t=t, E=E.reshape(3, 3), norms=norms[:P], Hs=Hs[:P].reshape(-1, 3, 3), info=info)
    return out


def jacobi33(a, variant=0):
    lib = load()
    a = np.ascontiguousarray(a, np.float64).reshape(9)
    d, v = np.zeros(3), np.zeros(9)
    ok = lib.hao_jacobi33(_p(a), int(variant), _p(d), _p(v))
    return ok, d, v.reshape(3, 3)


def solve_by_inverse(a, b):
    lib = load()
    a = np.ascontiguousarray(a, np.float64)
    n = a.shape[0]
    b = np.ascontiguousarray(b, np.float64).reshape(n)
    m = np.zeros(n)
    ok = lib.hao_solve_by_inverse(_p(a.reshape(-1)), _p(b), n, _p(m))
    return ok, m


def reproj_error2(p1, p2, E):
    """computeReprojError2 (pose_helper.cpp:639-664): the Sampson error of every correspondence under E, in its order of operations."""
    p1 = np.asarray(p1, np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, np.float64).reshape(-1, 2)
    E = np.asarray(E, np.float64).reshape(3, 3)
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    a0 = (E[0, 0] * x1 + E[0, 1] * y1) + E[0, 2]
    a1 = (E[1, 0] * x1 + E[1, 1] * y1) + E[1, 2]
    a2 = (E[2, 0] * x1 + E[2, 1] * y1) + E[2, 2]
    num = (x2 * a0 + y2 * a1) + a2
    b0 = (E[0, 0] * x2 + E[1, 0] * y2) + E[2, 0]
    b1 = (E[0, 1] * x2 + E[1, 1] * y2) + E[2, 1]
    return (num * num) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1)


def pose_homographies(p1, p2, th, mask=None, check_plane_strength=False, var_th=False, rng_state=None, variant=0):
    """The whole of estimatePoseHomographies composed from the two restatements: the plane search of tests/cpp/homography_oracle.cpp
    (MAX_PLANES_PER_PAIR = 50, MIN_PTS_PLANE = 15) on the rows the mask keeps, the strength gate, the alignment, the strict mask."""
    import homography_oracle as ho

    p1 = np.ascontiguousarray(np.asarray(p1, np.float64).reshape(-1, 2))
    p2 = np.ascontiguousarray(np.asarray(p2, np.float64).reshape(-1, 2))
    n = len(p1)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    q1, q2 = np.ascontiguousarray(p1[keep]), np.ascontiguousarray(p2[keep])
    st = np.array(ho.RNG_FRESH, np.uint64) if rng_state is None else rng_state
    out = {"result": 0, "n_planes": 0, "num_inl": np.zeros(0, np.int32), "H": np.zeros((0, 3, 3)), "strength": np.zeros(0), "margin_planes": np.inf}
    labels = np.full(len(q1), -1, np.int32)
    if len(q1) >= 4:
        r = ho.mult_homographies(q1, q2, th, var_th=var_th, max_planes=50, min_pts_per_plane=15, rng_state=st, variant=variant, cap=50)
        if r["rc"] != 0 or r["n_planes"] < 0:
            out.update(result=-1, n_planes=-1, rng_state=st.copy())
            return out
        out.update(n_planes=r["n_planes"], num_inl=r["num_inl"].copy(), H=r["H"].copy(), strength=r["strength"].copy(), margin_planes=r["margin"],
                   doubt=r["doubt"])
        for k in range(r["n_planes"]):
            labels[r["masks"][k] != 0] = k
    out.update(rng_state=st.copy(), labels=labels)
    if check_plane_strength and not (out["strength"][out["strength"] > 0.1].sum() > 0.5):
        out["result"] = -2
        return out
    P = out["n_planes"]
    a = alignment(q1, q2, labels, P, out["H"][0] if P else np.eye(3), th, variant)
    out["align"] = a
    if a["code"] != 0:
        out["result"] = -3
        return out
    err = reproj_error2(p1, p2, a["E"])
    th2 = th * th
    out.update(R=a["R"], t=a["t"], E=a["E"], mask=(err < th2).astype(np.uint8), n_inliers=int((err < th2).sum()),
               margin_mask=float(np.abs(err - th2).min() / th2))
    return out
