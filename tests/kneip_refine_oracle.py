"""float64 restatement of poselib::refineEssentialLinear with PR_KNEIP (P/source/pose_linear_refinement.cpp:85-309 and :535-590) -- the
checker of mlpl_refine_essential_linear_rt.  TEST INFRASTRUCTURE ONLY.

The solver is the project's own CPU composition, dgm::eigensolver of matchinglib_poselib_amd/csrc/usac_degen_math.h, reached through the
ctypes shim tests/test_usac_degen_math.py uses (tests/cpp/degen_math_shim.cpp); tests/golden/kneip_eigensolver.npz holds it against the
reference's OpenGV on the share of problems where both end at the same minimum.  Around it, restated from the reference:
  the adapter (bearings of image 2, bearings of image 1); the solve on the current inlier list in list order, the translation's sign
  from the first list entry (opengv relative_pose/methods.cpp:496-549);
  t = translation / |translation| (Eigen: times the reciprocal of the norm); the step is rejected on a NaN in R, on a non-rotation
  (isMatRoationMat, pose_helper.cpp:2947-2954) or on t.isZero(1e-3); the model is E = [t]x R (getEfromRT);
  without a usable start rotation up to 12 attempts at step 0, each from the identity perturbed in Cayley space with three rand() draws
  (PoseFunctions.cpp:30-41), an attempt being taken when its count at th^2 reaches (1 - max_loss) * inliers; all 12 failing leaves the
  loop: true, E unchanged, the mask made 0 / 1, R cleared;
  R and t are written under the rule at :272-293 (in effect: at least one step was accepted).
The weight bits change nothing (OpenGV's useWeights stays false).  Stated deviation, shared with the device: with weight bits other than
0x10 / 0x20 the reference sums its zero-padded inlier vector until the first accepted step; here always the list itself.
`margin` is the smallest relative distance of an evaluated error from the threshold it was compared with, as linear_refine_oracle reports it.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import linear_refine_oracle as LRO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLPL_OK, MLPL_E_FAILED = 0, -3
PR_KNEIP = 0x4
MAX_SOLS_KNEIP = 12
RAND_MAX = 2147483647

_shim_cache = None


def shim():
    """The ctypes shim over usac_degen_math.h, compiled on first use (the recipe of tests/test_usac_degen_math.py)."""
    global _shim_cache
    if _shim_cache is None:
        src = os.path.join(ROOT, "tests", "cpp", "degen_math_shim.cpp")
        so = os.path.join(ROOT, "tests", "cpp", "libdegen_math_shim.so")
        hdr = os.path.join(ROOT, "matchinglib_poselib_amd", "csrc", "usac_degen_math.h")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src], check=True)
        lib = C.CDLL(so)
        for name in ("shim_eigensolver", "shim_e_from_rt"):
            getattr(lib, name).restype = None
        _shim_cache = lib
    return _shim_cache


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def glibc_rand(seed, count):
    """The first `count` values of rand() after srand(seed) (glibc's TYPE_3 additive feedback generator)."""
    r = [0] * 34
    r[0] = seed & 0xFFFFFFFF or 1
    for i in range(1, 31):
        x = r[i - 1] if r[i - 1] < 2 ** 31 else r[i - 1] - 2 ** 32  # int32; C division truncates
        hi = abs(x) // 127773 * (1 if x >= 0 else -1)
        lo = x - hi * 127773
        word = 16807 * lo - 2836 * hi
        r[i] = word + 2147483647 if word < 0 else word
    for i in range(31, 34):
        r[i] = r[i - 31]
    out = []
    for i in range(34, 344 + count):
        r.append((r[i - 31] + r[i - 3]) & 0xFFFFFFFF)
        if i >= 344:
            out.append(r[i] >> 1)
    return out


def is_rotation(R):
    """poselib::isMatRoationMat: every entry of R^T R - I within 1e-3, det R - 1 within 1e-3."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    if not np.all(np.isfinite(R)):
        return False
    chk = R.T @ R - np.eye(3)
    d = np.linalg.det(R) - 1.0
    return bool(np.all(np.abs(chk) <= 1e-3) and -1e-3 < d < 1e-3)


def perturbed_identity(raw3):
    """getPerturbedRotation(identity, 0.1): the Cayley parameters of the identity are zero; cayley2rot."""
    c = [0.0 + ((float(v) / float(RAND_MAX)) - 0.5) * 2.0 * 0.1 for v in raw3]
    Rr = [1 + c[0] * c[0] - c[1] * c[1] - c[2] * c[2], 2 * (c[0] * c[1] - c[2]), 2 * (c[0] * c[2] + c[1]),
          2 * (c[0] * c[1] + c[2]), 1 - c[0] * c[0] + c[1] * c[1] - c[2] * c[2], 2 * (c[1] * c[2] - c[0]),
          2 * (c[0] * c[2] - c[1]), 2 * (c[1] * c[2] + c[0]), 1 - c[0] * c[0] - c[1] * c[1] + c[2] * c[2]]
    scale = 1 + c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
    return np.array([(1 / scale) * v for v in Rr])


def eigensolver(pts, idx, R0):
    """dgm::eigensolver on the rows idx of pts = [x1 y1 x2 y2] (adapter view 1 = image 2), starting from R0 -> R (9), raw translation (3)."""
    idx = np.ascontiguousarray(idx, np.int32)
    R0 = np.ascontiguousarray(R0, np.float64).reshape(9)
    R, t = np.zeros(9), np.zeros(3)
    shim().shim_eigensolver(_ptr(pts), _ptr(idx), len(idx), _ptr(R0), _ptr(R), _ptr(t))
    return R, t


def solve_step(pts, idx, R0, solver=eigensolver):
    """refineModel, PR_KNEIP -> (R, t, E) or None when the reference rejects the step."""
    R, tt = solver(pts, idx, R0)
    with np.errstate(all="ignore"):
        inv = 1.0 / math.sqrt(tt[0] * tt[0] + (tt[1] * tt[1] + tt[2] * tt[2])) if np.all(np.isfinite(tt)) and np.any(tt != 0) else float("nan")
    t = np.array([tt[0] * inv, tt[1] * inv, tt[2] * inv])
    if np.any(np.isnan(R)) or not is_rotation(R) or not np.all(np.isfinite(t)) or np.all(np.abs(t) <= 1e-3):
        return None
    E = np.zeros(9)
    shim().shim_e_from_rt(_ptr(np.ascontiguousarray(R)), _ptr(t), _ptr(E))
    return R.copy(), t, E


def refine_essential_linear_rt(p1, p2, E, mask, method, R=None, th=0.008, steps=4, th_mult=2.0, ph_mult=0.1, max_loss=0.15, seed=1,
                               solver=eigensolver):
    """-> dict(rc, E, mask, n_inliers, steps_done, rt_valid, R, t, attempts_used, margin) as mlpl_refine_essential_linear_rt returns them
    (R / t None unless rt_valid).  `solver` replaces the eigensolver in tests of the control flow."""
    p1 = np.ascontiguousarray(p1, np.float64)
    p2 = np.ascontiguousarray(p2, np.float64)
    if method & 0xF != PR_KNEIP:
        res = LRO.refine_essential_linear(p1, p2, E, mask, method, th=th, steps=steps, th_mult=th_mult, ph_mult=ph_mult, max_loss=max_loss)
        res.update(rt_valid=False, R=None, t=None, attempts_used=0)
        return res
    E = np.array(E, np.float64).reshape(3, 3)
    mask = np.array(mask, np.uint8).reshape(-1)
    res = dict(rc=MLPL_E_FAILED, E=E.copy(), mask=mask.copy(), n_inliers=0, steps_done=0, rt_valid=False, R=None, t=None, attempts_used=0,
               margin=np.inf)
    cur = np.flatnonzero(mask != 0)
    if cur.size < 6:
        return res
    pts = np.ascontiguousarray(np.concatenate([p1, p2], axis=1))
    f, fp = LRO.bearing(p1), LRO.bearing(p2)
    R_start = np.zeros(9) if R is None else np.array(R, np.float64).reshape(9)
    th2 = th * th
    step_size = (th_mult * th2 - th2) / steps if steps else 0.0
    margin, done, attempts, pose = np.inf, 0, 0, None

    def count(Em, thr):
        nonlocal margin
        err = LRO.sampson_l2(Em, f, fp)
        margin = min(margin, float(np.min(np.abs(err - thr)) / thr))
        return np.flatnonzero(err < thr)

    for j in range(steps):
        need = (1.0 - max_loss) * float(cur.size)
        got = None
        if j == 0 and not is_rotation(R_start):
            raw = glibc_rand(seed, 3 * MAX_SOLS_KNEIP)
            for a in range(MAX_SOLS_KNEIP):
                attempts = a + 1
                s = solve_step(pts, cur, perturbed_identity(raw[3 * a:3 * a + 3]), solver)
                if s is None:
                    continue
                if float(count(s[2], th2).size) < need:
                    continue
                got = s
                break
        else:
            got = solve_step(pts, cur, R_start, solver)
        if got is None:
            break
        Rn, tn, En = got
        nxt = count(En, (th_mult * th2) - (j + 1) * step_size)
        if float(nxt.size) >= need:
            E, cur, done, pose, R_start = En.reshape(3, 3), nxt, done + 1, (Rn.reshape(3, 3), tn), Rn
        elif j == 0:
            res.update(margin=margin, attempts_used=attempts)
            return res
        else:
            break
    m = np.zeros_like(mask)
    m[cur] = 1
    res.update(rc=MLPL_OK, E=np.array(E, np.float64).reshape(3, 3).copy(), mask=m, n_inliers=int(cur.size), steps_done=done, margin=margin,
               attempts_used=attempts, rt_valid=pose is not None, R=None if pose is None else pose[0].copy(),
               t=None if pose is None else pose[1].copy())
    return res


def essential_from_pose(R, t):
    """E = [t / |t|]x R with the bits of dgm::e_from_rt."""
    E = np.zeros(9)
    shim().shim_e_from_rt(_ptr(np.ascontiguousarray(R, np.float64).reshape(9)), _ptr(np.ascontiguousarray(t, np.float64).reshape(3)), _ptr(E))
    return E.reshape(3, 3)


def make_scene(n_list, seed, extra=0.25, bad=0.1, mild_px=2.0, gross=0, rot_deg=5.0):
    """A test problem with n_list starting inliers: synth.pose_scene's motion; a share `bad` of the flagged correspondences carries
    `mild_px` pixels of extra noise in the second image, `gross` of that scene's outliers are flagged as well, `extra` * n_list further
    outliers stay out of the mask -> p1, p2, E0 (of the true pose), mask, R_true, th.  (The solver weighs every listed correspondence
    alike, so a few gross outliers in the list are enough to make step 0 lose too many.)"""
    from matchinglib_poselib_amd import synth

    n_in = n_list - gross
    n_out = gross + max(2, int(round(extra * n_list)))
    n = n_in + n_out
    p1, p2, R, t, inl, th = synth.pose_scene(n, n_in / n, seed=seed, noise_px=0.3, rot_deg=rot_deg)
    rng = np.random.default_rng(seed + 1)
    mild = np.flatnonzero(inl)[:int(round(bad * n_in))]
    p2 = p2.copy()
    p2[mild] += rng.normal(0, mild_px * synth.PIX_TO_CAM, (len(mild), 2))
    mask = inl.astype(np.uint8)
    mask[np.flatnonzero(~inl)[:gross]] = 1
    assert int(mask.sum()) == n_list
    return p1, p2, essential_from_pose(R, t), mask, R, th
