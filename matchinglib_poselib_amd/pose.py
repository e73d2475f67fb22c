"""Host-side mirror of poselib's robust relative-pose entry points (RANSAC path).

Reference interface: poselib/include/poselib/pose_estim.h:192-210 (getPoseTriangPts, estimateEssentialMat),
implementation poselib/source/pose_estim.cpp:857-946 over poselib/source/five-point-nister/*.  Same argument meaning
and failure behaviour; the arithmetic runs in libmlpl_hip.so (HIP, gfx950).  Nothing here computes on the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import Context, MlplError, check, default_context

PIX_MIN_GOOD_TH = 1.6  # poselib/include/poselib/pose_estim.h:59 (pixels; callers of the pose API pass camera-unit thresholds explicitly)


def _pts(p) -> np.ndarray:
    a = np.ascontiguousarray(p, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("points must be an n x 2 array")
    return a


def solve_5pt(p1, p2, samples, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Nister 5-point solver on `samples` (n_samples x 5 indices into p1/p2) -> (E [n_samples,10,3,3], n_models).
    Replaces CvEMEstimator::run5Point (five-point.cpp:366-471)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    samples = np.ascontiguousarray(samples, np.int32)
    ns = samples.shape[0]
    E = np.zeros((ns, 10, 3, 3))
    nm = np.zeros(ns, np.int32)
    check(ctx.lib.mlpl_solve_5pt(ctx.handle, p1.ctypes.data, p2.ctypes.data, p1.shape[0], samples.ctypes.data, ns,
                                 E.ctypes.data, nm.ctypes.data), "mlpl_solve_5pt")
    return E, nm


def score_models(p1, p2, E, thresh: float, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Sampson inlier count and float-error sum per model (findInliers + cv::sum(err), modelest.cpp:69-83,407)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    E = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
    good = np.zeros(E.shape[0], np.int32)
    esum = np.zeros(E.shape[0], np.float64)
    check(ctx.lib.mlpl_score_models(ctx.handle, p1.ctypes.data, p2.ctypes.data, p1.shape[0], E.ctypes.data, E.shape[0],
                                    float(thresh), good.ctypes.data, esum.ctypes.data), "mlpl_score_models")
    return good, esum


def count_models(p1, p2, E, thresh2: float, shape: int = 0, ctx: Optional[Context] = None) -> np.ndarray:
    """Inlier counts by the division-free predicate of the RANSAC passes; thresh2 = squared threshold (modelest.cpp:79)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    E = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
    good = np.zeros(E.shape[0], np.int32)
    check(ctx.lib.mlpl_count_models(ctx.handle, p1.ctypes.data, p2.ctypes.data, p1.shape[0], E.ctypes.data, E.shape[0], float(thresh2),
                                    int(shape), good.ctypes.data), "mlpl_count_models")
    return good


def median_models(p1, p2, E, ctx: Optional[Context] = None) -> np.ndarray:
    """Median Sampson error per model as runLMeDS takes it (modelest.cpp:540-544)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    E = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
    med = np.zeros(E.shape[0], np.float64)
    check(ctx.lib.mlpl_median_models(ctx.handle, p1.ctypes.data, p2.ctypes.data, p1.shape[0], E.ctypes.data, E.shape[0],
                                     med.ctypes.data), "mlpl_median_models")
    return med


def ransac_essential(p1, p2, thresh: float, confidence: float = 0.999, max_iters: int = 1000, refit: bool = True,
                     seed: int = 0, ctx: Optional[Context] = None) -> dict:
    """CvModelEstimator3::runRANSAC with the 5-point kernel (modelest.cpp:343-474); parameters the reference
    hard-codes (1000 iterations, p = 0.999, srand(time)) are explicit here."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    E = np.zeros((3, 3))
    mask = np.zeros(n, np.uint8)
    ninl, iters = C.c_int(0), C.c_int(0)
    rc = ctx.lib.mlpl_ransac_essential(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, float(thresh), float(confidence),
                                       int(max_iters), 1 if refit else 0, int(seed) & 0xFFFFFFFF, E.ctypes.data,
                                       mask.ctypes.data, C.byref(ninl), C.byref(iters))
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_ransac_essential", _lib.last_error())
    return dict(ok=(rc == 0), E=E, mask=mask, n_inliers=ninl.value, iters=iters.value)


def lmeds_essential(p1, p2, confidence: float = 0.999, max_iters: int = 2000, seed: int = 0,
                    ctx: Optional[Context] = None) -> dict:
    """CvModelEstimator3::runLMeDS with the 5-point kernel (modelest.cpp:483-564; findEssentialMat passes 2000 iterations,
    five-point.cpp:127)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    E = np.zeros((3, 3))
    mask = np.zeros(n, np.uint8)
    ninl, med = C.c_int(0), C.c_double(0)
    rc = ctx.lib.mlpl_lmeds_essential(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, float(confidence), int(max_iters),
                                      int(seed) & 0xFFFFFFFF, E.ctypes.data, mask.ctypes.data, C.addressof(ninl),
                                      C.addressof(med))
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_lmeds_essential", _lib.last_error())
    return dict(ok=(rc == 0), E=E, mask=mask, n_inliers=ninl.value, min_median=med.value)


# The reference's ARRSAC samplers draw from two function-local `static cv::RNG rng;` (prosac_sampler.h:115, random_sampler.h:65) that
# live as long as the process: this pair is their mirror for callers that do not keep their own.
ARRSAC_RNG_FRESH = (0xFFFFFFFF, 0xFFFFFFFF)
_arrsac_rng_state = np.array(ARRSAC_RNG_FRESH, np.uint64)


def arrsac_essential(p1, p2, thresh: float, refine: bool = True, rng_state=None, ctx: Optional[Context] = None) -> dict:
    """CvModelEstimator3::runARRSAC (modelest.cpp:197-341) as findEssentialMat(ARRSAC) drives it.  rng_state: uint64[2] array
    (updated in place) = the two cv::RNG states; None = the process-wide pair, as the reference's statics."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    st = _arrsac_rng_state if rng_state is None else rng_state
    assert st.dtype == np.uint64 and st.shape == (2,) and st.flags.c_contiguous
    E = np.zeros((3, 3))
    mask = np.zeros(n, np.uint8)
    ninl = C.c_int(0)
    rc = ctx.lib.mlpl_arrsac_essential(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, float(thresh), 1 if refine else 0, st.ctypes.data,
                                       E.ctypes.data, mask.ctypes.data, C.addressof(ninl))
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_arrsac_essential", _lib.last_error())
    stats = np.zeros(12, np.int64)
    ctx.lib.mlpl_arrsac_last_stats(ctx.handle, stats.ctypes.data)
    return dict(ok=(rc == 0), E=E, mask=mask, n_inliers=ninl.value, stats=stats)


class UsacParams(C.Structure):
    """mlpl_usac_params (include/mlpl_c.h): the configuration estimateEssentialMatUsac builds (usac_estimations.cpp:283-470)."""
    _fields_ = [("th", C.c_double), ("conf", C.c_double), ("max_hyp", C.c_int32), ("estimator", C.c_int32), ("refine", C.c_int32),
                ("seed", C.c_uint32), ("prosac_beta", C.c_double), ("sprt_delta", C.c_double), ("sprt_epsilon", C.c_double),
                ("sprt_mS", C.c_double), ("sprt_tM", C.c_double), ("sorted_idx", C.c_void_p), ("check_degeneracy", C.c_int32),
                ("reserved", C.c_int32), ("th_pixels", C.c_double), ("focal_length", C.c_double)]


def usac_essential(p1, p2, th: float, seed: int, sorted_idx=None, max_hyp: int = 50000, conf: float = 0.99, prosac_beta: float = 0.09,
                   sprt_delta: float = 0.05, sprt_epsilon: float = 0.15, sprt_ms: float = 8.5, sprt_tm: float = 2314.0, estimator: int = 0,
                   refine: int = 0, event_cap: int = 0, check_degeneracy: int = 0, th_pixels: float = 0.8, focal_length: float = 800.0,
                   ctx: Optional[Context] = None) -> dict:
    """estimateEssentialMatUsac with the Nister solver and REF_WEIGHTS (usac_estimations.cpp:283-735) on the device; `seed` is the
    reference's srand(time) seed.  sorted_idx (best match first) switches PROSAC on.  event_cap > 0 also returns the decision trace.
    check_degeneracy: 0 none, 1 the rotation-only / no-motion tests + model upgrade after every new best model (DEGEN_USAC_INTERNAL),
    3 also after every local optimisation; the result then carries `degen` = [1, inliers of the rotation, of "no motion", type],
    `R_degen`, `flags_rot`, `flags_nomot`."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    P = UsacParams()
    ctx.lib.mlpl_usac_default_params(C.addressof(P), float(th))
    P.conf, P.max_hyp, P.estimator, P.refine, P.seed = float(conf), int(max_hyp), int(estimator), int(refine), int(seed) & 0xFFFFFFFF
    P.prosac_beta, P.sprt_delta, P.sprt_epsilon, P.sprt_mS, P.sprt_tM = float(prosac_beta), float(sprt_delta), float(sprt_epsilon), \
        float(sprt_ms), float(sprt_tm)
    P.check_degeneracy, P.th_pixels, P.focal_length = int(check_degeneracy), float(th_pixels), float(focal_length)
    si = None
    if sorted_idx is not None:
        si = np.ascontiguousarray(sorted_idx, np.uint32)
        P.sorted_idx = si.ctypes.data
    E, mask, res = np.zeros(9), np.zeros(n, np.uint8), np.zeros(12)
    ev = np.zeros((max(event_cap, 1), 16))
    if event_cap:
        ctx.lib.mlpl_debug_usac_trace(ctx.handle, ev.ctypes.data, int(event_cap))
    rc = ctx.lib.mlpl_usac_essential(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, C.addressof(P), E.ctypes.data, mask.ctypes.data,
                                     res.ctypes.data)
    nev = ctx.lib.mlpl_debug_usac_trace(ctx.handle, None, 0) if event_cap else 0
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_usac_essential", _lib.last_error())
    stats = np.zeros(8, np.int64)
    ctx.lib.mlpl_usac_last_stats(ctx.handle, stats.ctypes.data)
    out = dict(ok=(rc == 0), E=E, flags=mask, final=res, events=ev[:min(nev, event_cap)], n_events=nev, stats=stats)
    if check_degeneracy and rc == 0:
        info, fr, fn = np.zeros(16), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        check(ctx.lib.mlpl_usac_last_degeneracy(ctx.handle, info.ctypes.data, fr.ctypes.data, fn.ctypes.data, n), "mlpl_usac_last_degeneracy")
        out.update(degen=info[:4].copy(), R_degen=info[4:13].copy(), flags_rot=fr, flags_nomot=fn)
    return out


def arrsac_essential_batch(d_p1, d_p2, counts, thresh: float, refine: bool = True, rng_states=None, masks_out=None, ctx: Optional[Context] = None) -> list:
    """A batch of ARRSAC problems in ONE library call (mlpl_arrsac_essential_batch_dev): d_p1, d_p2 float64 CUDA tensors [B, stride, 2],
    counts[b] valid rows; rng_states: uint64 [B, 2] (default: fresh streams for every problem), advanced in place.  Returns one dict per problem
    (ok, E, n_inliers, rng_state); masks through masks_out (uint8 CUDA tensor [B, stride])."""
    import torch

    ctx = ctx or default_context()
    B, stride = d_p1.shape[0], d_p1.shape[1]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (B, stride, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    cn = np.ascontiguousarray(counts, np.int32)
    st = np.tile(np.array(ARRSAC_RNG_FRESH, np.uint64), (B, 1)) if rng_states is None else rng_states
    assert st.dtype == np.uint64 and st.shape == (B, 2) and st.flags.c_contiguous
    if masks_out is None:
        masks_out = torch.zeros((B, stride), dtype=torch.uint8, device=d_p1.device)
    assert masks_out.is_cuda and masks_out.dtype == torch.uint8 and masks_out.shape == (B, stride) and masks_out.is_contiguous()
    E, ninl, status = np.zeros((B, 9)), np.zeros(B, np.int32), np.zeros(B, np.int32)
    rc = ctx.lib.mlpl_arrsac_essential_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, float(thresh), 1 if refine else 0,
                                                 st.ctypes.data, E.ctypes.data, masks_out.data_ptr(), ninl.ctypes.data, status.ctypes.data,
                                                 torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_arrsac_essential_batch_dev", _lib.last_error())
    return [dict(ok=bool(status[b] == 0), E=E[b].copy(), n_inliers=int(ninl[b]), rng_state=st[b].copy()) for b in range(B)]


def usac_essential_batch(d_p1, d_p2, counts, th: float, seeds, sorted_idx=None, max_hyp: int = 50000, conf: float = 0.99, prosac_beta: float = 0.09,
                         sprt_delta: float = 0.05, sprt_epsilon: float = 0.15, sprt_ms: float = 8.5, sprt_tm: float = 2314.0, estimator: int = 0,
                         refine: int = 0, event_cap: int = 0, check_degeneracy: int = 0, th_pixels: float = 0.8, focal_length: float = 800.0,
                         masks_out=None, ctx: Optional[Context] = None) -> list:
    """A batch of USAC problems in ONE library call (mlpl_usac_essential_batch_dev): d_p1, d_p2 float64 CUDA tensors [B, stride, 2],
    counts[b] valid rows, seeds[b]; sorted_idx: None or a list of per-problem PROSAC orders (None entries = uniform sampling).  Returns one
    dict per problem with the keys of usac_essential (ok, E, final, events, n_events, degen ...; flags only through masks_out, a uint8
    CUDA tensor [B, stride])."""
    import torch

    ctx = ctx or default_context()
    B, stride = d_p1.shape[0], d_p1.shape[1]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (B, stride, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    cn = np.ascontiguousarray(counts, np.int32)
    P = (UsacParams * B)()
    keep = []
    for b in range(B):
        ctx.lib.mlpl_usac_default_params(C.addressof(P[b]), float(th))
        P[b].conf, P[b].max_hyp, P[b].estimator, P[b].refine, P[b].seed = float(conf), int(max_hyp), int(estimator), int(refine), int(seeds[b]) & 0xFFFFFFFF
        P[b].prosac_beta, P[b].sprt_delta, P[b].sprt_epsilon, P[b].sprt_mS, P[b].sprt_tM = float(prosac_beta), float(sprt_delta), float(sprt_epsilon), \
            float(sprt_ms), float(sprt_tm)
        P[b].check_degeneracy, P[b].th_pixels, P[b].focal_length = int(check_degeneracy), float(th_pixels), float(focal_length)
        if sorted_idx is not None and sorted_idx[b] is not None:
            si = np.ascontiguousarray(sorted_idx[b], np.uint32)
            keep.append(si)
            P[b].sorted_idx = si.ctypes.data
    E, res, status, degen = np.zeros((B, 9)), np.zeros((B, 12)), np.zeros(B, np.int32), np.zeros((B, 16))
    ev = np.zeros((B, max(event_cap, 1), 16))
    lens = np.zeros(B, np.int32)
    if masks_out is not None:
        assert masks_out.is_cuda and masks_out.dtype == torch.uint8 and masks_out.shape == (B, stride) and masks_out.is_contiguous()
    st = torch.cuda.current_stream(d_p1.device).cuda_stream
    rc = ctx.lib.mlpl_usac_essential_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, C.addressof(P), E.ctypes.data,
                                               masks_out.data_ptr() if masks_out is not None else None, res.ctypes.data, status.ctypes.data,
                                               degen.ctypes.data, ev.ctypes.data if event_cap else None, int(event_cap), lens.ctypes.data if event_cap else None, st)
    if rc != 0:
        raise MlplError(rc, "mlpl_usac_essential_batch_dev", _lib.last_error())
    stats = np.zeros(8, np.int64)
    ctx.lib.mlpl_usac_last_stats(ctx.handle, stats.ctypes.data)
    out = []
    for b in range(B):
        if status[b] not in (0, _lib.MLPL_E_FAILED):
            raise MlplError(int(status[b]), "mlpl_usac_essential_batch_dev", f"problem {b}")
        out.append(dict(ok=bool(status[b] == 0), E=E[b].copy(), final=res[b].copy(), events=ev[b, :min(int(lens[b]), event_cap)].copy(), n_events=int(lens[b]),
                        degen=degen[b, :4].copy(), R_degen=degen[b, 4:13].copy(), stats=stats))
    return out


def arrsac_sample_models(p1, p2, idx, kind: int, thresh: float = 1e-3, ctx: Optional[Context] = None):
    """ARRSAC's estimators on one sample (modelest.cpp:111-178) -> (models [k,3,3] before the validity filter, valid flags [k])."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    idx = np.ascontiguousarray(idx, np.int32)
    E = np.zeros((10, 3, 3))
    nm = C.c_int(0)
    valid = np.zeros(10, np.uint8)
    check(ctx.lib.mlpl_arrsac_sample_models(ctx.handle, p1.ctypes.data, p2.ctypes.data, p1.shape[0], idx.ctypes.data, len(idx), int(kind),
                                            float(thresh), E.ctypes.data, C.addressof(nm), valid.ctypes.data), "mlpl_arrsac_sample_models")
    return E[: nm.value].copy(), valid[: nm.value].astype(bool)


def robust_essential_refine(p1, p2, E_init, th: float, mask=None, ctx: Optional[Context] = None):
    """poselib::robustEssentialRefine for the essential-matrix model (pose_estim.cpp:337-792) -> (E_refined, rounds, status)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    E0 = np.ascontiguousarray(E_init, np.float64).reshape(3, 3)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    E = np.zeros((3, 3))
    info = np.zeros(2, np.int32)
    check(ctx.lib.mlpl_robust_essential_refine(ctx.handle, p1.ctypes.data, p2.ctypes.data, p1.shape[0], None if m is None else m.ctypes.data,
                                               E0.ctypes.data, float(th), E.ctypes.data, info.ctypes.data), "mlpl_robust_essential_refine")
    return E, int(info[0]), int(info[1])


# poselib::RefinePostAlg (P/include/poselib/pose_estim.h:79-88): a solver nibble OR-ed with a weighting
PR_8PT, PR_NISTER, PR_STEWENIUS, PR_KNEIP = 0x1, 0x2, 0x3, 0x4
PR_TORR_WEIGHTS, PR_PSEUDOHUBER_WEIGHTS, PR_NO_WEIGHTS = 0x10, 0x20, 0x30


def refine_essential_linear(p1, p2, E, mask, refine_method: int = PR_8PT | PR_PSEUDOHUBER_WEIGHTS, th: float = 0.008, num_iterative_steps: int = 4,
                            threshold_multiplier: float = 2.0, pseudo_huber_threshold_multiplier: float = 0.1,
                            max_relative_inlier_cnt_loss: float = 0.15, ctx: Optional[Context] = None) -> dict:
    """poselib::refineEssentialLinear (pose_linear_refinement.cpp:85-309) -> dict(ok, E, mask, n_inliers, steps_done).  ok = False is the
    reference's false (E and mask returned unchanged); PR_KNEIP raises MlplError(MLPL_E_UNSUPPORTED), PR_8PT with weight bits other than
    0x10 / 0x20 / 0x30 MlplError(MLPL_E_BAD_INPUT)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    if p2.shape[0] != n:
        raise ValueError("p1 and p2 differ in length")
    E_io = np.array(E, np.float64).reshape(3, 3).copy()
    m = np.array(mask, np.uint8).reshape(-1).copy()
    if m.shape[0] != n:
        raise ValueError("the mask must hold one byte per correspondence")
    ninl, done = C.c_int(0), C.c_int(0)
    rc = ctx.lib.mlpl_refine_essential_linear(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, int(refine_method), float(th), int(num_iterative_steps),
                                              float(threshold_multiplier), float(pseudo_huber_threshold_multiplier),
                                              float(max_relative_inlier_cnt_loss), E_io.ctypes.data, m.ctypes.data, C.byref(ninl), C.byref(done))
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_refine_essential_linear", _lib.last_error())
    return dict(ok=(rc == 0), E=E_io, mask=m, n_inliers=ninl.value if rc == 0 else 0, steps_done=done.value if rc == 0 else 0)


def refine_essential_linear_batch(d_p1, d_p2, counts, E, d_masks, th, refine_method: int = PR_8PT | PR_PSEUDOHUBER_WEIGHTS,
                                  num_iterative_steps: int = 4, threshold_multiplier: float = 2.0, pseudo_huber_threshold_multiplier: float = 0.1,
                                  max_relative_inlier_cnt_loss: float = 0.15, ctx: Optional[Context] = None) -> dict:
    """mlpl_refine_essential_linear_batch_dev: d_p1, d_p2 float64 CUDA tensors [B, stride, 2], counts[b] valid rows, E float64 [B, 9] or
    [B, 3, 3] (host), d_masks uint8 CUDA tensor [B, stride] (refined in place), th a scalar or one per problem.  One launch for the batch.
    Returns dict(status int32 [B] (0 or MLPL_E_FAILED), E [B, 3, 3], n_inliers [B], steps_done [B])."""
    import torch

    B, stride = d_p1.shape[0], d_p1.shape[1]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (B, stride, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    assert d_masks.is_cuda and d_masks.dtype == torch.uint8 and d_masks.shape == (B, stride) and d_masks.is_contiguous()
    ctx = ctx or default_context(d_p1.device.index or 0)
    cn = np.ascontiguousarray(counts, np.int32).reshape(B)
    thv = np.ascontiguousarray(np.broadcast_to(np.asarray(th, np.float64), (B,)))
    E_io = np.array(E, np.float64).reshape(B, 9).copy()
    ninl, status, done = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    rc = ctx.lib.mlpl_refine_essential_linear_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, thv.ctypes.data,
                                                        int(refine_method), int(num_iterative_steps), float(threshold_multiplier),
                                                        float(pseudo_huber_threshold_multiplier), float(max_relative_inlier_cnt_loss), E_io.ctypes.data,
                                                        d_masks.data_ptr(), ninl.ctypes.data, status.ctypes.data, done.ctypes.data,
                                                        torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_refine_essential_linear_batch_dev", _lib.last_error())
    return dict(status=status, E=E_io.reshape(B, 3, 3), n_inliers=ninl, steps_done=done)


def refine_essential_linear_rt(p1, p2, E, mask, refine_method: int = PR_KNEIP | PR_PSEUDOHUBER_WEIGHTS, R=None, th: float = 0.008,
                               num_iterative_steps: int = 4, threshold_multiplier: float = 2.0, pseudo_huber_threshold_multiplier: float = 0.1,
                               max_relative_inlier_cnt_loss: float = 0.15, seed: int = 1, ctx: Optional[Context] = None) -> dict:
    """mlpl_refine_essential_linear_rt: refineEssentialLinear with R and t, i.e. with PR_KNEIP (OpenGV's eigensolver) among the solvers.
    R = a start rotation or None (the reference's empty R: up to 12 perturbed-identity starts drawn from srand(seed)).  Returns
    dict(ok, E, mask, n_inliers, steps_done, rt_valid, R, t, attempts_used); R / t are None unless rt_valid (the reference clears R)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    if p2.shape[0] != n:
        raise ValueError("p1 and p2 differ in length")
    E_io = np.array(E, np.float64).reshape(3, 3).copy()
    m = np.array(mask, np.uint8).reshape(-1).copy()
    if m.shape[0] != n:
        raise ValueError("the mask must hold one byte per correspondence")
    R_io = np.zeros((3, 3)) if R is None else np.array(R, np.float64).reshape(3, 3).copy()
    t_io = np.zeros(3)
    ninl, done, valid, used = C.c_int(0), C.c_int(0), C.c_int(0 if R is None else 1), C.c_int(0)
    rc = ctx.lib.mlpl_refine_essential_linear_rt(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, int(refine_method), float(th), int(num_iterative_steps),
                                                 float(threshold_multiplier), float(pseudo_huber_threshold_multiplier),
                                                 float(max_relative_inlier_cnt_loss), E_io.ctypes.data, m.ctypes.data, C.byref(ninl), C.byref(done),
                                                 R_io.ctypes.data, t_io.ctypes.data, C.byref(valid), int(seed) & 0xFFFFFFFF, C.byref(used))
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_refine_essential_linear_rt", _lib.last_error())
    ok = rc == 0
    posed = ok and valid.value != 0
    return dict(ok=ok, E=E_io, mask=m, n_inliers=ninl.value if ok else 0, steps_done=done.value if ok else 0, rt_valid=posed,
                R=R_io if posed else None, t=t_io if posed else None, attempts_used=used.value)


def refine_essential_linear_rt_batch(d_p1, d_p2, counts, E, d_masks, th, refine_method: int = PR_KNEIP | PR_PSEUDOHUBER_WEIGHTS, R=None, rt_valid=None,
                                     seeds=None, num_iterative_steps: int = 4, threshold_multiplier: float = 2.0,
                                     pseudo_huber_threshold_multiplier: float = 0.1, max_relative_inlier_cnt_loss: float = 0.15,
                                     ctx: Optional[Context] = None) -> dict:
    """mlpl_refine_essential_linear_rt_batch_dev in the layout of refine_essential_linear_batch.  R: [B, 3, 3] start rotations (host) with
    rt_valid [B] saying which of them count (None: all when R is given, none otherwise); seeds [B] or None (1).  Returns dict(status, E,
    n_inliers, steps_done, R [B, 3, 3], t [B, 3], rt_valid [B], attempts_used [B]); R[b] / t[b] are what was passed in / zero unless rt_valid[b]."""
    import torch

    B, stride = d_p1.shape[0], d_p1.shape[1]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (B, stride, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    assert d_masks.is_cuda and d_masks.dtype == torch.uint8 and d_masks.shape == (B, stride) and d_masks.is_contiguous()
    ctx = ctx or default_context(d_p1.device.index or 0)
    cn = np.ascontiguousarray(counts, np.int32).reshape(B)
    thv = np.ascontiguousarray(np.broadcast_to(np.asarray(th, np.float64), (B,)))
    E_io = np.array(E, np.float64).reshape(B, 9).copy()
    R_io = np.zeros((B, 9)) if R is None else np.array(R, np.float64).reshape(B, 9).copy()
    valid = np.full(B, 0 if R is None else 1, np.int32) if rt_valid is None else np.array(rt_valid, np.int32).reshape(B).copy()
    sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, np.int64) & 0xFFFFFFFF, np.uint32).reshape(B)
    t_io = np.zeros((B, 3))
    ninl, status, done, used = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    rc = ctx.lib.mlpl_refine_essential_linear_rt_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, thv.ctypes.data,
                                                           int(refine_method), int(num_iterative_steps), float(threshold_multiplier),
                                                           float(pseudo_huber_threshold_multiplier), float(max_relative_inlier_cnt_loss),
                                                           E_io.ctypes.data, d_masks.data_ptr(), ninl.ctypes.data, status.ctypes.data, done.ctypes.data,
                                                           R_io.ctypes.data, t_io.ctypes.data, valid.ctypes.data, None if sd is None else sd.ctypes.data,
                                                           used.ctypes.data, torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_refine_essential_linear_rt_batch_dev", _lib.last_error())
    return dict(status=status, E=E_io.reshape(B, 3, 3), n_inliers=ninl, steps_done=done, R=R_io.reshape(B, 3, 3), t=t_io, rt_valid=valid,
                attempts_used=used)


def kneip_refine_times(ctx: Context, enable: int = -1) -> dict:
    """mlpl_kneip_refine_times: switch the per-part timing of the PR_KNEIP refinement on / off (enable 1 / 0; -1 leaves it) and return the
    last call's split in seconds: dict(sums, solve, eval, hops)."""
    out = np.zeros(4)
    rc = ctx.lib.mlpl_kneip_refine_times(ctx.handle, int(enable), out.ctypes.data)
    if rc != 0:
        raise MlplError(rc, "mlpl_kneip_refine_times", _lib.last_error())
    return dict(sums=float(out[0]), solve=float(out[1]), eval=float(out[2]), hops=float(out[3]))


def recover_pose_batch(d_p1, d_p2, counts, E, d_masks=None, dist: float = 50.0, ctx: Optional[Context] = None) -> dict:
    """mlpl_recover_pose_batch_dev: the cheirality step (getPoseTriangPts without points) for a batch in the layout above; d_masks (uint8 CUDA
    tensor [B, stride] or None = all points) receives the chosen candidate's mask.  Returns dict(n_good [B], R [B, 3, 3], t [B, 3])."""
    import torch

    B, stride = d_p1.shape[0], d_p1.shape[1]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (B, stride, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    if d_masks is not None:
        assert d_masks.is_cuda and d_masks.dtype == torch.uint8 and d_masks.shape == (B, stride) and d_masks.is_contiguous()
    ctx = ctx or default_context(d_p1.device.index or 0)
    cn = np.ascontiguousarray(counts, np.int32).reshape(B)
    Eh = np.ascontiguousarray(np.asarray(E, np.float64).reshape(B, 9))
    n_good, R, t = np.zeros(B, np.int32), np.zeros((B, 3, 3)), np.zeros((B, 3))
    rc = ctx.lib.mlpl_recover_pose_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, Eh.ctypes.data, float(dist),
                                             None if d_masks is None else d_masks.data_ptr(), n_good.ctypes.data, R.ctypes.data, t.ctypes.data,
                                             torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_recover_pose_batch_dev", _lib.last_error())
    return dict(n_good=n_good, R=R, t=t)


def ransac_essential_device(p1, p2, thresh: float, confidence: float = 0.999, max_iters: int = 1000, refit: bool = True,
                            seed: int = 0, ctx: Optional[Context] = None, mask_out=None, stream: Optional[int] = None) -> dict:
    """Same as ransac_essential on device-resident torch tensors (float64 [n,2]); the mask stays on the device."""
    import torch

    assert p1.is_cuda and p2.is_cuda and p1.dtype == torch.float64 and p1.is_contiguous() and p2.is_contiguous()
    ctx = ctx or default_context(p1.device.index or 0)
    n = p1.shape[0]
    if mask_out is None:
        mask_out = torch.empty(n, dtype=torch.uint8, device=p1.device)
    E = np.zeros((3, 3))
    ninl, iters = C.c_int(0), C.c_int(0)
    st = torch.cuda.current_stream(p1.device).cuda_stream if stream is None else stream
    rc = ctx.lib.mlpl_ransac_essential_dev(ctx.handle, p1.data_ptr(), p2.data_ptr(), n, float(thresh), float(confidence),
                                           int(max_iters), 1 if refit else 0, int(seed) & 0xFFFFFFFF, E.ctypes.data,
                                           mask_out.data_ptr(), C.byref(ninl), C.byref(iters), st)
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_ransac_essential_dev", _lib.last_error())
    return dict(ok=(rc == 0), E=E, mask=mask_out, n_inliers=ninl.value, iters=iters.value)


def arrsac_essential_device(p1, p2, thresh: float, refine: bool = True, rng_state=None, ctx: Optional[Context] = None, mask_out=None,
                            stream: Optional[int] = None) -> dict:
    """Same as arrsac_essential on device-resident torch tensors (float64 [n,2]); the mask stays on the device."""
    import torch

    assert p1.is_cuda and p2.is_cuda and p1.dtype == torch.float64 and p1.is_contiguous() and p2.is_contiguous()
    ctx = ctx or default_context(p1.device.index or 0)
    n = p1.shape[0]
    if mask_out is None:
        mask_out = torch.empty(n, dtype=torch.uint8, device=p1.device)
    st = _arrsac_rng_state if rng_state is None else rng_state
    E = np.zeros((3, 3))
    ninl = C.c_int(0)
    sm = torch.cuda.current_stream(p1.device).cuda_stream if stream is None else stream
    rc = ctx.lib.mlpl_arrsac_essential_dev(ctx.handle, p1.data_ptr(), p2.data_ptr(), n, float(thresh), 1 if refine else 0, st.ctypes.data,
                                           E.ctypes.data, mask_out.data_ptr(), C.addressof(ninl), sm)
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_arrsac_essential_dev", _lib.last_error())
    return dict(ok=(rc == 0), E=E, mask=mask_out, n_inliers=ninl.value)


def _rng_pair(rng_state):
    st = _arrsac_rng_state if rng_state is None else rng_state
    assert st.dtype == np.uint64 and st.shape == (2,) and st.flags.c_contiguous
    return st


def homography_arrsac(p1, p2, th: float, rng_state=None, ctx: Optional[Context] = None) -> dict:
    """poselib::computeHomographyArrsac (pose_homography.cpp:478-555): ARRSAC over the 4-point DLT, findHomographyInliers, refineHomography.
    rng_state as in arrsac_essential: the SAME two cv::RNG streams (the reference's samplers are shared by both estimators).
    ok = False is the reference's `false`."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    st = _rng_pair(rng_state)
    H, mask, ninl, stats = np.zeros((3, 3)), np.zeros(max(n, 1), np.uint8), C.c_int(0), np.zeros(12, np.int64)
    rc = ctx.lib.mlpl_homography_arrsac(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, float(th), st.ctypes.data, H.ctypes.data, mask.ctypes.data,
                                        C.addressof(ninl), stats.ctypes.data)
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_homography_arrsac", _lib.last_error())
    return dict(ok=(rc == 0), H=H, mask=mask[:n], n_inliers=ninl.value, stats=stats)


def homography_arrsac_device(p1, p2, th: float, rng_state=None, ctx: Optional[Context] = None, mask_out=None, stream: Optional[int] = None) -> dict:
    """homography_arrsac on device-resident torch tensors (float64 [n,2]); the mask stays on the device."""
    import torch

    assert p1.is_cuda and p2.is_cuda and p1.dtype == torch.float64 and p1.is_contiguous() and p2.is_contiguous()
    ctx = ctx or default_context(p1.device.index or 0)
    n = p1.shape[0]
    if mask_out is None:
        mask_out = torch.empty(max(n, 1), dtype=torch.uint8, device=p1.device)
    st = _rng_pair(rng_state)
    H, ninl, stats = np.zeros((3, 3)), C.c_int(0), np.zeros(12, np.int64)
    sm = torch.cuda.current_stream(p1.device).cuda_stream if stream is None else stream
    rc = ctx.lib.mlpl_homography_arrsac_dev(ctx.handle, p1.data_ptr(), p2.data_ptr(), n, float(th), st.ctypes.data, H.ctypes.data,
                                            mask_out.data_ptr(), C.addressof(ninl), stats.ctypes.data, sm)
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_homography_arrsac_dev", _lib.last_error())
    return dict(ok=(rc == 0), H=H, mask=mask_out[:n], n_inliers=ninl.value, stats=stats)


def homography_inliers(p1, p2, H, th: float, ctx: Optional[Context] = None):
    """findHomographyInliers (pose_homography.cpp:785-813): (mask, count) with mask[i] = transfer error <= th^2."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    H = np.ascontiguousarray(H, np.float64).reshape(3, 3)
    mask, ninl = np.zeros(n, np.uint8), C.c_int(0)
    check(ctx.lib.mlpl_homography_inliers(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, H.ctypes.data, float(th), mask.ctypes.data,
                                          C.addressof(ninl)), "mlpl_homography_inliers")
    return mask, ninl.value


def _plane_cap(n: int, min_pts_per_plane: int, max_planes: int) -> int:
    """The most planes a call can report: every one holds at least max(min_pts_per_plane, 1) correspondences of its own."""
    cap = n // max(int(min_pts_per_plane), 1) + 1
    return min(cap, int(max_planes)) if max_planes else cap


def mult_homographies(p1, p2, th: float, var_th: bool = True, max_planes: int = 0, min_pts_per_plane: int = 4, rng_state=None, cap=None,
                      want_masks: bool = True, ctx: Optional[Context] = None) -> dict:
    """poselib::estimateMultHomographys (pose_homography.cpp:291-463): rc = 0 / -1 as the reference; the planes in its output order
    (by inlier count, descending, when more than one was found); masks in the original indexing, built from one label per
    correspondence (labels: output plane or -1); found_at: the round that found each plane (ascending = order of discovery).
    cap (planes the arrays hold) defaults to the most a call can report."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    st = _rng_pair(rng_state)
    cap = _plane_cap(n, min_pts_per_plane, max_planes) if cap is None else int(cap)
    npl = C.c_int(0)
    H, num, strength, thu = np.zeros((max(cap, 1), 3, 3)), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
    found, labels = np.zeros(max(cap, 1), np.int32), np.full(max(n, 1), -1, np.int32)
    check(ctx.lib.mlpl_mult_homographies_labels(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, float(th), 1 if var_th else 0, int(max_planes),
                                                int(min_pts_per_plane), st.ctypes.data, cap, C.addressof(npl), H.ctypes.data, num.ctypes.data,
                                                strength.ctypes.data, thu.ctypes.data, found.ctypes.data,
                                                labels.ctypes.data if want_masks else None, None), "mlpl_mult_homographies_labels")
    k = max(npl.value, 0)
    out = dict(rc=-1 if npl.value < 0 else 0, n_planes=k, H=H[:k].copy(), num_inl=num[:k].copy(), strength=strength[:k].copy(),
               th_used=thu[:k].copy(), found_at=found[:k].copy())
    if want_masks:
        out["labels"] = labels[:n]
        out["masks"] = (labels[None, :n] == np.arange(k, dtype=np.int32)[:, None]).astype(np.uint8)
    return out


def mult_homographies_device(p1, p2, th: float, var_th: bool = True, max_planes: int = 0, min_pts_per_plane: int = 4, rng_state=None, cap=None,
                             ctx: Optional[Context] = None, stream: Optional[int] = None) -> dict:
    """mult_homographies on device-resident torch tensors (float64 [n,2]); the labels ([n] int32) and the masks ([n_planes, n] uint8)
    stay on the device."""
    import torch

    assert p1.is_cuda and p2.is_cuda and p1.dtype == torch.float64 and p1.is_contiguous() and p2.is_contiguous()
    ctx = ctx or default_context(p1.device.index or 0)
    n = p1.shape[0]
    st = _rng_pair(rng_state)
    cap = _plane_cap(n, min_pts_per_plane, max_planes) if cap is None else int(cap)
    npl = C.c_int(0)
    H, num, strength, thu = np.zeros((max(cap, 1), 3, 3)), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
    found = np.zeros(max(cap, 1), np.int32)
    labels = torch.full((max(n, 1),), -1, dtype=torch.int32, device=p1.device)
    sm = torch.cuda.current_stream(p1.device).cuda_stream if stream is None else stream
    check(ctx.lib.mlpl_mult_homographies_labels_dev(ctx.handle, p1.data_ptr(), p2.data_ptr(), n, float(th), 1 if var_th else 0, int(max_planes),
                                                    int(min_pts_per_plane), st.ctypes.data, cap, C.addressof(npl), H.ctypes.data, num.ctypes.data,
                                                    strength.ctypes.data, thu.ctypes.data, found.ctypes.data, labels.data_ptr(), None, sm),
          "mlpl_mult_homographies_labels_dev")
    k = max(npl.value, 0)
    masks = (labels[None, :n] == torch.arange(k, dtype=torch.int32, device=p1.device)[:, None]).to(torch.uint8)
    return dict(rc=-1 if npl.value < 0 else 0, n_planes=k, H=H[:k].copy(), num_inl=num[:k].copy(), strength=strength[:k].copy(),
                th_used=thu[:k].copy(), found_at=found[:k].copy(), labels=labels[:n], masks=masks)


def _plane_batch_inputs(d_p1, d_p2, counts, rng_states):
    import torch

    B, stride = d_p1.shape[0], d_p1.shape[1]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (B, stride, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    cn = np.ascontiguousarray(counts, np.int32)
    assert cn.shape == (B,)
    st = np.tile(np.array(ARRSAC_RNG_FRESH, np.uint64), (B, 1)) if rng_states is None else rng_states
    assert st.dtype == np.uint64 and st.shape == (B, 2) and st.flags.c_contiguous
    return B, stride, cn, st


def homography_arrsac_batch(d_p1, d_p2, counts, th: float, rng_states=None, masks_out=None, ctx: Optional[Context] = None) -> list:
    """A batch of computeHomographyArrsac problems in ONE library call (mlpl_homography_arrsac_batch_dev): d_p1, d_p2 float64 CUDA tensors
    [B, stride, 2], counts[b] valid rows; rng_states: uint64 [B, 2] (default: fresh streams for every problem), advanced in place.  Returns
    one dict per problem (ok, H, n_inliers, stats, rng_state) -- what homography_arrsac_device returns for it alone; masks through
    masks_out (uint8 CUDA tensor [B, stride])."""
    import torch

    ctx = ctx or default_context()
    B, stride, cn, st = _plane_batch_inputs(d_p1, d_p2, counts, rng_states)
    if masks_out is None:
        masks_out = torch.zeros((B, stride), dtype=torch.uint8, device=d_p1.device)
    assert masks_out.is_cuda and masks_out.dtype == torch.uint8 and masks_out.shape == (B, stride) and masks_out.is_contiguous()
    H, ninl, status, stats = np.zeros((B, 3, 3)), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 12), np.int64)
    rc = ctx.lib.mlpl_homography_arrsac_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, float(th), st.ctypes.data,
                                                  H.ctypes.data, masks_out.data_ptr(), ninl.ctypes.data, status.ctypes.data, stats.ctypes.data,
                                                  torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_homography_arrsac_batch_dev", _lib.last_error())
    return [dict(ok=bool(status[b] == 0), H=H[b].copy(), n_inliers=int(ninl[b]), stats=stats[b].copy(), rng_state=st[b].copy()) for b in range(B)]


def mult_homographies_batch(d_p1, d_p2, counts, th: float, var_th: bool = True, max_planes: int = 0, min_pts_per_plane: int = 4, rng_states=None,
                            cap=None, labels_out=None, ctx: Optional[Context] = None) -> list:
    """A batch of estimateMultHomographys problems in ONE library call (mlpl_mult_homographies_batch_dev), inputs as homography_arrsac_batch.
    cap (planes the arrays hold per problem) defaults to the most the largest problem can report.  Returns one dict per problem with the
    keys of mult_homographies_device (rc, n_planes, H, num_inl, strength, th_used, found_at) plus ok (False: fewer than 4 correspondences)
    and rng_state; labels through labels_out (int32 CUDA tensor [B, stride]: output plane or -1 over counts[b])."""
    import torch

    ctx = ctx or default_context()
    B, stride, cn, st = _plane_batch_inputs(d_p1, d_p2, counts, rng_states)
    cap = max(_plane_cap(int(cn.max()) if B else 0, min_pts_per_plane, max_planes), 1) if cap is None else int(cap)
    if labels_out is None:
        labels_out = torch.full((B, stride), -1, dtype=torch.int32, device=d_p1.device)
    assert labels_out.is_cuda and labels_out.dtype == torch.int32 and labels_out.shape == (B, stride) and labels_out.is_contiguous()
    c1 = max(cap, 1)
    npl, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    H, num, strength, thu, found = np.zeros((B, c1, 3, 3)), np.zeros((B, c1), np.int32), np.zeros((B, c1)), np.zeros((B, c1)), np.zeros((B, c1), np.int32)
    rc = ctx.lib.mlpl_mult_homographies_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, float(th), 1 if var_th else 0,
                                                  int(max_planes), int(min_pts_per_plane), st.ctypes.data, cap, npl.ctypes.data, H.ctypes.data,
                                                  num.ctypes.data, strength.ctypes.data, thu.ctypes.data, found.ctypes.data, labels_out.data_ptr(),
                                                  status.ctypes.data, torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_mult_homographies_batch_dev", _lib.last_error())
    out = []
    for b in range(B):
        k = max(int(npl[b]), 0)
        out.append(dict(ok=bool(status[b] == 0), rc=-1 if npl[b] < 0 else 0, n_planes=k, H=H[b, :k].copy(), num_inl=num[b, :k].copy(),
                        strength=strength[b, :k].copy(), th_used=thu[b, :k].copy(), found_at=found[b, :k].copy(), rng_state=st[b].copy()))
    return out


POSE_HOM_MAX_PLANES = 50   # MAX_PLANES_PER_PAIR of the reference's pose_homography.cpp


def homography_alignment(p1, p2, labels, n_planes: int, num_inl, H0, tol: float, ctx: Optional[Context] = None) -> dict:
    """Homographys_Alignment and its caller's part (mlpl_homography_alignment): the pose from labelled plane correspondences, no plane
    search inside.  code = 0 or -3; with 0: R, t, E, norms [n_planes, 3], Hs [n_planes, 3, 3]; info = the 24 doubles of mlpl_c.h."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n, P = p1.shape[0], int(n_planes)
    labels = np.ascontiguousarray(labels, np.int32)
    num = np.ascontiguousarray(num_inl, np.int32)
    assert labels.shape == (n,) and num.shape == (P,)
    H0 = np.ascontiguousarray(H0, np.float64).reshape(3, 3)
    R, t, E, info = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3)), np.zeros(24)
    norms, Hs = np.zeros((max(P, 1), 3)), np.zeros((max(P, 1), 3, 3))
    check(ctx.lib.mlpl_homography_alignment(ctx.handle, p1.ctypes.data, p2.ctypes.data, labels.ctypes.data, n, P, num.ctypes.data if P else labels.ctypes.data,
                                            H0.ctypes.data, float(tol), R.ctypes.data, t.ctypes.data, E.ctypes.data, norms.ctypes.data, Hs.ctypes.data,
                                            info.ctypes.data), "mlpl_homography_alignment")
    return dict(code=int(info[0]), R=R, t=t, E=E, norms=norms[:P], Hs=Hs[:P], info=info)


def _pose_hom_result(result, R, t, E, ninl, npl, H, num, strength, info):
    k = max(npl.value, 0)
    return dict(result=result.value, R=R, t=t, E=E, n_inliers=ninl.value, n_planes=npl.value, H=H[:k].copy(), num_inl=num[:k].copy(),
                strength=strength[:k].copy(), info=info)


def pose_homographies(p1, p2, th: float, mask=None, check_plane_strength: bool = False, var_th: bool = False, rng_state=None,
                      ctx: Optional[Context] = None) -> dict:
    """poselib::estimatePoseHomographies (mlpl_pose_homographies): result = 0 / -1 / -2 / -3 as the reference; with 0: R, t, E, the strict
    mask over all rows and n_inliers.  n_planes, H, num_inl, strength describe the planes found; labels: the plane of every row the input
    mask kept (in the kept rows' order)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    st = _rng_pair(rng_state)
    m_in = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, np.uint8)
    assert m_in is None or m_in.shape == (n,)
    cap = POSE_HOM_MAX_PLANES
    result, ninl, npl = C.c_int(0), C.c_int(0), C.c_int(0)
    R, t, E, info = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3)), np.zeros(24)
    H, num, strength = np.zeros((cap, 3, 3)), np.zeros(cap, np.int32), np.zeros(cap)
    mask_out, labels = np.zeros(max(n, 1), np.uint8), np.full(max(n, 1), -1, np.int32)
    check(ctx.lib.mlpl_pose_homographies(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, None if m_in is None else m_in.ctypes.data, float(th),
                                         1 if check_plane_strength else 0, 1 if var_th else 0, st.ctypes.data, C.addressof(result), R.ctypes.data,
                                         t.ctypes.data, E.ctypes.data, C.addressof(ninl), mask_out.ctypes.data, cap, C.addressof(npl), H.ctypes.data,
                                         num.ctypes.data, strength.ctypes.data, labels.ctypes.data, info.ctypes.data), "mlpl_pose_homographies")
    out = _pose_hom_result(result, R, t, E, ninl, npl, H, num, strength, info)
    kept = n if m_in is None else int(m_in.sum())
    out.update(mask=mask_out[:n], labels=labels[:kept])
    return out


def pose_homographies_device(p1, p2, th: float, mask=None, check_plane_strength: bool = False, var_th: bool = False, rng_state=None,
                             ctx: Optional[Context] = None, stream: Optional[int] = None) -> dict:
    """pose_homographies on device-resident torch tensors (float64 [n,2]; mask: uint8 [n] or None); the output mask and the labels stay on
    the device."""
    import torch

    assert p1.is_cuda and p2.is_cuda and p1.dtype == torch.float64 and p1.is_contiguous() and p2.is_contiguous()
    assert mask is None or (mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.shape == (p1.shape[0],))
    ctx = ctx or default_context(p1.device.index or 0)
    n = p1.shape[0]
    st = _rng_pair(rng_state)
    cap = POSE_HOM_MAX_PLANES
    result, ninl, npl = C.c_int(0), C.c_int(0), C.c_int(0)
    R, t, E, info = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3)), np.zeros(24)
    H, num, strength = np.zeros((cap, 3, 3)), np.zeros(cap, np.int32), np.zeros(cap)
    mask_out = torch.zeros(max(n, 1), dtype=torch.uint8, device=p1.device)
    labels = torch.full((max(n, 1),), -1, dtype=torch.int32, device=p1.device)
    sm = torch.cuda.current_stream(p1.device).cuda_stream if stream is None else stream
    check(ctx.lib.mlpl_pose_homographies_dev(ctx.handle, p1.data_ptr(), p2.data_ptr(), n, None if mask is None else mask.data_ptr(), float(th),
                                             1 if check_plane_strength else 0, 1 if var_th else 0, st.ctypes.data, C.addressof(result), R.ctypes.data,
                                             t.ctypes.data, E.ctypes.data, C.addressof(ninl), mask_out.data_ptr(), cap, C.addressof(npl), H.ctypes.data,
                                             num.ctypes.data, strength.ctypes.data, labels.data_ptr(), info.ctypes.data, sm), "mlpl_pose_homographies_dev")
    out = _pose_hom_result(result, R, t, E, ninl, npl, H, num, strength, info)
    out.update(mask=mask_out[:n], labels=labels[:n])
    return out


def pose_homographies_batch(d_p1, d_p2, counts, th: float, check_plane_strength: bool = False, var_th: bool = False, rng_states=None,
                            masks_out=None, labels_out=None, ctx: Optional[Context] = None) -> list:
    """A batch of estimatePoseHomographies problems in ONE library call (mlpl_pose_homographies_batch_dev), inputs as
    mult_homographies_batch.  Returns one dict per problem with the keys of pose_homographies_device (result, R, t, E, n_inliers,
    n_planes, H, num_inl, strength, info) plus rng_state; masks through masks_out (uint8 CUDA tensor [B, stride]), labels through
    labels_out (int32 CUDA tensor [B, stride])."""
    import torch

    ctx = ctx or default_context()
    B, stride, cn, st = _plane_batch_inputs(d_p1, d_p2, counts, rng_states)
    cap = POSE_HOM_MAX_PLANES
    if masks_out is None:
        masks_out = torch.zeros((B, stride), dtype=torch.uint8, device=d_p1.device)
    if labels_out is None:
        labels_out = torch.full((B, stride), -1, dtype=torch.int32, device=d_p1.device)
    assert masks_out.is_cuda and masks_out.dtype == torch.uint8 and masks_out.shape == (B, stride) and masks_out.is_contiguous()
    assert labels_out.is_cuda and labels_out.dtype == torch.int32 and labels_out.shape == (B, stride) and labels_out.is_contiguous()
    res, ninl, npl, status = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    R, t, E, info = np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros((B, 3, 3)), np.zeros((B, 24))
    H, num, strength = np.zeros((B, cap, 3, 3)), np.zeros((B, cap), np.int32), np.zeros((B, cap))
    rc = ctx.lib.mlpl_pose_homographies_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, float(th),
                                                  1 if check_plane_strength else 0, 1 if var_th else 0, st.ctypes.data, res.ctypes.data, R.ctypes.data,
                                                  t.ctypes.data, E.ctypes.data, ninl.ctypes.data, masks_out.data_ptr(), cap, npl.ctypes.data, H.ctypes.data,
                                                  num.ctypes.data, strength.ctypes.data, labels_out.data_ptr(), info.ctypes.data, status.ctypes.data,
                                                  torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_pose_homographies_batch_dev", _lib.last_error())
    out = []
    for b in range(B):
        k = max(int(npl[b]), 0)
        out.append(dict(result=int(res[b]), R=R[b].copy(), t=t[b].copy(), E=E[b].copy(), n_inliers=int(ninl[b]), n_planes=int(npl[b]), H=H[b, :k].copy(),
                        num_inl=num[b, :k].copy(), strength=strength[b, :k].copy(), info=info[b].copy(), rng_state=st[b].copy()))
    return out


def estimatePoseHomographies(p1, p2, th: float, mask=None, checkPlaneStrength: bool = False, varTh: bool = False, ctx: Optional[Context] = None):
    """The reference's signature in Python: (rc, R, t, E, inliers, mask, inlier_points, numbersHinliers, homographies, planeStrengths); the
    process-wide stream pair, as its statics.  inlier_points: per plane the pair (left, right) of its correspondences among the rows the
    input mask kept.  With rc != 0 everything but rc is None, as the reference leaves its outputs alone."""
    q1, q2 = _pts(p1), _pts(p2)
    r = pose_homographies(q1, q2, th, mask=mask, check_plane_strength=checkPlaneStrength, var_th=varTh, ctx=ctx)
    if r["result"] != 0:
        return r["result"], None, None, None, None, None, None, None, None, None
    if mask is not None:
        keep = np.asarray(mask).reshape(-1) != 0
        q1, q2 = q1[keep], q2[keep]
    pts = [(q1[r["labels"] == k].copy(), q2[r["labels"] == k].copy()) for k in range(r["n_planes"])]
    return (0, r["R"], r["t"].reshape(3, 1), r["E"], r["n_inliers"], r["mask"].reshape(1, -1), pts, [int(v) for v in r["num_inl"]],
            [h for h in r["H"]], [float(v) for v in r["strength"]])


def homography_sample_models(p1, p2, idx, ctx: Optional[Context] = None):
    """mlpl_debug_homography_models: the device's estimator on index lists idx [count, m] -> (H [count,3,3], ok [count])."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    idx = np.ascontiguousarray(np.atleast_2d(idx), np.int32)
    count, m = idx.shape
    H, ok = np.zeros((count, 3, 3)), np.zeros(count, np.int32)
    check(ctx.lib.mlpl_debug_homography_models(ctx.handle, p1.ctypes.data, p2.ctypes.data, p1.shape[0], idx.ctypes.data, m, count, H.ctypes.data,
                                               ok.ctypes.data), "mlpl_debug_homography_models")
    return H, ok


def computeHomographyArrsac(points1, points2, th: float, ctx: Optional[Context] = None):
    """The reference's signature in Python: (ok, H, mask, p_filtered1, p_filtered2); the process-wide stream pair, as its statics."""
    p1, p2 = _pts(points1), _pts(points2)
    r = homography_arrsac(p1, p2, th, ctx=ctx)
    if not r["ok"]:
        return False, None, None, None, None
    keep = r["mask"].astype(bool)
    return True, r["H"], r["mask"], p1[keep], p2[keep]


def estimateMultHomographys(p1, p2, th: float, varTh: bool = True, maxPlanes: int = 0, minPtsPerPlane: int = 4, ctx: Optional[Context] = None):
    """The reference's signature in Python: (rc, inl_mask, inl_points, Hs, num_inl, planeStrength) as lists, rc = 0 / -1."""
    p1, p2 = _pts(p1), _pts(p2)
    r = mult_homographies(p1, p2, th, var_th=varTh, max_planes=maxPlanes, min_pts_per_plane=minPtsPerPlane, ctx=ctx)
    if r["rc"]:
        return -1, [], [], [], [], []
    masks = [m for m in r["masks"]]
    pts = [(p1[m.astype(bool)], p2[m.astype(bool)]) for m in masks]
    return 0, masks, pts, [h for h in r["H"]], [int(v) for v in r["num_inl"]], [float(v) for v in r["strength"]]


def estimateEssentialMat(p1, p2, method: str = "ARRSAC", threshold: float = PIX_MIN_GOOD_TH, refine: bool = True,
                         seed: Optional[int] = None, ctx: Optional[Context] = None):
    """poselib::estimateEssentialMat (pose_estim.h:204-210, pose_estim.cpp:857-890) -> (ok, E, mask).

    "RANSAC" (the hot path), "LMEDS" and "ARRSAC" (the reference's default) are built in this library.  Like the reference, "USAC"
    and unknown method names are fatal (the reference prints and calls exit(1), pose_estim.cpp:878-887): SystemExit(1) is raised.
    `seed` = None mirrors the reference's std::srand(std::time(nullptr)) (modelest.cpp:58); ARRSAC takes no seed (its cv::RNG
    streams are process-wide, see arrsac_essential)."""
    if method in ("RANSAC", "LMEDS", "ARRSAC"):
        import time

        a, b = _pts(p1), _pts(p2)
        if a.shape[0] == 5:
            # findEssentialMat's minimal case (five-point.cpp:108-114): one solver call, up to 10 stacked 3x3 matrices,
            # mask all true
            Es, nm = solve_5pt(a, b, np.arange(5, dtype=np.int32)[None, :], ctx=ctx)
            return True, Es[0, : nm[0]].reshape(-1, 3).copy(), np.ones(5, np.uint8)
        if method == "ARRSAC":
            r = arrsac_essential(p1, p2, threshold, refine=refine, ctx=ctx)
            return r["ok"], r["E"], r["mask"]
        s = int(time.time()) if seed is None else seed
        if method == "LMEDS":  # no least-squares refit on this branch (pose_estim.cpp:874-877)
            r = lmeds_essential(p1, p2, confidence=0.999, max_iters=2000, seed=s, ctx=ctx)
        else:
            r = ransac_essential(p1, p2, threshold, confidence=0.999, max_iters=1000, refit=refine, seed=s, ctx=ctx)
        return r["ok"], r["E"], r["mask"]
    if method == "USAC":
        print("USAC must be executed by function estimateEssentialOrPoseUSAC as it needs additional paramters! Exiting.")
    else:
        print("Either there is a typo in the specified robust estimation method or the method is not supported. Exiting.")
    raise SystemExit(1)


def getPoseTriangPts(E, p1, p2, mask=None, dist: float = 50.0, translatE: bool = False,
                     ctx: Optional[Context] = None):
    """poselib::getPoseTriangPts (pose_estim.h:192-200, pose_estim.cpp:913-946) -> (n_good, R, t, Q, mask)."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    E = np.ascontiguousarray(E, np.float64).reshape(3, 3)
    n = p1.shape[0]
    R, t, Q = np.zeros((3, 3)), np.zeros((3, 1)), np.zeros((n, 3))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1).copy()
    if translatE:
        # getTfromTransEssential (pose_helper.cpp:422-433): t = (E12, E20, E01), normalised unless already unit
        tv = np.array([E[1, 2], E[2, 0], E[0, 1]])
        nrm = float(np.sqrt(tv[0] * tv[0] + tv[1] * tv[1] + tv[2] * tv[2]))
        if abs(nrm - 1.0) > 1e-3:
            tv = tv / nrm
        tv = np.ascontiguousarray(tv)
        rc = ctx.lib.mlpl_recover_pose_translation(ctx.handle, tv.ctypes.data, p1.ctypes.data, p2.ctypes.data, n, float(dist),
                                                   R.ctypes.data, t.ctypes.data, Q.ctypes.data,
                                                   None if m is None else m.ctypes.data)
    else:
        rc = ctx.lib.mlpl_recover_pose(ctx.handle, E.ctypes.data, p1.ctypes.data, p2.ctypes.data, n, float(dist),
                                       R.ctypes.data, t.ctypes.data, Q.ctypes.data, None if m is None else m.ctypes.data)
    if rc < 0:
        raise MlplError(rc, "mlpl_recover_pose", _lib.last_error())
    return rc, R, t, Q, m


def getPoseTriangPts_device(E, p1, p2, mask=None, dist: float = 50.0, Q_out=None, ctx: Optional[Context] = None,
                            stream: Optional[int] = None):
    """getPoseTriangPts on device-resident torch tensors (float64 [n,2]; mask uint8 [n], rewritten in place; Q_out float64 [n,3]
    or None) -> (n_good, R, t).  One host hop."""
    import torch

    assert p1.is_cuda and p2.is_cuda and p1.dtype == torch.float64 and p1.is_contiguous() and p2.is_contiguous()
    ctx = ctx or default_context(p1.device.index or 0)
    E = np.ascontiguousarray(E, np.float64).reshape(3, 3)
    R, t = np.zeros((3, 3)), np.zeros((3, 1))
    st = torch.cuda.current_stream(p1.device).cuda_stream if stream is None else stream
    rc = ctx.lib.mlpl_recover_pose_dev(ctx.handle, E.ctypes.data, p1.data_ptr(), p2.data_ptr(), p1.shape[0], float(dist),
                                       R.ctypes.data, t.ctypes.data, None if Q_out is None else Q_out.data_ptr(),
                                       None if mask is None else mask.data_ptr(), st)
    if rc < 0:
        raise MlplError(rc, "mlpl_recover_pose_dev", _lib.last_error())
    return rc, R, t


def triangPts3D(R, t, p1, p2, mask=None, dist: float = 50.0, ctx: Optional[Context] = None):
    """poselib::triangPts3D (pose_estim.h:202, pose_estim.cpp:964-1044): triangulation with the given pose -> (n_good, Q, mask).  Q holds
    every point (inf / NaN where the homogeneous w is zero); mask is None when none was passed."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    if p2.shape[0] != n:
        raise ValueError("p1 and p2 differ in length")
    Rh = np.ascontiguousarray(R, np.float64).reshape(3, 3)
    th = np.ascontiguousarray(t, np.float64).reshape(3)
    Q = np.zeros((n, 3))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1).copy()
    if m is not None and m.shape[0] != n:
        raise ValueError("the mask must hold one byte per correspondence")
    rc = ctx.lib.mlpl_triang_pts3d(ctx.handle, Rh.ctypes.data, th.ctypes.data, p1.ctypes.data, p2.ctypes.data, n, float(dist), Q.ctypes.data,
                                   None if m is None else m.ctypes.data)
    if rc < 0:
        raise MlplError(rc, "mlpl_triang_pts3d", _lib.last_error())
    return rc, Q, m


def triangPts3D_device(R, t, p1, p2, mask=None, dist: float = 50.0, Q_out=None, ctx: Optional[Context] = None, stream: Optional[int] = None):
    """triangPts3D on device-resident torch tensors (float64 [n,2]; mask uint8 [n] or None, rewritten in place; Q_out float64 [n,3] or
    None) -> n_good.  Only the count is read back."""
    import torch

    assert p1.is_cuda and p2.is_cuda and p1.dtype == torch.float64 and p1.shape == p2.shape and p1.is_contiguous() and p2.is_contiguous()
    n = p1.shape[0]
    if mask is not None:
        assert mask.is_cuda and mask.dtype == torch.uint8 and mask.shape == (n,) and mask.is_contiguous()
    if Q_out is not None:
        assert Q_out.is_cuda and Q_out.dtype == torch.float64 and Q_out.shape == (n, 3) and Q_out.is_contiguous()
    ctx = ctx or default_context(p1.device.index or 0)
    Rh = np.ascontiguousarray(R, np.float64).reshape(3, 3)
    th = np.ascontiguousarray(t, np.float64).reshape(3)
    st = torch.cuda.current_stream(p1.device).cuda_stream if stream is None else stream
    rc = ctx.lib.mlpl_triang_pts3d_dev(ctx.handle, Rh.ctypes.data, th.ctypes.data, p1.data_ptr(), p2.data_ptr(), n, float(dist),
                                       None if Q_out is None else Q_out.data_ptr(), None if mask is None else mask.data_ptr(), st)
    if rc < 0:
        raise MlplError(rc, "mlpl_triang_pts3d_dev", _lib.last_error())
    return rc


def triang_pts3d_batch(d_p1, d_p2, counts, R, t, d_masks=None, d_Q=None, dist: float = 50.0, ctx: Optional[Context] = None) -> np.ndarray:
    """mlpl_triang_pts3d_batch_dev in the layout of recover_pose_batch: R [B, 3, 3], t [B, 3] (host); d_masks (uint8 CUDA tensor [B, stride]
    or None = all points) is rewritten in place up to counts[b]; d_Q (float64 CUDA tensor [B, stride, 3] or None) receives every point.
    Returns n_good [B]."""
    import torch

    B, stride = d_p1.shape[0], d_p1.shape[1]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (B, stride, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    if d_masks is not None:
        assert d_masks.is_cuda and d_masks.dtype == torch.uint8 and d_masks.shape == (B, stride) and d_masks.is_contiguous()
    if d_Q is not None:
        assert d_Q.is_cuda and d_Q.dtype == torch.float64 and d_Q.shape == (B, stride, 3) and d_Q.is_contiguous()
    ctx = ctx or default_context(d_p1.device.index or 0)
    cn = np.ascontiguousarray(counts, np.int32).reshape(B)
    Rh = np.ascontiguousarray(np.asarray(R, np.float64).reshape(B, 9))
    th = np.ascontiguousarray(np.asarray(t, np.float64).reshape(B, 3))
    n_good = np.zeros(B, np.int32)
    rc = ctx.lib.mlpl_triang_pts3d_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data, Rh.ctypes.data, th.ctypes.data,
                                             float(dist), None if d_masks is None else d_masks.data_ptr(), None if d_Q is None else d_Q.data_ptr(),
                                             n_good.ctypes.data, torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_triang_pts3d_batch_dev", _lib.last_error())
    return n_good


ROBUST_THRESH = 0.005  # BA_driver.h: the pseudo-Huber threshold in pixels that a negative huber_thresh selects


def ba_threshold(K1, K2, huber_thresh: float = -1.0) -> float:
    """The Huber threshold in camera units as poselib::refineStereoBA converts it (pose_estim.cpp:1132-1136, :1195): the sum reads
    K(1,1) and K(2,2) -- fy and the 1.0 --, as the reference indexes."""
    th = huber_thresh if huber_thresh >= 0 else ROBUST_THRESH
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    return float(4.0 * th / (np.sqrt(2.0) * (K1[1, 1] + K1[2, 2] + K2[1, 1] + K2[2, 2])))


def _ba_last_mu(ctx, n):
    mu = np.zeros(n)
    got = ctx.lib.mlpl_debug_ba_last_mu(mu.ctypes.data, n)
    return mu if got == n else None


def refine_stereo_ba(p1, p2, R, t, Q, th: float, mask=None, angle_thresh: float = 1.25, t_norm_thresh: float = 0.05,
                     ctx: Optional[Context] = None) -> dict:
    """mlpl_refine_stereo_ba: bundle adjustment of one stereo pair (motion and structure, first camera fixed, pseudo-Huber cost) on
    camera-coordinate correspondences; th in CAMERA units (ba_threshold).  -> dict(accepted, R [3, 3], t [3], Q [n, 3], info [10], mu);
    a rejected or failed run returns R, t and Q as they came."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    n = p1.shape[0]
    Rh = np.array(R, np.float64).reshape(3, 3).copy()
    tv = np.array(t, np.float64).reshape(3).copy()
    Qh = np.ascontiguousarray(np.array(Q, np.float64).reshape(-1, 3)).copy()
    if p2.shape[0] != n or Qh.shape[0] != n:
        raise ValueError("p1, p2 and Q differ in length")
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    if m is not None and m.shape[0] != n:
        raise ValueError("the mask must hold one byte per correspondence")
    info = np.zeros(10)
    rc = ctx.lib.mlpl_refine_stereo_ba(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, None if m is None else m.ctypes.data, Rh.ctypes.data,
                                       tv.ctypes.data, Qh.ctypes.data, float(th), float(angle_thresh), float(t_norm_thresh), info.ctypes.data)
    if rc < 0:
        raise MlplError(rc, "mlpl_refine_stereo_ba", _lib.last_error())
    mu = _ba_last_mu(ctx, 1) if n > 0 else None
    return dict(accepted=bool(rc), R=Rh, t=tv, Q=Qh, info=info, mu=0.0 if mu is None else float(mu[0]))


def refine_stereo_ba_device(d_p1, d_p2, R, t, d_Q, th: float, d_mask=None, angle_thresh: float = 1.25, t_norm_thresh: float = 0.05,
                            ctx: Optional[Context] = None, stream: Optional[int] = None) -> dict:
    """mlpl_refine_stereo_ba_dev on device-resident torch tensors (float64 [n, 2], d_Q float64 [n, 3] refined in place when accepted, d_mask
    uint8 [n] or None) -> dict(accepted, R, t, info, mu).  Only the pose and info are read back."""
    import torch

    n = d_p1.shape[0]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (n, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    assert d_Q.is_cuda and d_Q.dtype == torch.float64 and d_Q.shape == (n, 3) and d_Q.is_contiguous()
    if d_mask is not None:
        assert d_mask.is_cuda and d_mask.dtype == torch.uint8 and d_mask.shape == (n,) and d_mask.is_contiguous()
    ctx = ctx or default_context(d_p1.device.index or 0)
    Rh = np.array(R, np.float64).reshape(3, 3).copy()
    tv = np.array(t, np.float64).reshape(3).copy()
    info = np.zeros(10)
    st = torch.cuda.current_stream(d_p1.device).cuda_stream if stream is None else stream
    rc = ctx.lib.mlpl_refine_stereo_ba_dev(ctx.handle, d_p1.data_ptr(), d_p2.data_ptr(), n, None if d_mask is None else d_mask.data_ptr(),
                                           Rh.ctypes.data, tv.ctypes.data, d_Q.data_ptr(), float(th), float(angle_thresh), float(t_norm_thresh),
                                           info.ctypes.data, st)
    if rc < 0:
        raise MlplError(rc, "mlpl_refine_stereo_ba_dev", _lib.last_error())
    mu = _ba_last_mu(ctx, 1) if n > 0 else None
    return dict(accepted=bool(rc), R=Rh, t=tv, info=info, mu=0.0 if mu is None else float(mu[0]))


def refine_stereo_ba_batch(d_p1, d_p2, counts, R, t, d_Q, th, d_masks=None, angle_thresh: float = 1.25, t_norm_thresh: float = 0.05,
                           ctx: Optional[Context] = None) -> dict:
    """mlpl_refine_stereo_ba_batch_dev in the layout of triang_pts3d_batch, behind which it chains: R [B, 3, 3], t [B, 3] (host), th a scalar
    or [B]; d_Q (float64 CUDA tensor [B, stride, 3]) is refined in place for the accepted problems, rows outside the mask and beyond
    counts[b] untouched.  One launch.  -> dict(accepted [B], R [B, 3, 3], t [B, 3], info [B, 10], mu [B])."""
    import torch

    B, stride = d_p1.shape[0], d_p1.shape[1]
    assert d_p1.is_cuda and d_p1.dtype == torch.float64 and d_p1.shape == d_p2.shape == (B, stride, 2) and d_p1.is_contiguous() and d_p2.is_contiguous()
    assert d_Q.is_cuda and d_Q.dtype == torch.float64 and d_Q.shape == (B, stride, 3) and d_Q.is_contiguous()
    if d_masks is not None:
        assert d_masks.is_cuda and d_masks.dtype == torch.uint8 and d_masks.shape == (B, stride) and d_masks.is_contiguous()
    ctx = ctx or default_context(d_p1.device.index or 0)
    cn = np.ascontiguousarray(counts, np.int32).reshape(B)
    Rh = np.ascontiguousarray(np.array(R, np.float64).reshape(B, 9)).copy()
    tv = np.ascontiguousarray(np.array(t, np.float64).reshape(B, 3)).copy()
    thv = np.ascontiguousarray(np.broadcast_to(np.asarray(th, np.float64), (B,))).copy()
    acc, info = np.zeros(B, np.int32), np.zeros((B, 10))
    rc = ctx.lib.mlpl_refine_stereo_ba_batch_dev(ctx.handle, B, d_p1.data_ptr(), d_p2.data_ptr(), stride, cn.ctypes.data,
                                                 None if d_masks is None else d_masks.data_ptr(), d_Q.data_ptr(), Rh.ctypes.data, tv.ctypes.data,
                                                 thv.ctypes.data, float(angle_thresh), float(t_norm_thresh), acc.ctypes.data, info.ctypes.data,
                                                 torch.cuda.current_stream(d_p1.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_refine_stereo_ba_batch_dev", _lib.last_error())
    return dict(accepted=acc.astype(bool), R=Rh.reshape(B, 3, 3), t=tv, info=info, mu=_ba_last_mu(ctx, B))


def ba_threshold_multicam(Ks, huber_thresh: float = -1.0) -> float:
    """The Huber threshold in camera units as poselib::refineMultCamBA converts it (pose_estim.cpp:1510-1514, :1566-1571): the threshold in
    pixels over the mean of (K(1,1) + K(2,2)) / 2 -- fy and the 1.0 --, as the reference indexes."""
    th = huber_thresh if huber_thresh >= 0 else ROBUST_THRESH
    f_mean = 0.0
    for K in Ks:
        K = np.asarray(K, np.float64)
        f_mean += (K[1, 1] + K[2, 2]) / 2.0
    f_mean /= float(len(Ks))
    return float(th / f_mean)


def _ba_multicam_last_mu(ctx, n):
    mu = np.zeros(n)
    got = ctx.lib.mlpl_debug_ba_multicam_last_mu(mu.ctypes.data, n)
    return mu if got == n else None


def refine_multicam_ba(p, vis, R, t, Q, th: float, angle_thresh: float = 1.25, t_norm_thresh: float = 0.05,
                       ctx: Optional[Context] = None) -> dict:
    """mlpl_refine_multicam_ba: bundle adjustment of m cameras over one shared structure (motion and structure, the first camera fixed at the
    pose given, pseudo-Huber cost).  p [m, n, 2] in camera coordinates (read where vis is nonzero), vis [m, n], R [m, 3, 3], t [m, 3],
    Q [n, 3]; th in CAMERA units (ba_threshold_multicam).  -> dict(accepted, R [m, 3, 3], t [m, 3], Q [n, 3], info [10], mu); a rejected or
    failed run returns R, t and Q as they came; an accepted one returns every t as the optimiser left it (not normalised)."""
    ctx = ctx or default_context()
    vh = np.ascontiguousarray(vis, np.uint8)
    if vh.ndim != 2:
        raise ValueError("vis must be [m, n]")
    m, n = vh.shape
    ph = np.ascontiguousarray(np.asarray(p, np.float64).reshape(m, n, 2))
    Rh = np.ascontiguousarray(np.array(R, np.float64).reshape(m, 9)).copy()
    tv = np.ascontiguousarray(np.array(t, np.float64).reshape(m, 3)).copy()
    Qh = np.ascontiguousarray(np.array(Q, np.float64).reshape(-1, 3)).copy()
    if Qh.shape[0] != n:
        raise ValueError("vis and Q differ in the number of points")
    info = np.zeros(10)
    rc = ctx.lib.mlpl_refine_multicam_ba(ctx.handle, ph.ctypes.data, vh.ctypes.data, m, n, Rh.ctypes.data, tv.ctypes.data, Qh.ctypes.data,
                                         float(th), float(angle_thresh), float(t_norm_thresh), info.ctypes.data)
    if rc < 0:
        raise MlplError(rc, "mlpl_refine_multicam_ba", _lib.last_error())
    mu = _ba_multicam_last_mu(ctx, 1) if n > 0 else None
    return dict(accepted=bool(rc), R=Rh.reshape(m, 3, 3), t=tv, Q=Qh, info=info, mu=0.0 if mu is None else float(mu[0]))


def refine_multicam_ba_device(d_p, d_vis, R, t, d_Q, th: float, angle_thresh: float = 1.25, t_norm_thresh: float = 0.05,
                              ctx: Optional[Context] = None, stream: Optional[int] = None) -> dict:
    """mlpl_refine_multicam_ba_dev on device-resident torch tensors (d_p float64 [m, n, 2], d_vis uint8 [m, n], d_Q float64 [n, 3] refined in
    place when accepted) -> dict(accepted, R, t, info, mu).  Only the poses and info are read back."""
    import torch

    m, n = d_vis.shape
    assert d_p.is_cuda and d_p.dtype == torch.float64 and d_p.shape == (m, n, 2) and d_p.is_contiguous()
    assert d_vis.is_cuda and d_vis.dtype == torch.uint8 and d_vis.is_contiguous()
    assert d_Q.is_cuda and d_Q.dtype == torch.float64 and d_Q.shape == (n, 3) and d_Q.is_contiguous()
    ctx = ctx or default_context(d_p.device.index or 0)
    Rh = np.ascontiguousarray(np.array(R, np.float64).reshape(m, 9)).copy()
    tv = np.ascontiguousarray(np.array(t, np.float64).reshape(m, 3)).copy()
    info = np.zeros(10)
    st = torch.cuda.current_stream(d_p.device).cuda_stream if stream is None else stream
    rc = ctx.lib.mlpl_refine_multicam_ba_dev(ctx.handle, d_p.data_ptr(), d_vis.data_ptr(), m, n, Rh.ctypes.data, tv.ctypes.data, d_Q.data_ptr(),
                                             float(th), float(angle_thresh), float(t_norm_thresh), info.ctypes.data, st)
    if rc < 0:
        raise MlplError(rc, "mlpl_refine_multicam_ba_dev", _lib.last_error())
    mu = _ba_multicam_last_mu(ctx, 1) if n > 0 else None
    return dict(accepted=bool(rc), R=Rh.reshape(m, 3, 3), t=tv, info=info, mu=0.0 if mu is None else float(mu[0]))


def refine_multicam_ba_batch(d_p, d_vis, n_cams, counts, R, t, d_Q, th, angle_thresh: float = 1.25, t_norm_thresh: float = 0.05,
                             ctx: Optional[Context] = None) -> dict:
    """mlpl_refine_multicam_ba_batch_dev: d_p float64 [B, cams_stride, stride, 2], d_vis uint8 [B, cams_stride, stride], d_Q float64
    [B, stride, 3] (refined in place for the accepted problems; rows beyond counts[b] untouched), n_cams [B], counts [B], R
    [B, cams_stride, 3, 3], t [B, cams_stride, 3] (host), th a scalar or [B].  One launch.
    -> dict(accepted [B], R [B, cams_stride, 3, 3], t [B, cams_stride, 3], info [B, 10], mu [B])."""
    import torch

    B, cams_stride, stride = d_vis.shape
    assert d_p.is_cuda and d_p.dtype == torch.float64 and d_p.shape == (B, cams_stride, stride, 2) and d_p.is_contiguous()
    assert d_vis.is_cuda and d_vis.dtype == torch.uint8 and d_vis.is_contiguous()
    assert d_Q.is_cuda and d_Q.dtype == torch.float64 and d_Q.shape == (B, stride, 3) and d_Q.is_contiguous()
    ctx = ctx or default_context(d_p.device.index or 0)
    nc = np.ascontiguousarray(n_cams, np.int32).reshape(B)
    cn = np.ascontiguousarray(counts, np.int32).reshape(B)
    Rh = np.ascontiguousarray(np.array(R, np.float64).reshape(B, cams_stride, 9)).copy()
    tv = np.ascontiguousarray(np.array(t, np.float64).reshape(B, cams_stride, 3)).copy()
    thv = np.ascontiguousarray(np.broadcast_to(np.asarray(th, np.float64), (B,))).copy()
    acc, info = np.zeros(B, np.int32), np.zeros((B, 10))
    rc = ctx.lib.mlpl_refine_multicam_ba_batch_dev(ctx.handle, B, d_p.data_ptr(), d_vis.data_ptr(), cams_stride, stride, nc.ctypes.data,
                                                   cn.ctypes.data, d_Q.data_ptr(), Rh.ctypes.data, tv.ctypes.data, thv.ctypes.data,
                                                   float(angle_thresh), float(t_norm_thresh), acc.ctypes.data, info.ctypes.data,
                                                   torch.cuda.current_stream(d_p.device).cuda_stream)
    if rc != 0:
        raise MlplError(rc, "mlpl_refine_multicam_ba_batch_dev", _lib.last_error())
    return dict(accepted=acc.astype(bool), R=Rh.reshape(B, cams_stride, 3, 3), t=tv, info=info, mu=_ba_multicam_last_mu(ctx, B))


def ImgToCamCoordTrans(points, K, ctx: Optional[Context] = None) -> np.ndarray:
    """poselib::ImgToCamCoordTrans (pose_helper.cpp:1100-1109): float32 n x 2 pixel points -> camera coordinates."""
    ctx = ctx or default_context()
    pts = np.ascontiguousarray(points, np.float32).copy()
    K = np.asarray(K, np.float64)
    k4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) if K.shape == (3, 3) else K.astype(np.float64)
    check(ctx.lib.mlpl_img_to_cam(ctx.handle, pts.ctypes.data, pts.shape[0], k4.ctypes.data), "mlpl_img_to_cam")
    return pts


def Remove_LensDist(points1, points2, dist1, dist2, ctx: Optional[Context] = None):
    """poselib::Remove_LensDist (pose_helper.cpp:1169-1223) -> (ok, points1, points2) with failing pairs dropped."""
    ctx = ctx or default_context()
    a = np.ascontiguousarray(points1, np.float32).copy()
    b = np.ascontiguousarray(points2, np.float32).copy()
    d1 = np.ascontiguousarray(np.asarray(dist1, np.float64).reshape(-1))
    d2 = np.ascontiguousarray(np.asarray(dist2, np.float64).reshape(-1))
    assert d1.size == 8 and d2.size == 8 and a.shape == b.shape
    n_out = C.c_int(0)
    rc = ctx.lib.mlpl_remove_lens_dist(ctx.handle, a.ctypes.data, b.ctypes.data, a.shape[0], d1.ctypes.data, d2.ctypes.data,
                                       C.byref(n_out))
    if rc not in (0, _lib.MLPL_E_FAILED):
        raise MlplError(rc, "mlpl_remove_lens_dist", _lib.last_error())
    return rc == 0, a[: n_out.value], b[: n_out.value]


def getInliers(E, p1, p2, th2: float, ctx: Optional[Context] = None):
    """StereoRefine::getInliers (stereo_pose_refinement.cpp:2085-2090) -> (n_inliers, mask, error); strict `<`."""
    ctx = ctx or default_context()
    p1, p2 = _pts(p1), _pts(p2)
    E = np.ascontiguousarray(E, np.float64).reshape(3, 3)
    n = p1.shape[0]
    err = np.zeros(n)
    mask = np.zeros(n, np.uint8)
    rc = ctx.lib.mlpl_get_inliers_strict(ctx.handle, p1.ctypes.data, p2.ctypes.data, n, E.ctypes.data, float(th2),
                                         err.ctypes.data, mask.ctypes.data)
    if rc < 0:
        raise MlplError(rc, "mlpl_get_inliers_strict", _lib.last_error())
    return rc, mask, err


def estimateRelativePose(p1, p2, threshold: float = PIX_MIN_GOOD_TH, refine: bool = True, dist: float = 50.0,
                         seed: Optional[int] = None, ctx: Optional[Context] = None):
    """Convenience named in BASELINE.json: estimateEssentialMat("RANSAC") followed by getPoseTriangPts, as the
    reference's README and harness do (README.md:497-521, tests/poselib-test/main.cpp:1717,1827)."""
    ok, E, mask = estimateEssentialMat(p1, p2, "RANSAC", threshold, refine, seed=seed, ctx=ctx)
    if not ok:
        return False, E, None, None, None, mask
    n_good, R, t, Q, mask2 = getPoseTriangPts(E, p1, p2, mask, dist, ctx=ctx)
    return True, E, R, t, Q, mask2


# ---- stereo rectification (include/mlpl_c.h, "stereo rectification") --------------------------------------------------------------------------
def _dist(d):
    d = np.zeros(0) if d is None else np.ascontiguousarray(np.asarray(d, np.float64).reshape(-1))
    if d.size not in (0, 4, 5, 8):
        raise MlplError(_lib.MLPL_E_BAD_INPUT, "rectification", "0, 4, 5 or 8 distortion coefficients")
    return d


def _m33(m):
    return np.ascontiguousarray(np.asarray(m, np.float64).reshape(9))


def _u8_image(img, what):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2 or a.size == 0:
        raise MlplError(_lib.MLPL_E_BAD_INPUT, what, "images are 8-bit, single channel and not empty")
    return a if a.strides[1] == 1 and a.strides[0] >= a.shape[1] else np.ascontiguousarray(a)


def rectification_parameters(R, t, K1, K2, dist1, dist2, image_size, alpha: float = -1.0, new_image_size=(0, 0)) -> dict:
    """mlpl_rectify_parameters: poselib::getRectificationParameters with globRectFunct = true (Fusiello) -> dict(Rect1, Rect2, Knew [3, 3],
    roi [x, y, width, height], P1, P2 [3, 4], info [8] = {fc_new before scaling, s0, s1, s, reduction steps of the four undistortion loops}).
    image_size / new_image_size = (width, height); a new size with a zero side means the image size.  Host arithmetic: no device needed."""
    lib = _lib.load_library()
    Rm, tv, k1, k2, d1, d2 = _m33(R), np.ascontiguousarray(np.asarray(t, np.float64).reshape(3)), _m33(K1), _m33(K2), _dist(dist1), _dist(dist2)
    r1, r2, kn, roi, p1, p2, info = np.zeros(9), np.zeros(9), np.zeros(9), np.zeros(4, np.int32), np.zeros(12), np.zeros(12), np.zeros(8)
    rc = lib.mlpl_rectify_parameters(Rm.ctypes.data, tv.ctypes.data, k1.ctypes.data, k2.ctypes.data, d1.ctypes.data if d1.size else None, d1.size,
                                     d2.ctypes.data if d2.size else None, d2.size, int(image_size[0]), int(image_size[1]), float(alpha),
                                     int(new_image_size[0]), int(new_image_size[1]), r1.ctypes.data, r2.ctypes.data, kn.ctypes.data,
                                     roi.ctypes.data, p1.ctypes.data, p2.ctypes.data, info.ctypes.data)
    check(rc, "mlpl_rectify_parameters")
    return dict(Rect1=r1.reshape(3, 3), Rect2=r2.reshape(3, 3), Knew=kn.reshape(3, 3), roi=[int(v) for v in roi], P1=p1.reshape(3, 4),
                P2=p2.reshape(3, 4), info=info)


def rectify_maps(K, dist, Rect, Knew, size, ctx: Optional[Context] = None, device_out=None, stream: Optional[int] = None):
    """cv::initUndistortRectifyMap(K, dist, Rect, Knew, size, CV_32FC1) -> (mapx, mapy) float32 [height, width]; size = (width, height).
    device_out = (mapx, mapy) float32 CUDA tensors [height, >= width] with unit column stride: mlpl_rectify_maps_dev fills and returns them
    (enqueued on `stream`, None = torch's current stream, no synchronisation); otherwise numpy arrays through mlpl_rectify_maps."""
    ctx = ctx or default_context()
    k, d, r, kn = _m33(K), _dist(dist), _m33(Rect), _m33(Knew)
    w, h = int(size[0]), int(size[1])
    dp = d.ctypes.data if d.size else None
    if device_out is not None:
        import torch

        mx, my = device_out
        for m in (mx, my):
            assert m.is_cuda and m.dtype == torch.float32 and m.dim() == 2 and m.shape == (h, w) and m.stride(1) == 1 and m.stride(0) == mx.stride(0)
        st = torch.cuda.current_stream(mx.device).cuda_stream if stream is None else stream
        check(ctx.lib.mlpl_rectify_maps_dev(ctx.handle, k.ctypes.data, dp, d.size, r.ctypes.data, kn.ctypes.data, w, h, mx.data_ptr(), my.data_ptr(),
                                            mx.stride(0), st), "mlpl_rectify_maps_dev")
        return mx, my
    mx, my = np.zeros((max(h, 1), max(w, 1)), np.float32), np.zeros((max(h, 1), max(w, 1)), np.float32)
    check(ctx.lib.mlpl_rectify_maps(ctx.handle, k.ctypes.data, dp, d.size, r.ctypes.data, kn.ctypes.data, w, h, mx.ctypes.data, my.ctypes.data),
          "mlpl_rectify_maps")
    return mx, my


def remap_bilinear(img, mapx, mapy, ctx: Optional[Context] = None, device_out=None, stream: Optional[int] = None):
    """cv::remap(img, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT) on an 8-bit single-channel image, OpenCV's fixed-point arithmetic -> uint8
    [map height, map width].  numpy arguments: mlpl_remap_bilinear.  CUDA tensors (img uint8 [h, >= w], maps float32 of one row stride, all
    with unit column stride): mlpl_remap_bilinear_dev into device_out (uint8, allocated when None), enqueued without synchronising."""
    ctx = ctx or default_context()
    if hasattr(img, "is_cuda"):
        import torch

        assert img.is_cuda and img.dtype == torch.uint8 and img.dim() == 2 and img.stride(1) == 1
        for m in (mapx, mapy):
            assert m.is_cuda and m.dtype == torch.float32 and m.dim() == 2 and m.shape == mapx.shape and m.stride(1) == 1 and m.stride(0) == mapx.stride(0)
        oh, ow = mapx.shape
        out = torch.empty((oh, ow), dtype=torch.uint8, device=img.device) if device_out is None else device_out
        assert out.is_cuda and out.dtype == torch.uint8 and out.shape == (oh, ow) and out.stride(1) == 1
        st = torch.cuda.current_stream(img.device).cuda_stream if stream is None else stream
        check(ctx.lib.mlpl_remap_bilinear_dev(ctx.handle, img.data_ptr(), img.shape[1], img.shape[0], img.stride(0), mapx.data_ptr(), mapy.data_ptr(),
                                              mapx.stride(0), ow, oh, out.data_ptr(), out.stride(0), st), "mlpl_remap_bilinear_dev")
        return out
    im = _u8_image(img, "remap_bilinear")
    mx, my = np.ascontiguousarray(mapx, np.float32), np.ascontiguousarray(mapy, np.float32)
    if mx.ndim != 2 or mx.shape != my.shape:
        raise MlplError(_lib.MLPL_E_BAD_INPUT, "remap_bilinear", "two maps of one shape")
    out = np.zeros(mx.shape, np.uint8)
    check(ctx.lib.mlpl_remap_bilinear(ctx.handle, im.ctypes.data, im.shape[1], im.shape[0], im.strides[0], mx.ctypes.data, my.ctypes.data,
                                      mx.shape[1], mx.shape[0], out.ctypes.data, out.strides[0] if out.size else 0), "mlpl_remap_bilinear")
    return out


def rectify_param_block(K, dist, Rect, Knew) -> np.ndarray:
    """{K[9], dist[8], Rect[9], Knew[9]}: the per-image parameter block of rectify_images / rectify_images_batch (35 doubles)"""
    d = _dist(dist)
    return np.concatenate([_m33(K), d, np.zeros(8 - d.size), _m33(Rect), _m33(Knew)])


def rectify_images(img1, img2, params, new_size=None, ctx: Optional[Context] = None):
    """mlpl_rectify_images: the fused map + remap on one pair of 8-bit numpy images of one size -> (out1, out2) uint8 [new height, new
    width].  params: [2, 35], one rectify_param_block per image; new_size = (width, height), None = the image size."""
    ctx = ctx or default_context()
    a, b = _u8_image(img1, "rectify_images"), _u8_image(img2, "rectify_images")
    if a.shape != b.shape:
        raise MlplError(_lib.MLPL_E_BAD_INPUT, "rectify_images", "the two images must have one size")
    if a.strides[0] != b.strides[0]:
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    p = np.ascontiguousarray(np.asarray(params, np.float64).reshape(2, 35))
    ow, oh = (a.shape[1], a.shape[0]) if new_size is None else (int(new_size[0]), int(new_size[1]))
    o1, o2 = np.zeros((max(oh, 1), max(ow, 1)), np.uint8), np.zeros((max(oh, 1), max(ow, 1)), np.uint8)
    check(ctx.lib.mlpl_rectify_images(ctx.handle, a.ctypes.data, b.ctypes.data, a.shape[1], a.shape[0], a.strides[0], p.ctypes.data, ow, oh,
                                      o1.ctypes.data, o2.ctypes.data, o1.strides[0]), "mlpl_rectify_images")
    return o1, o2


def rectify_images_batch(img1, img2, params, new_size=None, out=None, ctx: Optional[Context] = None, stream: Optional[int] = None):
    """mlpl_rectify_images_dev: `B` pairs in one launch.  img1, img2: uint8 CUDA tensors [B, height, >= width] of one shape and strides, unit
    column stride; params: host array [B, 2, 35] (rectify_param_block per image), read before the call returns; out = (out1, out2) uint8 CUDA
    tensors [B, new height, new width] of one layout (allocated when None).  Enqueues on `stream` (None = torch's current stream) without
    synchronising; returns (out1, out2)."""
    import torch

    assert img1.is_cuda and img2.is_cuda and img1.dtype == torch.uint8 and img2.dtype == torch.uint8 and img1.dim() == 3
    assert img1.shape == img2.shape and img1.stride() == img2.stride() and img1.stride(2) == 1
    B, h, w = img1.shape
    ctx = ctx or default_context(img1.device.index or 0)
    p = np.ascontiguousarray(np.asarray(params, np.float64).reshape(B, 2, 35))
    ow, oh = (w, h) if new_size is None else (int(new_size[0]), int(new_size[1]))
    if out is None:
        out = (torch.empty((B, oh, ow), dtype=torch.uint8, device=img1.device), torch.empty((B, oh, ow), dtype=torch.uint8, device=img1.device))
    o1, o2 = out
    assert o1.is_cuda and o2.is_cuda and o1.dtype == torch.uint8 and o2.dtype == torch.uint8 and o1.shape == o2.shape == (B, oh, ow)
    assert o1.stride() == o2.stride() and o1.stride(2) == 1
    st = torch.cuda.current_stream(img1.device).cuda_stream if stream is None else stream
    check(ctx.lib.mlpl_rectify_images_dev(ctx.handle, B, img1.data_ptr(), img2.data_ptr(), w, h, img1.stride(1), img1.stride(0) if B > 1 else 0,
                                          p.ctypes.data, ow, oh, o1.data_ptr(), o2.data_ptr(), o1.stride(1), o1.stride(0) if B > 1 else 0, st),
          "mlpl_rectify_images_dev")
    return o1, o2


def smoke_check(ctx, oracle) -> None:
    """Used by __graft_entry__.smoke(): one small RANSAC + pose recovery on the GPU, checked against the CPU oracle."""
    from . import synth

    p1, p2, R, t, mask, th = synth.pose_scene(600, seed=3)
    g = ransac_essential(p1, p2, th, confidence=0.999, max_iters=300, refit=False, seed=99, ctx=ctx)
    o = oracle.ransac_essential(p1, p2, th, confidence=0.999, max_iters=300, lesqu=False, seed=99)
    assert g["ok"] and g["iters"] == o["iters"] and g["n_inliers"] == o["n_inliers"], "RANSAC differs from the oracle"
    d = min(np.abs(g["E"] - o["E"]).max(), np.abs(g["E"] + o["E"]).max())
    assert d < 1e-8, f"essential matrix differs from the oracle by {d}"
    n_good, Rg, tg, Q, m = getPoseTriangPts(g["E"], p1, p2, g["mask"], 50.0, ctx=ctx)
    go, Ro, to, Qo, mo = oracle.recover_pose(o["E"], p1, p2, 50.0, o["mask"])
    assert n_good == go and np.abs(Rg - Ro).max() < 1e-6 and np.abs(tg.ravel() - to).max() < 1e-6
    print(f"smoke: RANSAC 5pt {g['iters']} iters -> {g['n_inliers']} inliers, pose within 1e-6 of the oracle")
    # the sequential estimators as a batch (launch hub: fibers, merged launches, cohorts in flight): four USAC problems in one call, each
    # against the oracle's run of it
    import torch

    seeds = [5, 6, 7, 8]
    d1 = torch.from_numpy(np.repeat(p1[None], 4, 0).copy()).cuda()
    d2 = torch.from_numpy(np.repeat(p2[None], 4, 0).copy()).cuda()
    got = usac_essential_batch(d1, d2, [len(p1)] * 4, th, seeds, ctx=ctx)
    for b, sd in enumerate(seeds):
        ou = oracle.usac_essential(p1, p2, th, sd)
        # (hypotheses, inliers, local optimisations; the model COUNT may differ by the solutions of a sample with a double root)
        assert got[b]["ok"] and np.array_equal(got[b]["final"][[0, 1, 5, 7]], ou["final"][[0, 1, 5, 7]]), "batched USAC differs from the oracle"
        du = min(np.abs(got[b]["E"] - ou["E"]).max(), np.abs(got[b]["E"] + ou["E"]).max())
        assert du < 1e-8, f"batched USAC: essential matrix differs from the oracle by {du}"
    print(f"smoke: USAC x 4 in one batched call -> {int(got[0]['final'][5])} inliers each; hypotheses, inliers, local optimisations and E equal to the oracle's")
