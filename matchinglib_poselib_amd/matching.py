"""Host-side mirror of matchinglib::getMatches for the LINEAR (brute-force) matcher.

Reference interface: matchinglib/include/matchinglib/matchinglib_matchers.h:61-64, implementation
matchinglib/source/matchers.cpp:115-736 (LINEAR branch :525-714).  Same argument meaning, same return
codes; the arithmetic runs in libmlpl_hip.so (HIP, gfx950).  Nothing here computes distances on the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import Context, MlplError, check, default_context

# cv::DMatch {int queryIdx; int trainIdx; int imgIdx; float distance;}
DMATCH_DTYPE = np.dtype(
    [("queryIdx", np.int32), ("trainIdx", np.int32), ("imgIdx", np.int32), ("distance", np.float32)], align=True
)
assert DMATCH_DTYPE.itemsize == 16

CV_8U = 0
CV_32F = 5


def _rows_2d(a: np.ndarray, dtype) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != dtype:
        raise ValueError(f"expected a 2-D {np.dtype(dtype).name} array, got {a.dtype} with shape {a.shape}")
    if a.strides[1] != a.itemsize:  # rows must be dense; row stride may be anything (cv::Mat::step)
        a = np.ascontiguousarray(a)
    return a


def knn_hamming(q: np.ndarray, t: np.ndarray, k: int = 2, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Exact k-NN (k in {1,2}) of every row of q in t under bit-Hamming distance -> (idx, dist) int32 [nq,k].

    Replaces cvflann::Index<HammingLUT>(LinearIndexParams).knnSearch (matchers.cpp:584-588)."""
    ctx = ctx or default_context()
    q = _rows_2d(q, np.uint8)
    t = _rows_2d(t, np.uint8)
    if q.shape[1] != t.shape[1]:
        raise ValueError("descriptor widths differ")
    nq, nbytes = q.shape
    idx = np.empty((nq, k), np.int32)
    dist = np.empty((nq, k), np.int32)
    rc = ctx.lib.mlpl_knn2_hamming(
        ctx.handle, q.ctypes.data, nq, q.strides[0], t.ctypes.data, t.shape[0], t.strides[0], nbytes, k,
        idx.ctypes.data, dist.ctypes.data)
    check(rc, "mlpl_knn2_hamming")
    return idx, dist


def knn_l2sq(q: np.ndarray, t: np.ndarray, k: int = 2, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Exact k-NN under SQUARED L2 on float32 descriptors -> (idx int32 [nq,k], dist float32 [nq,k]).

    Replaces cvflann::Index<L2<float>>(LinearIndexParams).knnSearch (matchers.cpp:660-664)."""
    ctx = ctx or default_context()
    q = _rows_2d(q, np.float32)
    t = _rows_2d(t, np.float32)
    if q.shape[1] != t.shape[1]:
        raise ValueError("descriptor widths differ")
    nq, dim = q.shape
    idx = np.empty((nq, k), np.int32)
    dist = np.empty((nq, k), np.float32)
    rc = ctx.lib.mlpl_knn2_l2sq_f32(
        ctx.handle, q.ctypes.data, nq, q.strides[0] // 4, t.ctypes.data, t.shape[0], t.strides[0] // 4, dim, k,
        idx.ctypes.data, dist.ctypes.data)
    check(rc, "mlpl_knn2_l2sq_f32")
    return idx, dist


def ratio_compact(idx: np.ndarray, dist: np.ndarray, ratio: float = 0.75, ctx: Optional[Context] = None) -> np.ndarray:
    """Ratio test + DMatch emission (matchers.cpp:601-625 / :677-701) -> structured array of DMATCH_DTYPE."""
    ctx = ctx or default_context()
    idx = np.ascontiguousarray(idx, np.int32)
    nq, k = idx.shape
    out = np.empty(nq, DMATCH_DTYPE)
    n = C.c_int(0)
    if dist.dtype == np.float32:
        dist = np.ascontiguousarray(dist)
        rc = ctx.lib.mlpl_ratio_compact_f32(ctx.handle, idx.ctypes.data, dist.ctypes.data, nq, k, ratio,
                                            out.ctypes.data, C.byref(n))
    else:
        dist = np.ascontiguousarray(dist, np.int32)
        rc = ctx.lib.mlpl_ratio_compact_i32(ctx.handle, idx.ctypes.data, dist.ctypes.data, nq, k, ratio,
                                            out.ctypes.data, C.byref(n))
    check(rc, "mlpl_ratio_compact")
    return out[: n.value].copy()


def getMatches(
    keypoints1: Sequence,
    keypoints2: Sequence,
    descriptors1: np.ndarray,
    descriptors2: np.ndarray,
    imgSi=None,
    matcher_name: str = "GMBSOF",
    VFCrefine: bool = False,
    ratioTest: bool = True,
    descriptor_name: str = "",
    idxPars_NMSLIB: str = "",
    queryPars_NMSLIB: str = "",
    nr_threads: int = 0,
    ctx: Optional[Context] = None,
    vfc_seed: int = 1,
) -> Tuple[int, np.ndarray]:
    """matchinglib::getMatches (matchinglib_matchers.h:61-64).  Returns (err, finalMatches).

    err: 0 ok, -1 wrong input data, -2 matcher not supported, -3 matching failed (< 2 matches),
    -4 too few keypoints (matchers.cpp:109-114).  matcher_name "LINEAR" (cvflann brute force, matchers.cpp:525-714) and
    "BRUTEFORCENMS" (NMSLIB seq_search, matchers.cpp:476-519, with its 240-bit / sqrt-L2 semantics) are built in this
    library; every other name -- including the reference's default "GMBSOF" -- yields -2.
    A dtype mismatch raises ValueError where the reference's CV_Assert throws cv::Exception (matchers.cpp:119).
    VFCrefine (matchers.cpp:722-733): the matches are filtered with filter_with_vfc(seed = vfc_seed) and the filtered list replaces them
    when the filter returned 0 and (kept > 8 or n < 24); keypoints1 / keypoints2 must then carry coordinates ((x, y) rows or .pt).
    """
    d1 = np.asarray(descriptors1)
    d2 = np.asarray(descriptors2)
    empty = np.empty(0, DMATCH_DTYPE)
    if d1.dtype != d2.dtype:
        raise ValueError("descriptors1.type() == descriptors2.type() assertion failed")  # CV_Assert, :119
    n1, n2 = len(keypoints1), len(keypoints2)
    if n1 < 15 or n2 < 15:
        return -4, empty
    if d1.ndim != 2 or d2.ndim != 2 or n1 != d1.shape[0] or n2 != d2.shape[0]:
        return -1, empty
    if matcher_name not in ("LINEAR", "BRUTEFORCENMS"):
        return -2, empty
    if d1.dtype == np.uint8:
        desc_type = CV_8U
    elif d1.dtype == np.float32:
        desc_type = CV_32F
    else:
        return -1, empty  # "Format of descriptors not supported!" (matchers.cpp:540-547)
    if d1.shape[1] != d2.shape[1]:
        return -1, empty
    ctx = ctx or default_context()
    d1 = _rows_2d(d1, d1.dtype)
    d2 = _rows_2d(d2, d2.dtype)
    out = np.empty(max(n1, 1), DMATCH_DTYPE)
    n = C.c_int(0)
    entry = ctx.lib.mlpl_get_matches_linear if matcher_name == "LINEAR" else ctx.lib.mlpl_get_matches_bruteforce_nms
    rc = entry(
        ctx.handle, n1, n2, d1.ctypes.data, d1.shape[0], d1.strides[0], d2.ctypes.data, d2.shape[0], d2.strides[0],
        d1.shape[1], desc_type, 1 if ratioTest else 0, out.ctypes.data, C.byref(n))
    if rc in (0, -3):
        matches = out[: n.value].copy()
        if rc == 0 and VFCrefine:
            vrc, filtered = filter_with_vfc(keypoints1, keypoints2, matches, seed=vfc_seed, ctx=ctx)
            if vrc == 0 and (len(filtered) > 8 or len(matches) < 24):
                matches = filtered
        return rc, matches
    if rc in (-1, -4):
        return rc, empty
    raise MlplError(rc, "mlpl_get_matches_linear", _lib.last_error())


def _keypoint_xy(kps) -> np.ndarray:
    """(x, y) float32 rows of a keypoint sequence: an [n, 2] array, (x, y) pairs, or objects with .pt (cv2.KeyPoint)."""
    if isinstance(kps, np.ndarray):
        return np.ascontiguousarray(kps, np.float32).reshape(-1, 2)
    return np.ascontiguousarray([k.pt if hasattr(k, "pt") else k for k in kps], np.float32).reshape(-1, 2)


def vfc_filter_points(x1, x2, seed: int = 1, ctx: Optional[Context] = None) -> dict:
    """mlpl_vfc_filter on matched points x1[i] -> x2[i] (float32 [n, 2]) -> dict(rc, keep bool [n], n_keep, P float64 [n], m, iterations,
    refused, singular).  rc = 0, -1 (n < 5: everything kept) or -2 (fewer than 10 % kept)."""
    ctx = ctx or default_context()
    x1 = np.ascontiguousarray(x1, np.float32).reshape(-1, 2)
    x2 = np.ascontiguousarray(x2, np.float32).reshape(-1, 2)
    n = x1.shape[0]
    if x2.shape[0] != n:
        raise ValueError("x1 and x2 differ in length")
    keep, P, info, nk = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float64), np.zeros(4, np.int32), C.c_int(0)
    rc = ctx.lib.mlpl_vfc_filter(ctx.handle, x1.ctypes.data, x2.ctypes.data, n, int(seed) & 0xFFFFFFFF, keep.ctypes.data, C.byref(nk),
                                 P.ctypes.data, info.ctypes.data)
    if rc not in (0, -1, -2):
        raise MlplError(rc, "mlpl_vfc_filter", _lib.last_error())
    return dict(rc=rc, keep=keep[:n].astype(bool), n_keep=nk.value, P=P[:n], m=int(info[0]), iterations=int(info[1]), refused=bool(info[2]),
                singular=int(info[3]))


def filter_with_vfc(kp1, kp2, matches: np.ndarray, seed: int = 1, ctx: Optional[Context] = None) -> Tuple[int, np.ndarray]:
    """matchinglib::filterWithVFC (vfcMatches.cpp:63-100) -> (rc, matches_out): 0 ok, -1 fewer than 5 matches (matches_out empty), -2
    fewer than 10 % kept.  kp1 / kp2: keypoint coordinates (see getMatches); matches: DMATCH_DTYPE rows."""
    matches = np.ascontiguousarray(matches, DMATCH_DTYPE)
    if len(matches) < 5:
        return -1, np.empty(0, DMATCH_DTYPE)
    a, b = _keypoint_xy(kp1), _keypoint_xy(kp2)
    r = vfc_filter_points(a[matches["queryIdx"]], b[matches["trainIdx"]], seed, ctx)
    return r["rc"], matches[r["keep"]].copy()


# ---- device-resident (torch) entry: nothing leaves HBM -------------------------------------------------------

def match_hamming_device(q, t, ratio_test: bool = True, ratio: float = 0.75, ctx: Optional[Context] = None, out=None,
                         stream: Optional[int] = None):
    """Batched knn(+ratio+compaction) on CUDA/HIP torch tensors.

    q: uint8 [B, nq, nbytes] (or [nq, nbytes]), t: uint8 [B, nt, nbytes]; returns dict of torch tensors
    idx [B,nq,k] int32, dist [B,nq,k] int32, matches [B,nq,4] int32 (DMatch rows, .distance bit-cast),
    count [B] int32.  Enqueues on `stream` (a hipStream_t handle; None = torch's current stream) without
    synchronising.
    """
    import torch

    if q.dim() == 2:
        q = q.unsqueeze(0)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    assert q.is_cuda and t.is_cuda and q.dtype == torch.uint8 and t.dtype == torch.uint8
    assert q.stride(2) == 1 and t.stride(2) == 1
    B, nq, nbytes = q.shape
    nt = t.shape[1]
    ctx = ctx or default_context(q.device.index or 0)
    k = 2 if ratio_test else 1
    if out is None:
        out = {
            "idx": torch.empty((B, nq, k), dtype=torch.int32, device=q.device),
            "dist": torch.empty((B, nq, k), dtype=torch.int32, device=q.device),
            "matches": torch.empty((B, nq, 4), dtype=torch.int32, device=q.device),
            "count": torch.empty((B,), dtype=torch.int32, device=q.device),
        }
    rc = ctx.lib.mlpl_match_hamming_dev(
        ctx.handle, q.data_ptr(), nq, q.stride(1), q.stride(0), t.data_ptr(), nt, t.stride(1), t.stride(0), nbytes,
        1 if ratio_test else 0, ratio, B, out["idx"].data_ptr(), out["dist"].data_ptr(), out["matches"].data_ptr(),
        out["count"].data_ptr(), torch.cuda.current_stream(q.device).cuda_stream if stream is None else stream)
    check(rc, "mlpl_match_hamming_dev")
    return out


def match_l2_device(q, t, ratio_test: bool = True, ratio: float = 0.75, ctx: Optional[Context] = None, out=None,
                    stream: Optional[int] = None):
    """match_hamming_device for float descriptors (mlpl_match_l2_dev): squared-L2 knn + ratio + compaction on CUDA/HIP torch tensors.

    q: float32 [B, nq, dim] (or [nq, dim]), t: float32 [B, nt, dim]; rows may be padded (strides are passed in elements).  Returns dict
    of torch tensors idx [B,nq,k] int32, dist [B,nq,k] float32, matches [B,nq,4] int32 (DMatch rows, .distance bit-cast), count [B]
    int32.  Enqueues on `stream` (a hipStream_t handle; None = torch's current stream) without synchronising.
    """
    import torch

    if q.dim() == 2:
        q = q.unsqueeze(0)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    assert q.is_cuda and t.is_cuda and q.dtype == torch.float32 and t.dtype == torch.float32
    assert q.stride(2) == 1 and t.stride(2) == 1 and q.shape[0] == t.shape[0] and q.shape[2] == t.shape[2]
    B, nq, dim = q.shape
    nt = t.shape[1]
    ctx = ctx or default_context(q.device.index or 0)
    k = 2 if ratio_test else 1
    if out is None:
        rows = max(nq, 1)   # (nq = 0 is a valid call, and an empty tensor has no address: the library gets the blocks, the caller the views)
        out = {
            "idx": torch.empty((B, rows, k), dtype=torch.int32, device=q.device),
            "dist": torch.empty((B, rows, k), dtype=torch.float32, device=q.device),
            "matches": torch.empty((B, rows, 4), dtype=torch.int32, device=q.device),
            "count": torch.empty((B,), dtype=torch.int32, device=q.device),
        }
    rc = ctx.lib.mlpl_match_l2_dev(
        ctx.handle, q.data_ptr() or t.data_ptr(), nq, q.stride(1), q.stride(0), t.data_ptr(), nt, t.stride(1), t.stride(0), dim,
        1 if ratio_test else 0, ratio, B, out["idx"].data_ptr(), out["dist"].data_ptr(), out["matches"].data_ptr(),
        out["count"].data_ptr(), torch.cuda.current_stream(q.device).cuda_stream if stream is None else stream)
    check(rc, "mlpl_match_l2_dev")
    if nq == 0:
        out = {k_: (v[:, :0] if k_ != "count" else v) for k_, v in out.items()}
    return out


def vfc_filter_matches_device(matches, count, kp1, kp2, seeds=None, getmatches_rule: bool = False, ctx: Optional[Context] = None, out=None,
                              stream: Optional[int] = None):
    """Batched VFC filter on device-resident match lists (mlpl_vfc_filter_matches_dev), the step between match_hamming_device /
    match_l2_device and the gather.  matches: int32 [B, stride, 4] (DMatch rows), count: int32 [B], kp1: float32 [B, nq, 2], kp2:
    float32 [B, nt, 2] CUDA/HIP tensors; seeds: one per problem (host) or None (all 1).  Returns dict of torch tensors matches
    [B, stride, 4] (the kept matches, compacted in order), count [B], status [B] (0, -1: fewer than 5, passed through, -2: fewer than
    10 % kept).  getmatches_rule: pass a list through unless status is 0 and (kept > 8 or n < 24).  Enqueues on `stream` (None = torch's
    current stream) without synchronising."""
    import torch

    if matches.dim() == 2:
        matches, count, kp1, kp2 = matches.unsqueeze(0), count.reshape(1), kp1.unsqueeze(0), kp2.unsqueeze(0)
    assert matches.is_cuda and matches.dtype == torch.int32 and matches.is_contiguous() and matches.shape[2] == 4
    assert count.is_cuda and count.dtype == torch.int32 and count.is_contiguous()
    assert kp1.is_cuda and kp2.is_cuda and kp1.dtype == torch.float32 and kp2.dtype == torch.float32 and kp1.is_contiguous() and kp2.is_contiguous()
    B, stride = matches.shape[0], matches.shape[1]
    assert count.shape == (B,) and kp1.shape[0] == B and kp2.shape[0] == B and kp1.shape[2] == 2 and kp2.shape[2] == 2
    ctx = ctx or default_context(matches.device.index or 0)
    sd = None if seeds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, np.uint32), (B,)))
    if out is None:
        out = {
            "matches": torch.empty_like(matches),
            "count": torch.empty((B,), dtype=torch.int32, device=matches.device),
            "status": torch.empty((B,), dtype=torch.int32, device=matches.device),
        }
    rc = ctx.lib.mlpl_vfc_filter_matches_dev(
        ctx.handle, B, matches.data_ptr(), stride, count.data_ptr(), kp1.data_ptr(), kp1.shape[1], kp2.data_ptr(), kp2.shape[1],
        None if sd is None else sd.ctypes.data, 1 if getmatches_rule else 0, out["matches"].data_ptr(), out["count"].data_ptr(),
        out["status"].data_ptr(), torch.cuda.current_stream(matches.device).cuda_stream if stream is None else stream)
    check(rc, "mlpl_vfc_filter_matches_dev")
    return out


# ---- GMS match filter ------------------------------------------------------------------------------------------

def gms_filter(kp1, size1, kp2, size2, matches, use_scale: bool = False, use_rotation: bool = False, ctx: Optional[Context] = None) -> dict:
    """mlpl_gms_filter (matchinglib::filterMatchesGMS, the inlier-mask overload) -> dict(keep bool [n], n_keep, scale, rotation, dropped).
    kp1 / kp2: keypoint coordinates ([n, 2] arrays, (x, y) pairs or objects with .pt); size1 / size2: (width, height) of the images;
    matches: DMATCH_DTYPE rows.  scale / rotation: the winning scale level / rotation type, -1 when no run found an inlier (n_keep 0);
    dropped: matches the out-of-bounds rule dropped in the winning run (include/mlpl_c.h)."""
    ctx = ctx or default_context()
    a, b = _keypoint_xy(kp1), _keypoint_xy(kp2)
    matches = np.ascontiguousarray(matches, DMATCH_DTYPE)
    n = len(matches)
    keep, info, nk = np.zeros(max(n, 1), np.uint8), np.zeros(4, np.int32), C.c_int(0)
    rc = ctx.lib.mlpl_gms_filter(ctx.handle, a.ctypes.data, a.shape[0], int(size1[0]), int(size1[1]), b.ctypes.data, b.shape[0], int(size2[0]),
                                 int(size2[1]), matches.ctypes.data, n, 1 if use_scale else 0, 1 if use_rotation else 0, keep.ctypes.data,
                                 C.byref(nk), info.ctypes.data)
    check(rc, "mlpl_gms_filter")
    return dict(keep=keep[:n].astype(bool), n_keep=nk.value, scale=int(info[0]), rotation=int(info[1]), dropped=int(info[2]))


def filter_matches_gms(kp1, size1, kp2, size2, matches, use_scale: bool = False, use_rotation: bool = False,
                       ctx: Optional[Context] = None) -> Tuple[int, np.ndarray]:
    """matchinglib::filterMatchesGMS, the matches_filtered overload -> (n, matches_out): the kept matches in order (empty when n is 0)."""
    matches = np.ascontiguousarray(matches, DMATCH_DTYPE)
    r = gms_filter(kp1, size1, kp2, size2, matches, use_scale, use_rotation, ctx)
    return r["n_keep"], matches[r["keep"]].copy()


def gms_filter_matches_device(matches, count, kp1, kp2, size1, size2, use_scale: bool = False, use_rotation: bool = False,
                              min_final_rule: bool = False, ctx: Optional[Context] = None, out=None, stream: Optional[int] = None):
    """Batched GMS filter on device-resident match lists (mlpl_gms_filter_matches_dev), the step between match_hamming_device /
    match_l2_device and the gather.  matches: int32 [B, stride, 4] (DMatch rows), count: int32 [B], kp1: float32 [B, nq, 2], kp2:
    float32 [B, nt, 2] CUDA/HIP tensors; size1 / size2: (width, height).  Returns dict of torch tensors matches [B, stride, 4] (the kept
    matches, compacted in order), count [B], inliers [B] (the filter's count).  min_final_rule: a list passes through unchanged unless
    the filter kept at least 2 matches.  Enqueues on `stream` (None = torch's current stream) without synchronising."""
    import torch

    if matches.dim() == 2:
        matches, count, kp1, kp2 = matches.unsqueeze(0), count.reshape(1), kp1.unsqueeze(0), kp2.unsqueeze(0)
    assert matches.is_cuda and matches.dtype == torch.int32 and matches.is_contiguous() and matches.shape[2] == 4
    assert count.is_cuda and count.dtype == torch.int32 and count.is_contiguous()
    assert kp1.is_cuda and kp2.is_cuda and kp1.dtype == torch.float32 and kp2.dtype == torch.float32 and kp1.is_contiguous() and kp2.is_contiguous()
    B, stride = matches.shape[0], matches.shape[1]
    assert count.shape == (B,) and kp1.shape[0] == B and kp2.shape[0] == B and kp1.shape[2] == 2 and kp2.shape[2] == 2
    ctx = ctx or default_context(matches.device.index or 0)
    if out is None:
        out = {
            "matches": torch.empty_like(matches),
            "count": torch.empty((B,), dtype=torch.int32, device=matches.device),
            "inliers": torch.empty((B,), dtype=torch.int32, device=matches.device),
        }
    rc = ctx.lib.mlpl_gms_filter_matches_dev(
        ctx.handle, B, matches.data_ptr(), stride, count.data_ptr(), kp1.data_ptr(), kp1.shape[1], kp2.data_ptr(), kp2.shape[1],
        int(size1[0]), int(size1[1]), int(size2[0]), int(size2[1]), 1 if use_scale else 0, 1 if use_rotation else 0,
        1 if min_final_rule else 0, out["matches"].data_ptr(), out["count"].data_ptr(), out["inliers"].data_ptr(),
        torch.cuda.current_stream(matches.device).cuda_stream if stream is None else stream)
    check(rc, "mlpl_gms_filter_matches_dev")
    return out


# ---- sub-pixel refinement -----------------------------------------------------------------------------------------

def _image_u8(img) -> np.ndarray:
    """an 8-bit single-channel image with contiguous pixels inside each row (the row step may exceed the width)"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
        raise MlplError(-1, "subpix_matches", "images are 8-bit, single channel and not empty")
    if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img)
    return img


def subpix_matches(img1, img2, kp1, kp2, size1=None, size2=None, ctx: Optional[Context] = None) -> dict:
    """mlpl_subpix_matches (matchinglib::getSubPixMatches) -> dict(status, kp2 float32 [n, 2], inlier bool [n], n_refined, dropped_border,
    dropped_side, dropped_coord, max_side).  img1 / img2: uint8 [height, width] arrays (rows may be strided views); kp1 / kp2: matched
    keypoint coordinates, index by index ([n, 2] arrays, (x, y) pairs or objects with .pt); size1 / size2: the keypoints' sizes [n] or None
    (all 0: a 17 x 17 template).  status: 0, or -1 when fewer than n / 3 or fewer than 2 matches were refined (kp2 and inlier are filled in
    either way).  The declared deviations from the reference: include/mlpl_c.h."""
    ctx = ctx or default_context()
    i1, i2 = _image_u8(img1), _image_u8(img2)
    a = _keypoint_xy(kp1)
    b = np.array(_keypoint_xy(kp2), np.float32, copy=True)
    n = a.shape[0]
    if b.shape[0] != n:
        raise MlplError(-1, "subpix_matches", "the keypoint lists must have the same length")
    s1 = None if size1 is None else np.ascontiguousarray(size1, np.float32).reshape(-1)
    s2 = None if size2 is None else np.ascontiguousarray(size2, np.float32).reshape(-1)
    if (s1 is not None and len(s1) != n) or (s2 is not None and len(s2) != n):
        raise MlplError(-1, "subpix_matches", "one size per keypoint")
    inl, info, nr, st = np.zeros(max(n, 1), np.uint8), np.zeros(4, np.int32), C.c_int(0), C.c_int(0)
    rc = ctx.lib.mlpl_subpix_matches(ctx.handle, i1.ctypes.data, i1.shape[1], i1.shape[0], i1.strides[0], i2.ctypes.data, i2.shape[1],
                                     i2.shape[0], i2.strides[0], a.ctypes.data, b.ctypes.data, None if s1 is None else s1.ctypes.data,
                                     None if s2 is None else s2.ctypes.data, n, inl.ctypes.data, C.byref(nr), C.byref(st), info.ctypes.data)
    check(rc, "mlpl_subpix_matches")
    return dict(status=st.value, kp2=b, inlier=inl[:n].astype(bool), n_refined=nr.value, dropped_border=int(info[0]), dropped_side=int(info[1]),
                dropped_coord=int(info[2]), max_side=int(info[3]))


def subpix_template_side(size1: float, size2: float, ctx: Optional[Context] = None) -> int:
    """mlpl_subpix_template_side: the template side for a pair of keypoint sizes (17 ... 255), 0 when the side rule drops the match"""
    ctx = ctx or default_context()
    return int(ctx.lib.mlpl_subpix_template_side(float(size1), float(size2)))


def subpix_matches_device(matches, count, kp1, kp2, img1, img2, size1=None, size2=None, max_side: int = 0, correspondences_rule: bool = False,
                          ctx: Optional[Context] = None, out=None, stream: Optional[int] = None):
    """Batched sub-pixel refinement on device-resident match lists (mlpl_subpix_matches_dev), the step behind match_hamming_device /
    match_l2_device and the VFC / GMS filters and in front of the gather.  matches: int32 [B, stride, 4] (DMatch rows), count: int32 [B],
    kp1: float32 [B, nq, 2], kp2: float32 [B, nt, 2], img1 / img2: uint8 [B, height, width] (the last dimension contiguous; row and batch
    strides are passed on), size1 / size2: float32 [B, nq] / [B, nt] or None -- CUDA/HIP tensors.  max_side: the largest template side to
    provision for (0 = 255; 17 is enough without sizes).  Returns dict of torch tensors matches [B, stride, 4] (the inliers, compacted),
    count [B], status [B], kp2 [B, nt, 2] (every match's refined or unchanged position at its train keypoint, the last match of a keypoint
    wins), inlier uint8 [B, stride].  correspondences_rule: correspondences.cpp:474-494 -- on status -1 list and keypoints pass through,
    on status 0 the inliers come in reverse list order.  Enqueues on `stream` (None = torch's current stream) without synchronising."""
    import torch

    if matches.dim() == 2:
        matches, count, kp1, kp2, img1, img2 = matches.unsqueeze(0), count.reshape(1), kp1.unsqueeze(0), kp2.unsqueeze(0), img1.unsqueeze(0), img2.unsqueeze(0)
        size1 = None if size1 is None else size1.unsqueeze(0)
        size2 = None if size2 is None else size2.unsqueeze(0)
    assert matches.is_cuda and matches.dtype == torch.int32 and matches.is_contiguous() and matches.shape[2] == 4
    assert count.is_cuda and count.dtype == torch.int32 and count.is_contiguous()
    assert kp1.is_cuda and kp2.is_cuda and kp1.dtype == torch.float32 and kp2.dtype == torch.float32 and kp1.is_contiguous() and kp2.is_contiguous()
    B, stride = matches.shape[0], matches.shape[1]
    assert count.shape == (B,) and kp1.shape[0] == B and kp2.shape[0] == B and kp1.shape[2] == 2 and kp2.shape[2] == 2
    for im in (img1, img2):
        assert im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[0] == B and im.stride(2) == 1 and im.stride(1) >= im.shape[2]
    for sz, k in ((size1, kp1), (size2, kp2)):
        assert sz is None or (sz.is_cuda and sz.dtype == torch.float32 and sz.is_contiguous() and sz.shape == k.shape[:2])
    ctx = ctx or default_context(matches.device.index or 0)
    if out is None:
        out = {
            "matches": torch.empty_like(matches),
            "count": torch.empty((B,), dtype=torch.int32, device=matches.device),
            "status": torch.empty((B,), dtype=torch.int32, device=matches.device),
            "kp2": torch.empty_like(kp2),
            "inlier": torch.zeros((B, stride), dtype=torch.uint8, device=matches.device),
        }
    rc = ctx.lib.mlpl_subpix_matches_dev(
        ctx.handle, B, matches.data_ptr(), stride, count.data_ptr(), kp1.data_ptr(), kp1.shape[1], kp2.data_ptr(), kp2.shape[1],
        None if size1 is None else size1.data_ptr(), None if size2 is None else size2.data_ptr(),
        img1.data_ptr(), img1.shape[2], img1.shape[1], img1.stride(1), img1.stride(0) if B > 1 else 0,
        img2.data_ptr(), img2.shape[2], img2.shape[1], img2.stride(1), img2.stride(0) if B > 1 else 0, int(max_side),
        1 if correspondences_rule else 0, out["matches"].data_ptr(), out["count"].data_ptr(), out["status"].data_ptr(), out["kp2"].data_ptr(),
        out["inlier"].data_ptr(), torch.cuda.current_stream(matches.device).cuda_stream if stream is None else stream)
    check(rc, "mlpl_subpix_matches_dev")
    return out


def subpix_separate(img1, img2, kp1, kp2, size1=None, size2=None, ctx: Optional[Context] = None) -> dict:
    """mlpl_subpix_separate (matchinglib::getSubPixMatches_seperate_Imgs: cv::cornerSubPix on each image on its own) -> dict(status,
    kp1, kp2 float32 [n, 2], inlier bool [n], iters int32 [n, 2], n_refined, w1, w2, dropped_coord, reset_far).  Arguments as subpix_matches;
    the smallest positive size of a list sets the window half-size of its image (3 ... 10; None: 10).  status: 0, or -1 when fewer than
    n / 3 or fewer than 2 matches stayed within sqrt(12) px (kp1, kp2 and inlier are filled in either way).  iters: loop passes per match
    and image.  The contract and its declared deviations: include/mlpl_c.h."""
    ctx = ctx or default_context()
    try:
        i1, i2 = _image_u8(img1), _image_u8(img2)
    except MlplError as e:
        raise MlplError(e.code, "subpix_separate", "images are 8-bit, single channel and not empty") from None
    a = np.array(_keypoint_xy(kp1), np.float32, copy=True)
    b = np.array(_keypoint_xy(kp2), np.float32, copy=True)
    n = a.shape[0]
    if b.shape[0] != n:
        raise MlplError(-1, "subpix_separate", "the keypoint lists must have the same length")
    s1 = None if size1 is None else np.ascontiguousarray(size1, np.float32).reshape(-1)
    s2 = None if size2 is None else np.ascontiguousarray(size2, np.float32).reshape(-1)
    if (s1 is not None and len(s1) != n) or (s2 is not None and len(s2) != n):
        raise MlplError(-1, "subpix_separate", "one size per keypoint")
    inl, its, info, nr, st = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 2), np.int32), np.zeros(4, np.int32), C.c_int(0), C.c_int(0)
    rc = ctx.lib.mlpl_subpix_separate(ctx.handle, i1.ctypes.data, i1.shape[1], i1.shape[0], i1.strides[0], i2.ctypes.data, i2.shape[1],
                                      i2.shape[0], i2.strides[0], a.ctypes.data, b.ctypes.data, None if s1 is None else s1.ctypes.data,
                                      None if s2 is None else s2.ctypes.data, n, inl.ctypes.data, its.ctypes.data, C.byref(nr), C.byref(st),
                                      info.ctypes.data)
    check(rc, "mlpl_subpix_separate")
    return dict(status=st.value, kp1=a, kp2=b, inlier=inl[:n].astype(bool), iters=its[:n], n_refined=nr.value, w1=int(info[0]), w2=int(info[1]),
                dropped_coord=int(info[2]), reset_far=int(info[3]))


def subpix_separate_window(min_size: float, ctx: Optional[Context] = None) -> int:
    """mlpl_subpix_separate_window: the window half-size (3 ... 10) for the smallest positive keypoint size of a list"""
    ctx = ctx or default_context()
    return int(ctx.lib.mlpl_subpix_separate_window(float(min_size)))


def subpix_separate_device(matches, count, kp1, kp2, img1, img2, size1=None, size2=None, correspondences_rule: bool = False,
                           ctx: Optional[Context] = None, out=None, stream: Optional[int] = None):
    """Batched cornerSubPix refinement on device-resident match lists (mlpl_subpix_separate_dev); tensors as subpix_matches_device (images of
    at least 25 x 25 pixels).  Returns dict of torch tensors matches [B, stride, 4] (the inliers, compacted), count [B], status [B],
    kp1 [B, nq, 2] and kp2 [B, nt, 2] (every match's refined or unchanged position at its keypoint, the last match of a keypoint wins; under
    correspondences_rule kp1 is a copy of the input), inlier uint8 [B, stride].  correspondences_rule: correspondences.cpp:474-494 -- on
    status -1 list and keypoints pass through, on status 0 the inliers come in reverse list order.  Enqueues on `stream` (None = torch's
    current stream) without synchronising."""
    import torch

    if matches.dim() == 2:
        matches, count, kp1, kp2, img1, img2 = matches.unsqueeze(0), count.reshape(1), kp1.unsqueeze(0), kp2.unsqueeze(0), img1.unsqueeze(0), img2.unsqueeze(0)
        size1 = None if size1 is None else size1.unsqueeze(0)
        size2 = None if size2 is None else size2.unsqueeze(0)
    assert matches.is_cuda and matches.dtype == torch.int32 and matches.is_contiguous() and matches.shape[2] == 4
    assert count.is_cuda and count.dtype == torch.int32 and count.is_contiguous()
    assert kp1.is_cuda and kp2.is_cuda and kp1.dtype == torch.float32 and kp2.dtype == torch.float32 and kp1.is_contiguous() and kp2.is_contiguous()
    B, stride = matches.shape[0], matches.shape[1]
    assert count.shape == (B,) and kp1.shape[0] == B and kp2.shape[0] == B and kp1.shape[2] == 2 and kp2.shape[2] == 2
    for im in (img1, img2):
        assert im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[0] == B and im.stride(2) == 1 and im.stride(1) >= im.shape[2]
    for sz, k in ((size1, kp1), (size2, kp2)):
        assert sz is None or (sz.is_cuda and sz.dtype == torch.float32 and sz.is_contiguous() and sz.shape == k.shape[:2])
    ctx = ctx or default_context(matches.device.index or 0)
    if out is None:
        out = {
            "matches": torch.empty_like(matches),
            "count": torch.empty((B,), dtype=torch.int32, device=matches.device),
            "status": torch.empty((B,), dtype=torch.int32, device=matches.device),
            "kp1": torch.empty_like(kp1),
            "kp2": torch.empty_like(kp2),
            "inlier": torch.zeros((B, stride), dtype=torch.uint8, device=matches.device),
        }
    rc = ctx.lib.mlpl_subpix_separate_dev(
        ctx.handle, B, matches.data_ptr(), stride, count.data_ptr(), kp1.data_ptr(), kp1.shape[1], kp2.data_ptr(), kp2.shape[1],
        None if size1 is None else size1.data_ptr(), None if size2 is None else size2.data_ptr(),
        img1.data_ptr(), img1.shape[2], img1.shape[1], img1.stride(1), img1.stride(0) if B > 1 else 0,
        img2.data_ptr(), img2.shape[2], img2.shape[1], img2.stride(1), img2.stride(0) if B > 1 else 0,
        1 if correspondences_rule else 0, out["matches"].data_ptr(), out["count"].data_ptr(), out["status"].data_ptr(),
        None if out.get("kp1") is None else out["kp1"].data_ptr(), out["kp2"].data_ptr(), out["inlier"].data_ptr(),
        torch.cuda.current_stream(matches.device).cuda_stream if stream is None else stream)
    check(rc, "mlpl_subpix_separate_dev")
    return out
