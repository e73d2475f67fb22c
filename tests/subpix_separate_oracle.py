"""numpy restatement of matchinglib::getSubPixMatches_seperate_Imgs as include/mlpl_c.h states it (cv::cornerSubPix restated: the five steps,
the summation order of step 3c as explicit loops, the declared deviations), and of the batched entry's composition (last writer per
keypoint, reverse order under the rule of correspondences.cpp:474-494).  float32 and float64 numpy arithmetic rounds every operation on
its own; the points of one image are iterated together, each with its own trajectory."""
import numpy as np

DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
MAX_ITER = 40
EPS2 = 1e-6
SINGULAR = np.finfo(np.float64).eps * np.finfo(np.float64).eps


def window(min_size) -> int:
    """step 1's clamp and ceil on a float32"""
    m = F32(min_size)
    m = F32(20.0) if m > F32(20.0) else m
    m = F32(6.0) if m < F32(6.0) else m
    if np.isnan(m):
        m = F32(20.0)
    return int(np.ceil(m / F32(2.0)))


def list_window(sizes) -> int:
    """step 1 for the sizes of one image's points (None: no size array)"""
    m = FLT_MAX
    if sizes is not None:
        for s in np.asarray(sizes, F32).reshape(-1):
            if s > 0 and s < m:          # NaN and non-positive sizes never compare true
                m = s
    return window(m)


def profile(w: int) -> np.ndarray:
    """step 2: g[i] = (float)exp(-(double)(y * y)), float y = (float)(i - w) / w"""
    y = (np.arange(2 * w + 1) - w).astype(F32) / F32(w)
    return np.exp(-((y * y).astype(np.float64))).astype(F32)


def wave_sum(terms: np.ndarray) -> np.ndarray:
    """step 3c over the last axis: lane l = k mod 64 adds its terms in increasing k starting from its first one (lanes without terms hold
    +0.0), then v[l] = v[l] + v[l + s] for s = 32 ... 1"""
    K = terms.shape[-1]
    v = np.zeros(terms.shape[:-1] + (64,), np.float64)
    for t in range((K + 63) // 64):
        chunk = terms[..., 64 * t:64 * t + 64]
        L = chunk.shape[-1]
        if t == 0:
            v[..., :L] = chunk
        else:
            v[..., :L] = v[..., :L] + chunk
    for s in (32, 16, 8, 4, 2, 1):
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
    return v[..., 0]


def coordinate_ok(pts: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (np.isfinite(pts) & (pts >= F32(-2147483648.0)) & (pts < F32(2147483648.0))).all(axis=1)


def sample(img: np.ndarray, cI: np.ndarray, w: int) -> np.ndarray:
    """step 3a for points cI [m, 2] -> S float32 [m, 2w + 3, 2w + 3]"""
    rows, cols = img.shape
    PS = 2 * w + 4
    one = F32(1.0)
    cx, cy = cI[:, 0] - F32(w + 1), cI[:, 1] - F32(w + 1)
    fx, fy = np.floor(cx), np.floor(cy)
    a, b = (cx - fx)[:, None, None], (cy - fy)[:, None, None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    X = np.clip(ix[:, None] + np.arange(PS)[None, :], 0, cols - 1)
    Y = np.clip(iy[:, None] + np.arange(PS)[None, :], 0, rows - 1)
    P = img[Y[:, :, None], X[:, None, :]].astype(F32)
    a11, a12, a21, a22 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    S = ((P[:, :-1, :-1] * a11 + P[:, :-1, 1:] * a12) + P[:, 1:, :-1] * a21) + P[:, 1:, 1:] * a22
    assert S.dtype == F32
    return S


def sums(S: np.ndarray, w: int) -> np.ndarray:
    """steps 3b and 3c -> [m, 5] = a, b, c, bb1, bb2"""
    W = 2 * w + 1
    g = profile(w)
    mask = (g[:, None] * g[None, :]).astype(np.float64)
    assert (g[:, None] * g[None, :]).dtype == F32
    D = S.astype(np.float64)
    tgx = D[:, 1:-1, 2:] - D[:, 1:-1, :-2]
    tgy = D[:, 2:, 1:-1] - D[:, :-2, 1:-1]
    gxx, gxy, gyy = (tgx * tgx) * mask, (tgx * tgy) * mask, (tgy * tgy) * mask
    px = (np.arange(W) - w).astype(np.float64)[None, None, :]
    py = (np.arange(W) - w).astype(np.float64)[None, :, None]
    terms = np.stack([gxx, gxy, gyy, gxx * px + gxy * py, gxy * px + gyy * py], axis=1)
    return wave_sum(terms.reshape(len(S), 5, W * W))


def refine(img, pts, w: int):
    """step 3 for the points [n, 2] of one image -> (refined float32 [n, 2], iters int32 [n], dropped bool [n], far bool [n], left bool [n]:
    the loop ended in step 3f, singular bool [n]: it ended in step 3d)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    rows, cols = img.shape
    assert cols >= 2 * w + 5 and rows >= 2 * w + 5, "MLPL_E_BAD_INPUT"
    cT = np.asarray(pts, F32).reshape(-1, 2)
    n = len(cT)
    cI = cT.copy()
    iters = np.zeros(n, np.int32)
    dropped = ~coordinate_ok(cT)
    nonfinite, left, sing = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    active = ~dropped
    while active.any():
        idx = np.nonzero(active)[0]
        r = sums(sample(img, cI[idx], w), w)
        a, b, c, bb1, bb2 = r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4]
        with np.errstate(all="ignore"):
            det = a * c - b * b
            singular = np.abs(det) <= SINGULAR
            scale = 1.0 / det
            nx = ((cI[idx, 0].astype(np.float64) + (c * scale) * bb1) - (b * scale) * bb2).astype(F32)
            ny = ((cI[idx, 1].astype(np.float64) - (b * scale) * bb1) + (a * scale) * bb2).astype(F32)
            bad = ~singular & ~(np.isfinite(nx) & np.isfinite(ny))
            move = ~singular & ~bad
            ex, ey = nx - cI[idx, 0], ny - cI[idx, 1]
            err = (ex * ex + ey * ey).astype(np.float64)
        nonfinite[idx[bad]] = True
        cI[idx[move], 0], cI[idx[move], 1] = nx[move], ny[move]
        x, y = cI[idx, 0], cI[idx, 1]
        inside = ~((x < 0) | (x >= F32(cols)) | (y < 0) | (y >= F32(rows)))
        go = move & inside
        left[idx[move & ~inside]] = True
        sing[idx[singular]] = True
        iters[idx[go]] += 1
        go &= (iters[idx] < MAX_ITER) & (err > EPS2)
        active[idx] = go
    with np.errstate(invalid="ignore"):
        far = ~dropped & ~nonfinite & ((np.abs(cI[:, 0] - cT[:, 0]) > F32(w)) | (np.abs(cI[:, 1] - cT[:, 1]) > F32(w)))
    out = np.where((dropped | nonfinite | far)[:, None], cT, cI)
    return out, iters, dropped, far, left, sing


def subpix(img1, img2, kp1, kp2, size1=None, size2=None):
    """-> dict(inlier uint8 [n], kp1, kp2 float32 [n, 2], iters int32 [n, 2], n_refined, status, info [w1, w2, dropped points, points reset
    by the "too far" rule]; raw1, raw2: the refined points in front of step 4; far, left, singular bool [n, 2]: how step 3 ended)"""
    kp1 = np.array(kp1, F32).reshape(-1, 2)
    kp2 = np.array(kp2, F32).reshape(-1, 2)
    n = len(kp1)
    assert len(kp2) == n
    w1, w2 = list_window(size1), list_window(size2)
    r1, it1, drop1, far1, left1, sing1 = refine(img1, kp1, w1)
    r2, it2, drop2, far2, left2, sing2 = refine(img2, kp2, w2)
    with np.errstate(invalid="ignore"):
        e1, e2 = kp1 - r1, kp2 - r2
        d1 = e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1]
        d2 = e2[:, 0] * e2[:, 0] + e2[:, 1] * e2[:, 1]
        inlier = ~drop1 & ~drop2 & ~((d1 > F32(12.0)) | (d2 > F32(12.0)))
    assert d1.dtype == F32
    o1, o2 = np.where(inlier[:, None], r1, kp1), np.where(inlier[:, None], r2, kp2)
    n_refined = int(inlier.sum())
    status = -1 if (n_refined < n // 3 or n_refined < 2) else 0
    info = [w1, w2, int(drop1.sum() + drop2.sum()), int(far1.sum() + far2.sum())]
    return dict(inlier=inlier.astype(np.uint8), kp1=o1, kp2=o2, iters=np.stack([it1, it2], axis=1).astype(np.int32), n_refined=n_refined,
                status=status, info=info, raw1=r1, raw2=r2, far=np.stack([far1, far2], axis=1), left=np.stack([left1, left2], axis=1),
                singular=np.stack([sing1, sing2], axis=1))


def compose(img1, img2, matches, kp1, kp2, size1=None, size2=None, rule=False):
    """the batched entry on one list: matches (DMATCH rows) on keypoint arrays kp1 [nq, 2], kp2 [nt, 2] (indices outside are clamped)
    -> dict(matches: the emitted list, status, kp1_out [nq, 2], kp2_out [nt, 2], inlier uint8 [n], n_refined, single: the result of subpix on
    the gathered keypoints)"""
    kp1, kp2 = np.asarray(kp1, F32), np.asarray(kp2, F32)
    q = np.clip(matches["queryIdx"], 0, len(kp1) - 1)
    t = np.clip(matches["trainIdx"], 0, len(kp2) - 1)
    r = subpix(img1, img2, kp1[q], kp2[t], None if size1 is None else np.asarray(size1, F32)[q],
               None if size2 is None else np.asarray(size2, F32)[t])
    kp1_out, kp2_out = kp1.copy(), kp2.copy()
    keep = r["inlier"].astype(bool)
    if rule and r["status"] != 0:
        out = matches.copy()
    else:
        for i in range(len(matches)):            # in list order, so the last match of a keypoint wins
            kp2_out[t[i]] = r["kp2"][i]
            if not rule:                         # correspondences.cpp:480-483 takes the keypoints 2 only
                kp1_out[q[i]] = r["kp1"][i]
        out = matches[keep][::-1].copy() if rule else matches[keep].copy()
    return dict(matches=out, status=r["status"], kp1_out=kp1_out, kp2_out=kp2_out, inlier=r["inlier"], n_refined=r["n_refined"], single=r)
