"""numpy restatement of matchinglib::getSubPixMatches as include/mlpl_c.h states it (the seven steps and the declared deviations), and of the
batched entry's composition (last writer per train keypoint, reverse order under the rule of correspondences.cpp:474-494).
Sums are int64, the fit is np.float32 arithmetic with every operation rounded on its own; matches of one side are handled together with
sliding windows."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

BORDER = 100
DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


def cv_round(x):
    """cvRound of float32 values: round half to even"""
    return np.rint(np.asarray(x, np.float32)).astype(np.int64)


def side_literal(fs: int):
    """matchers.cpp:1156-1165 as written, for featuresize1 = fs >= 18 -> (side, diff1)"""
    half = np.float32(fs) / np.float32(2.0)
    rounded = np.float32(np.rint(half))   # cvRound
    diff1 = int(half) if (rounded - half) != 0.0 else int(half) - 1
    if (rounded - half) == 0.0:
        fs -= 1
    return fs, diff1


def side_reduced(fs: int):
    """the same in the reduced form of the contract -> (side, d1)"""
    if fs % 2 == 0:
        fs -= 1
    return fs, (fs - 1) // 2


def template_sides(size1, size2):
    """step 1 for arrays of float32 sizes -> int sides; 0 where the side rule drops the match"""
    a, b = np.asarray(size1, np.float32), np.asarray(size2, np.float32)
    with np.errstate(invalid="ignore"):
        m = np.where(a > b, a, b)                      # the reference's a > b ? a : b
        big = m >= np.float32(251.0)                   # (int)m + 6 > 256
        fs = np.where(m >= np.float32(12.0), np.where(big, 0.0, m).astype(np.int64) + 6, 18)   # NaN, negatives and < 12 end at the clamp
    fs = np.where(fs % 2 == 0, fs - 1, fs)
    return np.where(big, 0, fs).astype(np.int64)


def _tables(img1, img2, r1, r2, fs):
    """exact integer tables [m, 11, 11] of m matches of one side; r1 / r2: [m, 2] rectangle origins (x, y)"""
    p1 = np.pad(img1, BORDER)
    p2 = np.pad(img2, BORDER)
    m = len(r1)
    out = np.empty((m, 11, 11), np.int64)
    chunk = max(1, (16 << 20) // (121 * fs * fs))
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        T = np.stack([p1[y + BORDER:y + BORDER + fs, x + BORDER:x + BORDER + fs] for x, y in r1[s:e]]).astype(np.int32)
        W = np.stack([p2[y + BORDER:y + BORDER + fs + 10, x + BORDER:x + BORDER + fs + 10] for x, y in r2[s:e]]).astype(np.int32)
        win = sliding_window_view(W, (fs, fs), axis=(1, 2))           # [c, 11, 11, fs, fs]
        d = win - T[:, None, None]
        out[s:e] = (d * d).sum(axis=(3, 4), dtype=np.int64)
    return out


def subpix(img1, img2, kp1, kp2, size1=None, size2=None, tables=False):
    """-> dict(inlier uint8 [n], kp2 float32 [n, 2], n_refined, status, info [4]; with tables: table int64 [n, 11, 11] (0 for dropped matches),
    refined bool [n], nx, ny float32 [n] (the denominators, 1 for matches that are not inliers))"""
    img1, img2 = np.asarray(img1), np.asarray(img2)
    assert img1.dtype == np.uint8 and img2.dtype == np.uint8 and img1.ndim == 2 and img2.ndim == 2
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 2)
    kp2 = np.array(kp2, np.float32).reshape(-1, 2)
    n = len(kp1)
    assert len(kp2) == n
    s1 = np.zeros(n, np.float32) if size1 is None else np.asarray(size1, np.float32)
    s2 = np.zeros(n, np.float32) if size2 is None else np.asarray(size2, np.float32)
    fs = template_sides(s1, s2)
    xy = np.concatenate([kp1, kp2], axis=1)
    with np.errstate(invalid="ignore"):
        coord_ok = (np.isfinite(xy) & (xy >= np.float32(-2147483648.0)) & (xy < np.float32(2147483648.0))).all(axis=1)
    drop_coord = ~coord_ok
    drop_side = coord_ok & (fs == 0)
    live = coord_ok & (fs > 0)
    c = np.zeros((n, 4), np.int64)
    c[live] = cv_round(xy[live])
    d1 = (fs - 1) // 2
    r1 = c[:, 0:2] - d1[:, None]
    r2 = c[:, 2:4] - (d1 + 5)[:, None]
    (h1, w1), (h2, w2) = img1.shape, img2.shape
    inside = ((r1[:, 0] >= -BORDER) & (r1[:, 1] >= -BORDER) & (r1[:, 0] + fs <= w1 + BORDER) & (r1[:, 1] + fs <= h1 + BORDER) &
              (r2[:, 0] >= -BORDER) & (r2[:, 1] >= -BORDER) & (r2[:, 0] + fs + 10 <= w2 + BORDER) & (r2[:, 1] + fs + 10 <= h2 + BORDER))
    drop_border = live & ~inside
    live &= inside

    table = np.zeros((n, 11, 11), np.int64)
    for f in np.unique(fs[live]):
        idx = np.nonzero(live & (fs == f))[0]
        table[idx] = _tables(img1, img2, r1[idx], r2[idx], int(f))
    assert table.max(initial=0) < 2 ** 32
    R = table.astype(np.float32).reshape(n, 121)          # round to nearest even: the element type of cv::matchTemplate's result
    pm = np.argmin(R, axis=1)                             # the first minimum in row-major order
    my, mx = pm // 11, pm % 11
    inlier = live & ((mx - 5) ** 2 + (my - 5) ** 2 <= 16)
    out = kp2.copy()
    refined = np.zeros(n, bool)
    nx_all, ny_all = np.ones(n, np.float32), np.ones(n, np.float32)
    ii = np.nonzero(inlier)[0]
    if len(ii):
        two = np.float32(2.0)
        cc, xp, xn = R[ii, pm[ii]], R[ii, pm[ii] + 1], R[ii, pm[ii] - 1]
        yp, yn = R[ii, pm[ii] + 11], R[ii, pm[ii] - 11]
        nx = two * ((two * cc - xn) - xp)
        ny = two * ((two * cc - yn) - yp)
        nx_all[ii], ny_all[ii] = nx, ny
        ok = (nx != 0) & (ny != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ox, oy = (xp - xn) / nx, (yp - yn) / ny
        px = (r2[ii, 0] + mx[ii] + d1[ii]).astype(np.float32) + ox
        py = (r2[ii, 1] + my[ii] + d1[ii]).astype(np.float32) + oy
        out[ii[ok], 0], out[ii[ok], 1] = px[ok], py[ok]
        refined[ii[ok]] = True
    n_refined = int(refined.sum())
    status = -1 if (n_refined < n // 3 or n_refined < 2) else 0
    info = [int(drop_border.sum()), int(drop_side.sum()), int(drop_coord.sum()), int(fs[live].max(initial=0))]
    res = dict(inlier=inlier.astype(np.uint8), kp2=out, n_refined=n_refined, status=status, info=info)
    if tables:
        res.update(table=table, refined=refined, nx=nx_all, ny=ny_all)
    return res


def compose(img1, img2, matches, kp1, kp2, size1=None, size2=None, rule=False):
    """the batched entry on one list: matches (DMATCH rows) on keypoint arrays kp1 [nq, 2], kp2 [nt, 2] (indices outside are clamped)
    -> dict(matches: the emitted list, status, kp2_out [nt, 2], inlier uint8 [n], n_refined)"""
    kp1, kp2 = np.asarray(kp1, np.float32), np.asarray(kp2, np.float32)
    q = np.clip(matches["queryIdx"], 0, len(kp1) - 1)
    t = np.clip(matches["trainIdx"], 0, len(kp2) - 1)
    r = subpix(img1, img2, kp1[q], kp2[t], None if size1 is None else np.asarray(size1, np.float32)[q],
               None if size2 is None else np.asarray(size2, np.float32)[t])
    kp2_out = kp2.copy()
    keep = r["inlier"].astype(bool)
    if rule and r["status"] != 0:
        out = matches.copy()
    else:
        for i in range(len(matches)):            # correspondences.cpp:480-483: in list order, so the last match of a train keypoint wins
            kp2_out[t[i]] = r["kp2"][i]
        out = matches[keep][::-1].copy() if rule else matches[keep].copy()
    return dict(matches=out, status=r["status"], kp2_out=kp2_out, inlier=r["inlier"], n_refined=r["n_refined"])
