"""Sequential restatement of the stereo rectification entries (include/mlpl_c.h, "stereo rectification"):

  parameters(...)  poselib::getRectificationParameters with globRectFunct = true (P/source/pose_helper.cpp:1366-1422, rectifyFusiello
                   :1459-1857, cvUndistortPoints2 :2290-2412, icvGetRectanglesV0 :2429-2503) -> mlpl_rectify_parameters
  maps(...)        cv::initUndistortRectifyMap(K, dist, Rect, Knew, size, CV_32FC1)          -> mlpl_rectify_maps
  remap(...)       cv::remap(img, INTER_LINEAR, BORDER_CONSTANT) on 8-bit single channel     -> mlpl_remap_bilinear

Plain Python floats are IEEE doubles and nothing here is contracted, so one operation per line IS the operation order; the C code follows
it line by line.  A float32 value is a double that was passed through f32(); + - * / and sqrt of float32 operands evaluated in double and
rounded once more equal the float32 operation (53 >= 2 * 24 + 2), which is how the float32 arithmetic of the reference is restated.
`inverse` selects how the three 3 x 3 inverses are taken: "cof" (cofactors; what the library does) or "lu" (Gaussian elimination with
partial pivoting); the distance between the two is the yardstick of the parameter test."""
import math

import numpy as np


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------- 3 x 3 helpers (row major lists of 9)
def mul3(a, b):
    c = [0.0] * 9
    for i in range(3):
        for j in range(3):
            s = a[3 * i] * b[j]
            s = s + a[3 * i + 1] * b[3 + j]
            s = s + a[3 * i + 2] * b[6 + j]
            c[3 * i + j] = s
    return c


def mulv3(a, v):
    r = [0.0] * 3
    for i in range(3):
        s = a[3 * i] * v[0]
        s = s + a[3 * i + 1] * v[1]
        s = s + a[3 * i + 2] * v[2]
        r[i] = s
    return r


def inv3_cof(m):
    """adjugate over determinant; every cofactor is a * b - c * d, the determinant is expanded along the first row"""
    c00 = m[4] * m[8] - m[5] * m[7]
    c01 = m[5] * m[6] - m[3] * m[8]
    c02 = m[3] * m[7] - m[4] * m[6]
    det = m[0] * c00
    det = det + m[1] * c01
    det = det + m[2] * c02
    d = 1.0 / det
    return [c00 * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
            c01 * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
            c02 * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]


def inv3_lu(m):
    a = [[m[3 * i + j] for j in range(3)] + [1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for c in range(3):
        p = max(range(c, 3), key=lambda r: abs(a[r][c]))
        a[c], a[p] = a[p], a[c]
        for r in range(c + 1, 3):
            f = a[r][c] / a[c][c]
            for j in range(c, 6):
                a[r][j] = a[r][j] - f * a[c][j]
    out = [0.0] * 9
    for j in range(3):
        x = [0.0] * 3
        for r in (2, 1, 0):
            s = a[r][3 + j]
            for q in range(r + 1, 3):
                s = s - a[r][q] * x[q]
            x[r] = s / a[r][r]
        for r in range(3):
            out[3 * r + j] = x[r]
    return out


# ---------------------------------------------------------------------------------------------------------------- cvUndistortPoints2
def undistort_points(pts, A, k, RR):
    """pts: list of (x, y) float32 values; k: 8 coefficients or None (no coefficients: one pass); RR: 9 values or None (identity).
    -> (list of float32 (x, y), list of valid flags)"""
    iters = 5 if k is not None else 1
    if k is None:
        k = [0.0] * 8
    fx, fy, cx, cy = A[0], A[4], A[2], A[5]
    ifx = 1.0 / fx
    ify = 1.0 / fy
    out, mask = [], []
    for (px, py) in pts:
        x = (px - cx) * ifx
        y = (py - cy) * ify
        x0, y0 = x, y
        for _ in range(iters):
            r2 = x * x + y * y
            icdist = (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            dx = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x)
            dy = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
        r2 = x * x + y * y
        icdist = (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
        dx = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x)
        dy = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y
        with np.errstate(all="ignore"):
            qx = np.float32(x * icdist + dx - x0)          # Point2f proofdist
            qy = np.float32(y * icdist + dy - y0)
            d = np.sqrt(np.float32(np.float32(qx * qx) + np.float32(qy * qy)))    # float32 products, sum and root
        mask.append(not (float(d) > 0.25))                 # a NaN passes, as in the reference
        if RR is not None:
            xx = RR[0] * x + RR[1] * y + RR[2]
            yy = RR[3] * x + RR[4] * y + RR[5]
            ww = 1.0 / (RR[6] * x + RR[7] * y + RR[8])
            x = xx * ww
            y = yy * ww
        with np.errstate(all="ignore"):
            out.append((f32(x), f32(y)))
    return out, mask


def coeffs8(dist):
    d = [float(v) for v in (dist if dist is not None else [])]
    assert len(d) in (0, 4, 5, 8)
    return d + [0.0] * (8 - len(d))


def corner_points(A, k, nx, ny):
    """rectifyFusiello :1703-1744: the four image corners, undistorted IN PLACE inside the loop (a valid point goes back to its saved
    pixel position, an invalid one moves inwards), with the coefficient-free pass once the reduction reaches 0.25 -> (points, steps)"""
    pts = [(f32((i % 2) * (nx - 1.0)), f32((1 if i >= 2 else 0) * (ny - 1.0))) for i in range(4)]
    sv = list(pts)
    reduction = 0.01
    steps = 0
    cx, cy = nx / 2.0, ny / 2.0
    while True:
        pts, mask = undistort_points(pts, A, k, None)
        valid = sum(mask)
        if valid < 4:
            for i in range(4):
                j = 1 if i >= 2 else 0
                if not mask[i]:
                    px = f32(math.floor((1.0 - reduction) * ((i % 2) * nx - cx)) + cx - 1.0)
                    py = f32(math.floor((1.0 - reduction) * (j * ny - cy)) + cy - 1.0)
                    sv[i] = pts[i] = (px, py)
                else:
                    pts[i] = sv[i]
            reduction = reduction + 0.01
            steps += 1
        if not (valid < 4 and reduction < 0.25):
            break
    if reduction >= 0.25:
        pts, _ = undistort_points(pts, A, None, None)
    return pts, steps


def rectangles(A, k, Rk, pp, w, h):
    """icvGetRectanglesV0 on the 9 x 9 grid -> (inner, outer) as float32 (x, y, width, height), steps"""
    N = 9
    RR = mul3(pp, Rk)
    grid = [(f32(f32(float(x) * w) / (N - 1)), f32(f32(float(y) * h) / (N - 1))) for y in range(N) for x in range(N)]
    pts = list(grid)
    sv = list(grid)
    reduction = np.float32(0.01)
    steps = 0
    cx, cy = f32(float(w) / 2.0), f32(float(h) / 2.0)
    while True:
        pts, mask = undistort_points(pts, A, k, RR)
        valid = sum(mask)
        if valid < N * N:
            red = 1.0 - float(reduction)
            for i in range(N * N):
                if not mask[i]:
                    sv[i] = pts[i] = (f32(red * f32(grid[i][0] - cx) + cx), f32(red * f32(grid[i][1] - cy) + cy))
                else:
                    pts[i] = sv[i]
            reduction = np.float32(reduction + np.float32(0.01))
            steps += 1
        if not (valid < N * N and float(reduction) < 0.25):
            break
    if float(reduction) >= 0.25:
        pts, _ = undistort_points(pts, A, None, RR)
    fmax = float(np.finfo(np.float32).max)
    iX0, iX1, iY0, iY1 = -fmax, fmax, -fmax, fmax
    oX0, oX1, oY0, oY1 = fmax, -fmax, fmax, -fmax
    for y in range(N):
        for x in range(N):
            px, py = pts[y * N + x]
            oX0 = px if px < oX0 else oX0        # std::min / std::max: the left argument stays on a NaN
            oX1 = px if oX1 < px else oX1
            oY0 = py if py < oY0 else oY0
            oY1 = py if oY1 < py else oY1
            if x == 0:
                iX0 = px if iX0 < px else iX0
            if x == N - 1:
                iX1 = px if px < iX1 else iX1
            if y == 0:
                iY0 = py if iY0 < py else iY0
            if y == N - 1:
                iY1 = py if py < iY1 else iY1
    with np.errstate(all="ignore"):
        inner = (iX0, iY0, f32(iX1 - iX0), f32(iY1 - iY0))
        outer = (oX0, oY0, f32(oX1 - oX0), f32(oY1 - oY0))
    return inner, outer, steps


def _sat_int(x):
    """(int) of a double that went through ceil / floor, with the library's rule: NaN -> 0, saturating"""
    if x != x:
        return 0
    return int(max(-2147483648.0, min(2147483647.0, x)))


def roi_arguments(inner, cx0, cy0, s, cx1, cy1):
    """the four doubles under ceil / floor at :1819-1822"""
    return ((inner[0] - cx0) * s + cx1, (inner[1] - cy0) * s + cy1, inner[2] * s, inner[3] * s)


def parameters(R, t, K1, K2, dist1, dist2, size, alpha=-1.0, new_size=(0, 0), inverse="cof"):
    inv3 = inv3_cof if inverse == "cof" else inv3_lu
    R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    t = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
    K1 = [float(v) for v in np.asarray(K1, np.float64).reshape(9)]
    K2 = [float(v) for v in np.asarray(K2, np.float64).reshape(9)]
    k1 = coeffs8(dist1)
    k2 = coeffs8(dist2)
    n1 = 0 if dist1 is None else len(dist1)
    n2 = 0 if dist2 is None else len(dist2)
    w, h = int(size[0]), int(size[1])
    nw, nh = int(new_size[0]), int(new_size[1])
    if nw * nh == 0:
        nw, nh = w, h
    nx, ny = float(w), float(h)
    # ---- t normalised (:1394-1397)
    tn = t[0] * t[0]
    tn = tn + t[1] * t[1]
    tn = tn + t[2] * t[2]
    tn = math.sqrt(tn)
    if abs(tn - 1.0) > 1e-4:
        t = [t[0] / tn, t[1] / tn, t[2] / tn]
    # ---- focal length and first principal point (:1521-1544)
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    fc_new = float("inf")
    for (A, k, n) in ((K1, k1, n1), (K2, k2, n2)):
        dk1 = k[0] if n else 0.0
        fc = A[4 * (idx ^ 1)]
        if dk1 < 0:
            fc = fc * (1.0 + dk1 * (nx * nx + ny * ny) / (4.0 * fc * fc))
        fc_new = fc if fc < fc_new else fc_new
    ccx = (nx - 1.0) / 2.0
    ccy = (ny - 1.0) / 2.0
    ccx = float(nw) * ccx / float(w)
    ccy = float(nh) * ccy / float(h)
    Knew = [fc_new, 0.0, ccx, 0.0, fc_new, ccy, 0.0, 0.0, 1.0]
    # ---- optical centres: c1 = 0, c2 = -(R^T (K2^-1 (K2 t))) (:1549-1550)
    K2inv = inv3(K2)
    a = mulv3(K2inv, mulv3(K2, t))
    Rt = [R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]]
    c2 = mulv3(Rt, a)
    c2 = [-c2[0], -c2[1], -c2[2]]
    # ---- new axes (:1556-1569)
    v1 = c2
    v2 = [-v1[1], v1[0], 0.0]
    v3 = [v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]]
    Rv = []
    for v in (v1, v2, v3):
        n = v[0] * v[0]
        n = n + v[1] * v[1]
        n = n + v[2] * v[2]
        n = math.sqrt(n)
        Rv += [v[0] / n, v[1] / n, v[2] / n]
    # ---- first pass with K2 (skew 0) as the new matrix: the shift that centres the images (:1572-1610)
    Kn = list(K2)
    Kn[1] = 0.0
    Po1i = inv3(K1)
    Po2i = inv3(mul3(K2, R))
    KR = mul3(Kn, Rv)
    Ra = mul3(KR, Po1i)
    Rb = mul3(KR, Po2i)
    imc = [(nx - 1.0) / 2.0, (ny - 1.0) / 2.0, 1.0]
    pa = mulv3(Ra, imc)
    pb = mulv3(Rb, imc)
    d1x = imc[0] - pa[0] / pa[2]
    d1y = imc[1] - pa[1] / pa[2]
    d2x = imc[0] - pb[0] / pb[2]
    d2y = imc[1] - pb[1] / pb[2]
    Knew[2] = Knew[2] + (d1x + d2x) / 2.0
    Knew[5] = Knew[5] + (d1y + d2y) / 2.0
    # ---- second pass with Knew, then into 3-D space (:1615-1680)
    KR = mul3(Knew, Rv)
    Ra = mul3(KR, Po1i)
    Rb = mul3(KR, Po2i)
    Kni = inv3(Knew)
    Rect1 = mul3(Kni, mul3(Ra, K1))
    Rect2 = mul3(Kni, mul3(Rb, K2))
    # ---- principal point from the undistorted corners (:1692-1780)
    steps = [0, 0, 0, 0]
    cc = []
    for kk, (A, k, n, Rk) in enumerate(((K1, k1, n1, Rect1), (K2, k2, n2, Rect2))):
        pts, steps[kk] = corner_points(A, k if n else [0.0] * 8, nx, ny)
        sx = sy = None
        for (px, py) in pts:                                 # cv::projectPoints, the matrix used directly, t = 0, no distortion
            X = Rk[0] * px + Rk[1] * py + Rk[2]
            Y = Rk[3] * px + Rk[4] * py + Rk[5]
            Z = Rk[6] * px + Rk[7] * py + Rk[8]
            Z = 1.0 / Z if Z != 0 else 1.0
            u = (X * Z) * fc_new
            v = (Y * Z) * fc_new
            sx = u if sx is None else sx + u
            sy = v if sy is None else sy + v
        cc.append(((nx - 1.0) / 2.0 - sx / 4.0, (ny - 1.0) / 2.0 - sy / 4.0))
    cx0 = (cc[0][0] + cc[1][0]) * 0.5
    cy0 = (cc[0][1] + cc[1][1]) * 0.5
    pp = [fc_new, 0.0, cx0, 0.0, fc_new, cy0, 0.0, 0.0, 1.0]
    alpha = min(float(alpha), 1.0)
    inner1, outer1, steps[2] = rectangles(K1, k1 if n1 else [0.0] * 8, Rect1, pp, w, h)
    inner2, outer2, steps[3] = rectangles(K2, k2 if n2 else [0.0] * 8, Rect2, pp, w, h)
    cx1 = float(nw) * cx0 / float(w)
    cy1 = float(nh) * cy0 / float(h)
    s = 1.0
    s0 = s1 = 0.0
    if alpha >= 0:
        with np.errstate(all="ignore"):
            def div(a, b):
                return float(np.float64(a) / np.float64(b))
            s0 = max(max(max(div(cx1, cx0 - inner1[0]), div(cy1, cy0 - inner1[1])), div(nw - cx1, f32(inner1[0] + inner1[2]) - cx0)),
                     div(nh - cy1, f32(inner1[1] + inner1[3]) - cy0))
            s1 = min(min(min(div(cx1, cx0 - outer1[0]), div(cy1, cy0 - outer1[1])), div(nw - cx1, f32(outer1[0] + outer1[2]) - cx0)),
                     div(nh - cy1, f32(outer1[1] + outer1[3]) - cy0))
        s = s0 * (1.0 - alpha) + s1 * alpha
        if s > 2.0 or s < 0.5:
            s = 1.0
    info = [fc_new, s0, s1, s] + [float(v) for v in steps]
    fc_s = fc_new * s
    Kout = [fc_s, 0.0, cx1, 0.0, fc_s, cy1, 0.0, 0.0, 1.0]
    args = roi_arguments(inner1, cx0, cy0, s, cx1, cy1)
    up = [a if not math.isfinite(a) else float(math.ceil(a)) for a in args[:2]]
    down = [a if not math.isfinite(a) else float(math.floor(a)) for a in args[2:]]
    rx, ry, rw, rh = _sat_int(up[0]), _sat_int(up[1]), _sat_int(down[0]), _sat_int(down[1])
    x1, y1 = max(rx, 0), max(ry, 0)                          # cv::Rect & cv::Rect(0, 0, nw, nh), sums in 64 bits
    ww, hh = min(rx + rw, nw) - x1, min(ry + rh, nh) - y1
    roi = [x1, y1, ww, hh] if ww > 0 and hh > 0 else [0, 0, 0, 0]
    P = []
    for c in ([0.0, 0.0, 0.0], c2):
        tc = mulv3(Rv, c)
        Pt = [Rv[0], Rv[1], Rv[2], -tc[0], Rv[3], Rv[4], Rv[5], -tc[1], Rv[6], Rv[7], Rv[8], -tc[2]]
        Pm = [0.0] * 12
        for i in range(3):
            for j in range(4):
                q = Kout[3 * i] * Pt[j]
                q = q + Kout[3 * i + 1] * Pt[4 + j]
                q = q + Kout[3 * i + 2] * Pt[8 + j]
                Pm[4 * i + j] = q
        P.append(np.array(Pm).reshape(3, 4))
    return dict(Rect1=np.array(Rect1).reshape(3, 3), Rect2=np.array(Rect2).reshape(3, 3), Knew=np.array(Kout).reshape(3, 3), roi=roi,
                P1=P[0], P2=P[1], info=np.array(info), roi_args=args, inner=inner1, outer=outer1, inner2=inner2, outer2=outer2,
                cx0=cx0, cy0=cy0)


# ---------------------------------------------------------------------------------------------------------------- maps
def map_matrix(K, dist, Rect, Knew):
    """what the host hands the kernel: ir = (Knew Rect)^-1 by cofactors, the eight coefficients, fx, fy, cx, cy"""
    K = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
    A = mul3([float(v) for v in np.asarray(Knew, np.float64).reshape(9)], [float(v) for v in np.asarray(Rect, np.float64).reshape(9)])
    return inv3_cof(A), coeffs8(dist), (K[0], K[4], K[2], K[5])


def map_formula(u, v, ir, k, f, xp=np.float64):
    """the per-pixel formula on arrays of type xp (float64: the restatement; longdouble: its yardstick); one operation per line"""
    ir = [xp(q) for q in ir]
    k1, k2, p1, p2, k3, k4, k5, k6 = [xp(q) for q in k]
    fx, fy, cx, cy = [xp(q) for q in f]
    one, two = xp(1.0), xp(2.0)
    with np.errstate(all="ignore"):
        _x = v * ir[1]
        _x = _x + ir[2]
        _x = u * ir[0] + _x
        _y = v * ir[4]
        _y = _y + ir[5]
        _y = u * ir[3] + _y
        _w = v * ir[7]
        _w = _w + ir[8]
        _w = u * ir[6] + _w
        x = _x / _w
        y = _y / _w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = (two * x) * y
        num = k3 * r2
        num = num + k2
        num = num * r2
        num = num + k1
        num = num * r2
        num = one + num
        den = k6 * r2
        den = den + k5
        den = den * r2
        den = den + k4
        den = den * r2
        den = one + den
        kr = num / den
        xd = x * kr
        xd = xd + p1 * _2xy
        xd = xd + p2 * (r2 + two * x2)
        yd = y * kr
        yd = yd + p1 * (r2 + two * y2)
        yd = yd + p2 * _2xy
        mx = fx * xd + cx
        my = fy * yd + cy
    return mx, my


def maps(K, dist, Rect, Knew, width, height):
    ir, k, f = map_matrix(K, dist, Rect, Knew)
    u = np.arange(width, dtype=np.float64)[None, :].repeat(height, 0)
    v = np.arange(height, dtype=np.float64)[:, None].repeat(width, 1)
    mx, my = map_formula(u, v, ir, k, f)
    with np.errstate(all="ignore"):
        return mx.astype(np.float32), my.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- remap
def remap(img, mapx, mapy):
    """OpenCV's fixed-point bilinear remap of an 8-bit image, BORDER_CONSTANT 0"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    mapx = np.asarray(mapx, np.float32)
    mapy = np.asarray(mapy, np.float32)
    with np.errstate(all="ignore"):
        ax = mapx * np.float32(32.0)                         # float32 product
        ay = mapy * np.float32(32.0)
        lo, hi = np.float32(-2147483648.0), np.float32(2147483648.0)
        ok = (ax >= lo) & (ax < hi) & (ay >= lo) & (ay < hi)     # false for a NaN
        sx = np.where(ok, np.rint(ax), np.float32(0)).astype(np.int64)    # round half even
        sy = np.where(ok, np.rint(ay), np.float32(0)).astype(np.int64)
    ix = np.clip(sx >> 5, -32768, 32767)
    iy = np.clip(sy >> 5, -32768, 32767)
    fx = sx & 31
    fy = sy & 31
    acc = np.zeros(mapx.shape, np.int64)
    for (dx, dy, wt) in ((0, 0, (32 - fx) * (32 - fy) * 32), (1, 0, fx * (32 - fy) * 32), (0, 1, (32 - fx) * fy * 32), (1, 1, fx * fy * 32)):
        x = ix + dx
        y = iy + dy
        inside = ok & (x >= 0) & (x < w) & (y >= 0) & (y < h)
        p = img[np.where(inside, y, 0), np.where(inside, x, 0)].astype(np.int64)
        acc += np.where(inside, wt * p, 0)
    return ((acc + 16384) >> 15).astype(np.uint8)
