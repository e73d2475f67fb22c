"""Seeded synthetic workloads for the BASELINE.json configs; numpy only."""
from __future__ import annotations

import numpy as np


def orb_pair(nq: int, nt: int, nbytes: int = 32, seed: int = 20260102, match_frac: float = 0.5, flip_p: float = 0.08):
    """Binary descriptor sets: `match_frac` of the queries are a train row with Binomial(bits, flip_p) bits
    flipped (true matches), the rest are i.i.d. uniform bytes.  C1: (2048,2048,seed 20260101); C2: (8192,8192,
    seed 20260102)."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, size=(nt, nbytes), dtype=np.uint8)
    q = rng.integers(0, 256, size=(nq, nbytes), dtype=np.uint8)
    n_match = int(nq * match_frac)
    which = rng.permutation(nq)[:n_match]
    src = rng.integers(0, nt, size=n_match)
    flips = rng.random((n_match, nbytes * 8)) < flip_p
    flip_bytes = np.packbits(flips, axis=1, bitorder="little")
    q[which] = t[src] ^ flip_bytes
    return q, t


def sift_pair(nq: int, nt: int, dim: int = 128, seed: int = 20260104, match_frac: float = 0.5):
    """Integer-valued 0..255 float32 descriptors in OpenCV-SIFT layout (L2-normalised to 512, clipped at 255,
    rounded); half of the queries are perturbed train rows.  C4: (4096,4096,128)."""
    rng = np.random.default_rng(seed)

    def make(n):
        x = rng.gamma(0.6, 1.0, size=(n, dim))
        x = x / np.linalg.norm(x, axis=1, keepdims=True) * 512.0
        return np.clip(np.rint(x), 0, 255)

    t = make(nt)
    q = make(nq)
    n_match = int(nq * match_frac)
    which = rng.permutation(nq)[:n_match]
    src = rng.integers(0, nt, size=n_match)
    q[which] = np.clip(np.rint(t[src] + rng.normal(0, 6.0, size=(n_match, dim))), 0, 255)
    return q.astype(np.float32), t.astype(np.float32)


def _rot(axis, deg):
    axis = np.asarray(axis, float)
    axis = axis / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


PIX_TO_CAM = 4.0 / (np.sqrt(2.0) * 3200.0)  # f = 800 on both cameras (stereo_pose_refinement.h:280-286)


def pose_scene(n: int = 5000, inlier_frac: float = 0.5, seed: int = 20260103, noise_px: float = 0.3, rot_deg: float = 5.0,
               t_len: float = 1.0):
    """C3 scene: camera-normalised correspondences with known (R, t).

    3-D points uniform in x,y in [-2,2], z in [4,12]; R = rot((0.2,0.9,0.1), 5 deg), t = (1,0.05,-0.02)/|.|;
    Gaussian noise sigma = noise_px * PIX_TO_CAM on both views; outliers = uniform points in the same image box
    paired at random; order shuffled.  Returns p1, p2 (n x 2 float64), R, t, inlier_mask, thresh (0.8 px).
    `rot_deg` / `t_len` (baseline length; the scene is 4..12 deep) make the degenerate motions USAC tests for: t_len = 0 is a pure
    rotation, rot_deg = 0 and t_len = 0 no motion at all."""
    rng = np.random.default_rng(seed)
    R = _rot((0.2, 0.9, 0.1), rot_deg)
    t = np.array([1.0, 0.05, -0.02])
    t = t / np.linalg.norm(t)
    n_in = int(round(n * inlier_frac))
    X = np.stack([rng.uniform(-2, 2, n_in), rng.uniform(-2, 2, n_in), rng.uniform(4, 12, n_in)], axis=1)
    x1 = X[:, :2] / X[:, 2:3]
    X2 = X @ R.T + t_len * t
    x2 = X2[:, :2] / X2[:, 2:3]
    sigma = noise_px * PIX_TO_CAM
    x1 = x1 + rng.normal(0, sigma, x1.shape)
    x2 = x2 + rng.normal(0, sigma, x2.shape)
    n_out = n - n_in
    lo1, hi1 = x1.min(0), x1.max(0)
    lo2, hi2 = x2.min(0), x2.max(0)
    o1 = rng.uniform(lo1, hi1, (n_out, 2))
    o2 = rng.uniform(lo2, hi2, (n_out, 2))
    p1 = np.concatenate([x1, o1])
    p2 = np.concatenate([x2, o2])
    mask = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(n)
    return (np.ascontiguousarray(p1[perm]), np.ascontiguousarray(p2[perm]), R, t, mask[perm], 0.8 * PIX_TO_CAM)


def stereo_pair(n: int = 2000, seed: int = 20260200, inlier_frac: float = 0.5, f: float = 800.0, cx: float = 320.0,
                cy: float = 240.0, nbytes: int = 32, flip_p: float = 0.04, unmatched_frac: float = 0.0):
    """One synthetic image pair for the whole pipeline (C5 unit): keypoints in pixels (float32), binary descriptors whose
    nearest neighbours are the true correspondences (train side shuffled), and the ground-truth pose.
    Returns dict(desc1, desc2, kp1, kp2, K, R, t, train_of_query)."""
    p1, p2, R, t, mask, th = pose_scene(n, inlier_frac=inlier_frac, seed=seed)
    rng = np.random.default_rng(seed + 7)
    perm = rng.permutation(n)                      # train row perm[i] belongs to query i
    kp1 = (p1 * f + np.array([cx, cy])).astype(np.float32)
    kp2_q = (p2 * f + np.array([cx, cy])).astype(np.float32)
    kp2 = np.empty_like(kp2_q)
    kp2[perm] = kp2_q
    d2 = rng.integers(0, 256, size=(n, nbytes), dtype=np.uint8)
    flips = np.packbits(rng.random((n, nbytes * 8)) < flip_p, axis=1, bitorder="little")
    d1 = d2[perm] ^ flips
    if unmatched_frac > 0:  # queries without a true neighbour: they fail the ratio test, so the match count varies with the seed
        lost = rng.random(n) < unmatched_frac
        d1[lost] = rng.integers(0, 256, size=(int(lost.sum()), nbytes), dtype=np.uint8)
    K = np.array([f, f, cx, cy], np.float64)
    return dict(desc1=d1, desc2=d2, kp1=kp1, kp2=kp2, K=K, R=R, t=t, train_of_query=perm.astype(np.int32))


def _sift_rows(rng, n: int, dim: int):
    """sift_pair's make(): gamma-distributed rows, L2-normalised to 512, clipped at 255, rounded."""
    x = rng.gamma(0.6, 1.0, size=(n, dim))
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * 512.0
    return np.clip(np.rint(x), 0, 255)


def stereo_pair_f32(n: int = 2000, seed: int = 20260400, dim: int = 128, sigma: float = 6.0, unmatched_frac: float = 0.0,
                    rootsift: bool = False, f: float = 800.0, cx: float = 320.0, cy: float = 240.0):
    """stereo_pair with float descriptors (the C5 unit for SIFT-like data): pose_scene geometry, keypoints in pixels, train side
    shuffled; desc2 = sift_pair's rows (integer-valued 0..255, OpenCV-SIFT layout), desc1 = clip(rint(desc2[perm] + N(0, sigma))), so
    the nearest neighbours are the true correspondences; `unmatched_frac` of the queries are fresh rows without a true neighbour (they
    fail the ratio test).  rootsift: both sides become sqrt(x / sum(x)) (RootSIFT) -- non-integer data, which the exact and the fp16
    L2 paths serve instead of the int8 one.  Returns the same dict keys as stereo_pair, descriptors float32."""
    p1, p2, R, t, mask, th = pose_scene(n, inlier_frac=0.5, seed=seed)
    rng = np.random.default_rng(seed + 7)
    perm = rng.permutation(n)                      # train row perm[i] belongs to query i
    kp1 = (p1 * f + np.array([cx, cy])).astype(np.float32)
    kp2_q = (p2 * f + np.array([cx, cy])).astype(np.float32)
    kp2 = np.empty_like(kp2_q)
    kp2[perm] = kp2_q
    d2 = _sift_rows(rng, n, dim)
    d1 = np.clip(np.rint(d2[perm] + rng.normal(0, sigma, size=(n, dim))), 0, 255)
    if unmatched_frac > 0:
        lost = rng.random(n) < unmatched_frac
        d1[lost] = _sift_rows(rng, int(lost.sum()), dim)
    if rootsift:
        d1 = np.sqrt(d1 / np.maximum(d1.sum(axis=1, keepdims=True), 1e-12))
        d2 = np.sqrt(d2 / np.maximum(d2.sum(axis=1, keepdims=True), 1e-12))
    K = np.array([f, f, cx, cy], np.float64)
    return dict(desc1=np.ascontiguousarray(d1, np.float32), desc2=np.ascontiguousarray(d2, np.float32), kp1=kp1, kp2=kp2, K=K, R=R, t=t,
                train_of_query=perm.astype(np.int32))


def vfc_scene(kind: str, n: int, seed: int = 0, width: float = 1280.0, height: float = 720.0):
    """Matched points for the VFC match filter (matchinglib::filterWithVFC): x1 uniform over a width x height image, x2 = H(x1) under a
    mild homography (2 degrees of rotation, 3 % of scale, a shift, a little perspective).
    kind "clean":  0.7 px of Gaussian noise on x2, and 20-50 % of the matches (the fraction is drawn per scene) replaced by uniform
                   outliers -- separable data: the inlier posterior is bimodal.
    kind "graded": no outliers, but a per-match noise sigma that is log-uniform in [0.5, 120] px -- a continuum between inlier and
                   outlier, on which the posterior comes arbitrarily close to the filter's threshold.
    Returns dict(x1, x2: float32 [n, 2], inlier: bool [n] ("clean": not replaced; "graded": sigma < 3 px), sigma [n])."""
    if kind not in ("clean", "graded"):
        raise ValueError("kind is 'clean' or 'graded'")
    rng = np.random.default_rng(20261719 + 7919 * seed + (0 if kind == "clean" else 1))
    x1 = rng.random((n, 2)) * np.array([width, height])
    a = np.deg2rad(2.0)
    H = np.array([[1.03 * np.cos(a), -1.03 * np.sin(a), 24.0], [1.03 * np.sin(a), 1.03 * np.cos(a), -15.0], [2e-5, -1e-5, 1.0]])
    h = np.concatenate([x1, np.ones((n, 1))], axis=1) @ H.T
    x2 = h[:, :2] / h[:, 2:3]
    if kind == "clean":
        sigma = np.full(n, 0.7)
        x2 = x2 + rng.normal(0.0, 1.0, (n, 2)) * 0.7
        frac = rng.uniform(0.2, 0.5)
        out = np.zeros(n, bool)
        out[rng.permutation(n)[: int(round(frac * n))]] = True
        x2[out] = rng.random((int(out.sum()), 2)) * np.array([width, height])
        inlier = ~out
    else:
        sigma = np.exp(rng.uniform(np.log(0.5), np.log(120.0), n))
        x2 = x2 + rng.normal(0.0, 1.0, (n, 2)) * sigma[:, None]
        inlier = sigma < 3.0
    return dict(x1=np.ascontiguousarray(x1, np.float32), x2=np.ascontiguousarray(x2, np.float32), inlier=inlier, sigma=sigma)


def gms_scene(kind: str, n: int, seed: int = 0, width: int = 1280, height: int = 720):
    """Keypoints and matches for the GMS match filter (matchinglib::filterMatchesGMS).  Both images are width x height.
    kind "smooth": a smooth motion field (3 % of shrink, a shift, a slow sine) with 1 px of noise; a quarter of the matches random.
    kind "rot90":  the same with the field rotated by 90 degrees about the image centre (in normalised coordinates, so that the 20 x 20
                   grid maps onto itself): the filter finds it with the rotation switch only, at rotation type 6.
    kind "scale2": the first image's points lie in its central half and the second image's content is scaled by 2 about the centre: the
                   filter finds it on the 10 x 10 right grid (scale level 1).
    kind "sparse": the smooth field with 70 % random matches -- few consistent matches per cell.
    Match i joins keypoint i of the first image and keypoint perm[i] of the second.
    Returns dict(kp1, kp2: float32 [n, 2], matches: DMatch rows [n], size1, size2: (width, height), inlier: bool [n])."""
    if kind not in ("smooth", "rot90", "scale2", "sparse"):
        raise ValueError("kind is 'smooth', 'rot90', 'scale2' or 'sparse'")
    rng = np.random.default_rng(20261811 + 104729 * seed + {"smooth": 0, "rot90": 1, "scale2": 2, "sparse": 3}[kind])
    wh = np.array([width, height], np.float64)
    u = rng.random((n, 2))
    if kind == "scale2":
        u = 0.25 + 0.5 * u
        v = 0.5 + 2.0 * (u - 0.5)
    else:
        v = 0.015 + 0.97 * u + 0.01 * np.sin(3.0 * u[:, ::-1])
        if kind == "rot90":
            v = np.stack([1.0 - v[:, 1], v[:, 0]], axis=1)
    x1 = u * wh
    x2 = v * wh + rng.normal(0.0, 1.0, (n, 2))
    out = np.zeros(n, bool)
    out[rng.permutation(n)[: int(round((0.7 if kind == "sparse" else 0.25) * n))]] = True
    x2[out] = rng.random((int(out.sum()), 2)) * wh
    x2 = np.clip(x2, 0.0, wh - 0.01)
    perm = rng.permutation(n)
    kp2 = np.empty((n, 2), np.float32)
    kp2[perm] = x2.astype(np.float32)
    matches = np.zeros(n, np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")]))
    matches["queryIdx"], matches["trainIdx"] = np.arange(n), perm
    matches["distance"] = rng.integers(0, 64, n).astype(np.float32)
    return dict(kp1=np.ascontiguousarray(x1, np.float32), kp2=kp2, matches=matches, size1=(width, height), size2=(width, height), inlier=~out)


def _smooth_texture(rng, terms: int = 24):
    """a smooth random function of the plane with values in about [0, 255]: a sum of sinusoids of 10 to 48 pixels wavelength"""
    wl = rng.uniform(10.0, 48.0, terms)
    ang = rng.uniform(0.0, 2.0 * np.pi, terms)
    ph = rng.uniform(0.0, 2.0 * np.pi, terms)
    amp = rng.uniform(0.5, 1.0, terms)
    kx, ky = 2.0 * np.pi / wl * np.cos(ang), 2.0 * np.pi / wl * np.sin(ang)

    def f(x, y):
        v = sum(a * np.sin(p + cx * x + cy * y) for a, p, cx, cy in zip(amp, ph, kx, ky))
        return 127.5 + v * (110.0 / np.sqrt(0.5 * np.sum(amp * amp)) / 3.0)

    return f


def subpix_scene(kind: str, n: int, seed: int = 0, width: int = 320, height: int = 240, shift=(3.3, -2.6), noise: float = 0.0,
                 scramble: float = 0.0, side: float = 0.0):
    """Images, keypoints and keypoint sizes for the sub-pixel refinement (matchinglib::getSubPixMatches); lists 1 and 2 match index by index.
    kind "texture":  a smooth texture; image 2 shows it moved by `shift` pixels (sampled from the continuous function, so the shift is exact),
                     both images with Gaussian noise of `noise` grey levels.  Keypoint 1 is uniform over the image, keypoint 2 = keypoint 1 +
                     shift + up to 1.5 px of jitter.  A share `scramble` of the keypoints 2 is moved 6 to 8 px further, which puts the true
                     position outside the search window: outliers.  `truth` = cvRound(keypoint 1) + shift, what the refinement should return.
    kind "constant": both images hold one grey level and the keypoints stay 24 px from the edges: all 121 sums are 0.
    kind "rounding": 200 x 200 images.  Image 1 holds a block of 96 x 96 pixels of 255 that every template contains whole, image 2 holds 0
                     wherever a placement can put that block, so all 121 sums share 96^2 * 255^2 > 2^29, where float32 steps by 64; the other
                     pixels are grey levels 0 to 3 (image 1: nine in ten of them 0), so the sums differ by the few pixels of image 2's
                     border that a placement covers: least, and nearly equal, around the centre.  Keypoints within 1.4 px of the centre, size 111.1 (side 117) unless `side`
                     says otherwise (at least 107).
    Returns dict(img1, img2: uint8 [height, width], kp1, kp2: float32 [n, 2], size1, size2: float32 [n], truth: float32 [n, 2],
    scrambled: bool [n])."""
    if kind not in ("texture", "constant", "rounding"):
        raise ValueError("kind is 'texture', 'constant' or 'rounding'")
    rng = np.random.default_rng(20261019 + 15485863 * seed + {"texture": 0, "constant": 1, "rounding": 2}[kind])
    scr = np.zeros(n, bool)
    if kind == "rounding":
        width = height = 200
        lo, hi = 100 - 48, 100 + 48
        img1 = (rng.integers(1, 4, (height, width)) * (rng.random((height, width)) < 0.1)).astype(np.uint8)
        img2 = rng.integers(0, 4, (height, width)).astype(np.uint8)
        img1[lo:hi, lo:hi] = 255
        img2[lo - 9:hi + 9, lo - 9:hi + 9] = 0
        kp1 = 100.0 + rng.integers(-1, 2, (n, 2)) + rng.uniform(-0.4, 0.4, (n, 2))
        kp2 = 100.0 + rng.integers(-1, 2, (n, 2)) + rng.uniform(-0.4, 0.4, (n, 2))
        sizes = np.full(n, side if side else 111.1, np.float32)
        truth = kp2.copy()
    else:
        if kind == "constant":
            img1 = np.full((height, width), 93, np.uint8)
            img2 = img1.copy()
        else:
            f = _smooth_texture(rng)
            yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
            a, b = f(xx, yy), f(xx - shift[0], yy - shift[1])
            if noise > 0.0:
                a, b = a + rng.normal(0.0, noise, a.shape), b + rng.normal(0.0, noise, b.shape)
            img1, img2 = np.clip(np.rint(a), 0, 255).astype(np.uint8), np.clip(np.rint(b), 0, 255).astype(np.uint8)
        kp1 = rng.random((n, 2)) * np.array([width - 1.0, height - 1.0])
        if kind == "constant":
            kp1 = 24.0 + rng.random((n, 2)) * np.array([width - 49.0, height - 49.0])   # templates and windows whole inside the images
        truth = np.rint(kp1.astype(np.float32)) + np.array(shift)
        kp2 = kp1 + np.array(shift) + rng.uniform(-1.5, 1.5, (n, 2))
        scr[rng.permutation(n)[: int(round(scramble * n))]] = True
        ang = rng.uniform(0.0, 2.0 * np.pi, n)
        far = rng.uniform(6.0, 8.0, n)[:, None] * np.stack([np.sign(np.cos(ang)), np.sign(np.sin(ang))], axis=1)
        kp2[scr] += far[scr]
        sizes = np.full(n, side, np.float32)
    return dict(img1=np.ascontiguousarray(img1), img2=np.ascontiguousarray(img2), kp1=np.ascontiguousarray(kp1, np.float32),
                kp2=np.ascontiguousarray(kp2, np.float32), size1=sizes.copy(), size2=sizes.copy(), truth=np.ascontiguousarray(truth, np.float32),
                scrambled=scr)


def corner_scene(width: int = 320, height: int = 240, cell: float = 24.0, angle: float = 0.12, origin=(5.3, 7.7), low: int = 40, high: int = 210,
                 supersample: int = 8, margin: float = 14.0):
    """An anti-aliased checkerboard with known sub-pixel corner positions, for the corner refinement (matchinglib::getSubPixMatches_seperate_Imgs).
    The board has square cells of `cell` pixels and grey levels `low` / `high`, is rotated by `angle` radians and has a corner at `origin`;
    pixel (x, y) is the mean of supersample^2 samples of the board over the unit square centred on (x, y).  Returns dict(img: uint8
    [height, width], corners: float32 [m, 2] (x, y), row by row of the board: the cell corners at least `margin` pixels inside the image)."""
    c, s = np.cos(angle), np.sin(angle)
    sub = (np.arange(supersample) + 0.5) / supersample - 0.5
    ys = (np.arange(height)[:, None] + sub[None, :]).reshape(-1)
    xs = (np.arange(width)[:, None] + sub[None, :]).reshape(-1)
    X, Y = xs[None, :] - origin[0], ys[:, None] - origin[1]
    u, v = c * X + s * Y, -s * X + c * Y
    odd = (np.floor(u / cell) + np.floor(v / cell)).astype(np.int64) & 1
    fine = np.where(odd == 1, float(high), float(low))
    img = fine.reshape(height, supersample, width, supersample).mean(axis=(1, 3))
    reach = int(np.ceil((width + height) / cell)) + 2
    k = np.arange(-reach, reach + 1) * cell
    bu, bv = np.meshgrid(k, k)                                   # rows of the board: v fixed, u running
    cx, cy = origin[0] + c * bu - s * bv, origin[1] + s * bu + c * bv
    keep = (cx >= margin) & (cx <= width - 1 - margin) & (cy >= margin) & (cy <= height - 1 - margin)
    corners = np.stack([cx[keep], cy[keep]], axis=1)
    return dict(img=np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8)), corners=np.ascontiguousarray(corners, np.float32))
