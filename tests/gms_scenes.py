"""Crafted scenes for the GMS filter tests (test_oracle_gms.py checks on the CPU that each has the property it was built for;
test_gpu_gms.py runs them on the device).  All images are 1280 x 720: a left cell is 64 x 36 pixels.  A scene is
dict(kp1, kp2: float32 [n, 2], matches: DMatch rows, size1, size2), match i joining keypoint i of both images."""
import numpy as np

import gms_oracle as G

W, H = 1280, 720
CW, CH = W / 20.0, H / 20.0
DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


def scene(p1, p2):
    p1, p2 = np.asarray(p1, np.float32).reshape(-1, 2), np.asarray(p2, np.float32).reshape(-1, 2)
    m = np.zeros(len(p1), DMATCH)
    m["queryIdx"] = m["trainIdx"] = np.arange(len(p1))
    return dict(kp1=np.ascontiguousarray(p1), kp2=np.ascontiguousarray(p2), matches=m, size1=(W, H), size2=(W, H))


def oracle(s, use_scale=False, use_rotation=False, **kw):
    return G.gms_oracle(s["kp1"], s["size1"], s["kp2"], s["size2"], s["matches"], use_scale, use_rotation, **kw)


def cell_points(cx, cy, k, ox=0.25, oy=0.25):
    """k points inside cell (cx, cy), a quarter cell from its corner (so that no half-cell shift moves them to another cell)"""
    return [((cx + ox) * CW + 0.3 * i, (cy + oy) * CH + 0.2 * i) for i in range(k)]


def junk_targets(k, start=0):
    """k right points in distinct cells of the two upper rows, far from every cluster's partner"""
    return [((1.25 + (start + i) % 18) * CW, (0.25 + (start + i) // 18) * CH) for i in range(k)]


def carry_over_scene():
    """Cluster A (20 matches) and cluster B (8), both with x in the last half cell, so grid type 2 drops them.  A earns its flag at grid
    type 1.  B straddles a row boundary: split 4 + 4 it fails at grid type 1 and would pass, united, at grid type 3 -- where the
    carried-over drop keeps it out."""
    a1 = [(1250.0 + i, 188.0 + 0.3 * i) for i in range(20)]
    b1 = [(1252.0 + 2 * i, y) for i, y in enumerate((354.0, 355.0, 356.0, 357.0, 361.0, 362.0, 363.0, 364.0))]
    b2 = [(x, y + 14.4) for x, y in b1]
    s = scene(a1 + b1, a1 + b2)
    s["A"], s["B"] = np.arange(20), np.arange(20, 28)
    return s


def fused_flip_values(size, span=512):
    """float32 coordinates at which floorf(v / size * 20 + 0.5f) differs between separate rounding and a contracted multiply-add.  They
    exist only half a cell in front of the image (v near -size / 40): the product rounds to -0.5f and the sum to 0, where the contracted
    form keeps a tiny negative sum that floors to -1.  (At every other cell boundary the sum is no finer than the product, and both forms
    round alike.)"""
    inv = np.float32(1.0) / np.float32(size)
    x = np.float32(-size / 40.0)
    for _ in range(span // 2):
        x = np.nextafter(x, np.float32(0.0))
    found = []
    for _ in range(span):
        v = np.array([x], np.float32) * inv
        a, _ = G._floor_int(G._scaled(v, G.GRID, True, False))
        b, _ = G._floor_int(G._scaled(v, G.GRID, True, True))
        if a[0] != b[0]:
            found.append(float(x))
        x = np.nextafter(x, np.float32(-np.inf))
    return found


def ulps(v, j):
    v = np.float32(v)
    for _ in range(abs(j)):
        v = np.nextafter(v, np.float32(np.inf if j > 0 else -np.inf))
    return float(v)


def boundary_scene():
    """(a) Ten matches whose x sits where a contracted multiply-add puts them into column -1 at grid types 2 and 4 and separate rounding
    into column 0.  Column -1 of row 5 aliases into cell (19, 4), as it does at grid types 1 and 3 for both forms; ten unrelated matches
    live there, and together they fail the threshold (10 of 20 points over 6 pairs).  Alone in cell (0, 5) the ten pass (10 points over
    6 pairs).  (b) Clusters on k / 20 and (k + 0.5) / 20 of the width and height, a few ulps either side, with the same coordinates in
    both images, including x just below the width (x / width rounds to 1.0f)."""
    flips = fused_flip_values(W)
    assert flips, "no coordinate found at which the contraction matters"
    row = 5
    c1 = [(flips[i % len(flips)], (row + 0.25) * CH + 0.2 * i) for i in range(10)]
    c2 = [((10.25) * CW + 0.3 * i, (10.25) * CH + 0.2 * i) for i in range(10)]
    j1 = cell_points(19, row - 1, 10)
    j2 = junk_targets(10)
    p1, p2 = c1 + j1, c2 + j2
    n_flip = len(c1)
    for k, r in ((1, 8), (5, 8), (10, 8), (19, 8), (20, 8), (3, 13), (12, 13), (19, 13)):
        for half in (0.0, 0.5):
            bx = np.float32((k + half) / 20.0 * W)
            pts = [(ulps(bx, j), (r + 0.25 + half) * CH + 0.1 * (j + 3)) for j in range(-3, 4) for _ in (0, 1) if ulps(bx, j) < W]
            p1 += pts
            p2 += pts
    for k in (2, 7, 19, 20):
        for half in (0.0, 0.5):
            by = np.float32((k + half) / 20.0 * H)
            pts = [((15.25) * CW + 0.1 * (j + 3), ulps(by, j)) for j in range(-3, 4) for _ in (0, 1) if ulps(by, j) < H]
            p1 += pts
            p2 += pts
    s = scene(p1, p2)
    s["flip"] = np.arange(n_flip)
    return s


def tie_threshold_scene():
    """Cells whose score sits exactly on 6 sqrt(thresh / numPair): interior cells with 4, 8 and 10 consistent matches and 4, 16 and 25
    points in the 3 x 3 block (the rest are unrelated matches in the cell to the right), an edge cell (6 pairs, 6 matches) and a corner cell
    (4 pairs, 9 matches).  Everything lies a quarter cell inside its cell, so all four grid types see the same cells."""
    p1, p2, groups, used = [], [], {}, 0
    for name, (cx, cy), k, extra in (("4", (3, 4), 4, 0), ("8", (8, 4), 8, 8), ("10", (13, 4), 10, 15), ("edge", (0, 10), 6, 0),
                                     ("corner", (0, 19), 9, 0)):
        groups[name] = np.arange(len(p1), len(p1) + k)
        p1 += cell_points(cx, cy, k)
        p2 += cell_points(cx + 4, 10 if cy == 4 else (14 if name == "edge" else 16), k)
        p1 += cell_points(cx + 1, cy, extra)
        p2 += junk_targets(extra, used)
        used += extra
    s = scene(p1, p2)
    s["groups"] = groups
    return s


def final_rule_scene(k):
    """The filter keeps exactly k (1 or 2) matches: cell L holds k matches, its right neighbour L' 4 - k, moving alike, so both score 4
    on 4 points; L' is rejected because its other neighbour L'' holds three unrelated matches."""
    p1 = cell_points(5, 8, k) + cell_points(6, 8, 4 - k) + cell_points(7, 8, 3)
    p2 = cell_points(10, 12, k) + cell_points(11, 12, 4 - k) + junk_targets(3)
    return scene(p1, p2)


def scaled_scene(ratio, n, seed, rotate=False):
    """The second image's content scaled by `ratio` about the centre (and turned by 90 degrees if `rotate`), 1 px of noise, a quarter of
    the matches random; for ratio > 1 the first image's points keep to the part that stays inside.  A left cell then covers 1 / (20 ratio)
    of the second image: ratios 2, sqrt 2, 1 / sqrt 2 and 1 / 2 are found on the right grids of 10, 14, 28 and 40 cells (scale levels
    1-4)."""
    rng = np.random.default_rng(20261900 + 977 * seed + int(1000 * ratio))
    lo = 0.5 - 0.5 * min(1.0, 1.0 / ratio)
    u = lo + (1.0 - 2.0 * lo) * rng.random((n, 2))
    v = 0.5 + ratio * (u - 0.5)
    if rotate:
        v = np.stack([1.0 - v[:, 1], v[:, 0]], axis=1)
    wh = np.array([W, H], np.float64)
    x2 = v * wh + rng.normal(0.0, 1.0, (n, 2))
    out = rng.random(n) < 0.25
    x2[out] = rng.random((int(out.sum()), 2)) * wh
    return scene(u * wh, np.clip(x2, 0.0, wh - 0.01))


def rotated_block(left, right, rot, k):
    """a 3 x 3 block of left cells about `left`, k matches each, whose right cells are the block about `right` turned by rotation type
    `rot`: consistent at that rotation type and at no other (k < 36: a cell alone does not reach the threshold)"""
    p1, p2 = [], []
    for j in range(9):
        t = int(G.PATTERN[rot][j])
        p1 += cell_points(left[0] + j % 3 - 1, left[1] + j // 3 - 1, k)
        p2 += cell_points(right[0] + t % 3 - 1, right[1] + t // 3 - 1, k)
    return p1, p2


def rotation_tie_scene(ka, kb):
    """Block A (9 ka matches) is consistent at rotation type 2 only, block B (9 kb) at rotation type 6 only: with ka = kb the runs
    (0, 2) and (0, 6) keep equally many matches, but different ones."""
    a1, a2 = rotated_block((4, 4), (12, 5), 2, ka)
    b1, b2 = rotated_block((13, 13), (5, 14), 6, kb)
    s = scene(a1 + b1, a2 + b2)
    s["A"], s["B"] = np.arange(9 * ka), np.arange(9 * ka, 9 * (ka + kb))
    return s


def unit_edge_scene():
    """1920 x 480 images, a size at which the float just below the width (height) times the float reciprocal rounds to 1.0f: the column
    (row) is then 20 on the left (dropped) and Wr on the right, which aliases into the next row.  U1: left inside cell (5, 5), right at x
    just below the width in row 7 (cell index 20 + 20 * 7: column 0 of row 8).  U2: both images at x just below the width.  U3: both at y
    just below the height."""
    w, h = 1920, 480
    xe, ye = ulps(w, -1), ulps(h, -1)
    u1l = [((5.25) * w / 20 + 0.3 * i, (5.25) * h / 20 + 0.2 * i) for i in range(12)]
    u1r = [(xe, (7.25) * h / 20 + 0.2 * i) for i in range(12)]
    u2 = [(xe, (11.25) * h / 20 + 0.2 * i) for i in range(12)]
    u3 = [((9.25) * w / 20 + 0.3 * i, ye) for i in range(12)]
    s = scene(u1l + u2 + u3, u1r + u2 + u3)
    s["size1"] = s["size2"] = (w, h)
    s["U1"] = np.arange(12)
    return s
