"""Restatements of the GMS match filter (matchinglib::filterMatchesGMS over gms-1.0's MatchGMS) for the tests.

gms_oracle   -- the literal one: the reference's loops (scale level, rotation type, grid type), dense motion tables, float32 arithmetic with
                every operation rounded separately, the threshold in float64.
gms_buckets  -- an independent one, sharing no helper or table with the first: its own scalar cell arithmetic (_bucket_codes: normalisation,
                bounds and drop rule), its own rotation table derived from angles (_bucket_pattern) and right-grid sizes, no dense table
                (sorted pair keys and searches), one pass per (scale level, grid type) serving all rotation types, the threshold compared
                in integers with math.sqrt at exact ties.
Both apply the library's documented deviations (include/mlpl_c.h): where the reference would read or write out of bounds, or convert an
unrepresentable float to int, the match is dropped like a negative index and counted.  Neither is compiled from the reference (it needs
OpenCV); parity rests on the two having been written separately against MatchGMS.cpp.

Switches of gms_oracle used to build test scenes: fused=True emulates a contracted multiply-add in `x * 20 + 0.5f`; carry=False switches
the carried-over drop off (a match dropped at one grid type is then looked at afresh at the next).
"""
import math

import numpy as np

GRID = 20
RIGHT_SIZE = tuple(int(GRID * r) for r in (1.0, 1.0 / 2, 1.0 / math.sqrt(2.0), math.sqrt(2.0), 2.0))   # 20, 10, 14, 28, 40
REF_DROP, DEV_DROP = -1, -2


def rotation_patterns():
    """pattern[r][j] = the 0-based slot of the right 3 x 3 block that slot j of the left block is compared with at rotation type r: the
    eight outer slots, taken clockwise, move by r places; the centre stays."""
    ring = [0, 1, 2, 5, 8, 7, 6, 3]
    pat = np.full((8, 9), 4, np.int64)
    for r in range(8):
        for t, j in enumerate(ring):
            pat[r, j] = ring[(t - r) % 8]
    return pat


PATTERN = rotation_patterns()


def neighbours(w, h):
    """N9 of every cell of a w x h grid, row by row from the upper left; -1 where the neighbour is outside."""
    n9 = np.full((w * h, 9), -1, np.int64)
    for c in range(w * h):
        x, y = c % w, c // w
        for yi in (-1, 0, 1):
            for xi in (-1, 0, 1):
                xx, yy = x + xi, y + yi
                if 0 <= xx < w and 0 <= yy < h:
                    n9[c, xi + 4 + yi * 3] = xx + yy * w
    return n9


LEFT_N9 = neighbours(GRID, GRID)
RIGHT_N9 = {w: neighbours(w, w) for w in RIGHT_SIZE}


def normalise(kp, size):
    kp = np.asarray(kp, np.float32).reshape(-1, 2)
    winv, hinv = np.float32(1.0) / np.float32(size[0]), np.float32(1.0) / np.float32(size[1])
    with np.errstate(all="ignore"):
        return kp[:, 0] * winv, kp[:, 1] * hinv


def _scaled(v, size, half, fused):
    with np.errstate(all="ignore"):
        if half and fused:
            return (v.astype(np.float64) * float(size) + 0.5).astype(np.float32)   # one rounding: the product is exact in double
        p = v * np.float32(size)
        return p + np.float32(0.5) if half else p


def _floor_int(f):
    """floorf and the conversion to int; ok = the floor is finite and fits an int."""
    with np.errstate(all="ignore"):
        fl = np.floor(f)
        ok = np.isfinite(fl) & (fl >= np.float32(-2147483648.0)) & (fl < np.float32(2147483648.0))
    return np.where(ok, fl, 0).astype(np.int64), ok


def left_codes(xn, yn, grid_type, fused=False):
    x, okx = _floor_int(_scaled(xn, GRID, grid_type in (2, 4), fused))
    y, oky = _floor_int(_scaled(yn, GRID, grid_type in (3, 4), fused))
    idx = x + GRID * y
    code = np.where((x >= GRID) | (y >= GRID) | (idx < 0), REF_DROP, idx)
    return np.where(okx & oky, code, DEV_DROP)


def right_codes(xn, yn, w):
    x, okx = _floor_int(_scaled(xn, w, False, False))
    y, oky = _floor_int(_scaled(yn, w, False, False))
    idx = x + w * y
    code = np.where(idx < 0, REF_DROP, np.where(idx >= w * w, DEV_DROP, idx))
    return np.where(okx & oky, code, DEV_DROP)


def _match_arrays(matches):
    if isinstance(matches, np.ndarray) and matches.dtype.names:
        return matches["queryIdx"].astype(np.int64), matches["trainIdx"].astype(np.int64)
    m = np.asarray(matches, np.int64).reshape(-1, 2)
    return m[:, 0], m[:, 1]


def gms_oracle(kp1, size1, kp2, size2, matches, use_scale=False, use_rotation=False, fused=False, carry=True):
    q, t = _match_arrays(matches)
    n = len(q)
    x1, y1 = normalise(kp1, size1)
    x2, y2 = normalise(kp2, size2)
    x1, y1, x2, y2 = x1[q], y1[q], x2[t], y2[t]
    best = dict(keep=np.zeros(n, bool), n_keep=0, scale=-1, rotation=-1, dropped=0)
    counts, masks = {}, {}
    for scale in range(5 if use_scale else 1):
        w = RIGHT_SIZE[scale]
        cells_r = w * w
        right_n9 = RIGHT_N9[w]
        for rot in range(8 if use_rotation else 1):
            inlier = np.zeros(n, bool)
            pair_l = np.zeros(n, np.int64)
            pair_r = np.zeros(n, np.int64)
            gone = np.zeros(n, bool)
            dev = np.zeros(n, bool)
            for grid_type in (1, 2, 3, 4):
                motion = np.zeros((GRID * GRID, cells_r), np.int64)
                lc = left_codes(x1, y1, grid_type, fused)
                if grid_type == 1:
                    pair_r = right_codes(x2, y2, w)
                if not carry:
                    gone = np.zeros(n, bool)
                live = ~gone
                bad = live & ((lc < 0) | (pair_r < 0))
                dev |= live & ((lc == DEV_DROP) | (pair_r == DEV_DROP))
                gone = gone | bad
                live = ~gone
                pair_l = np.where(live, lc, -1)
                np.add.at(motion, (pair_l[live], pair_r[live]), 1)
                points = np.bincount(pair_l[live], minlength=GRID * GRID)
                # verifyCellPairs
                partner = np.where(motion.sum(axis=1) == 0, -1, motion.argmax(axis=1))   # argmax: the first maximum
                ll = LEFT_N9
                rr = right_n9[np.maximum(partner, 0)][:, PATTERN[rot]]
                valid = (ll >= 0) & (rr >= 0)
                score = (motion[np.maximum(ll, 0), np.maximum(rr, 0)] * valid).sum(axis=1)
                thresh = (points[np.maximum(ll, 0)] * valid).sum(axis=1).astype(np.float64)
                num_pair = valid.sum(axis=1)
                thresh = 6.0 * np.sqrt(thresh / num_pair)
                partner = np.where((partner >= 0) & (score < thresh), -2, partner)
                inlier[live] |= partner[pair_l[live]] == pair_r[live]
            count = int(inlier.sum())
            counts[(scale, rot)] = count
            masks[(scale, rot)] = inlier.copy()
            if count > best["n_keep"]:
                best = dict(keep=inlier.copy(), n_keep=count, scale=scale, rotation=rot, dropped=int(dev.sum()))
    best["counts"], best["masks"] = counts, masks   # every run's count and mask, for the tests that look for ties
    return best


def _bucket_pattern():
    """The rotation table again, from geometry: slot j of a 3 x 3 block lies at the offset (j % 3 - 1, j // 3 - 1), y pointing down; rotation
    type r turns an outer offset by r eighths of a turn against the clockwise order of the ring and leaves the centre alone."""
    table = []
    for r in range(8):
        row = []
        for j in range(9):
            dx, dy = j % 3 - 1, j // 3 - 1
            if dx or dy:
                a = math.atan2(dy, dx) - r * math.pi / 4.0
                dx, dy = int(round(1.3 * math.cos(a))), int(round(1.3 * math.sin(a)))
            row.append(dx + 1 + 3 * (dy + 1))
        table.append(row)
    return table


def _bucket_cell(v, size, half):
    """one coordinate's column or row: the float32 product, the separately rounded + 0.5f, the floor as a Python int; None where the
    floor is not finite or does not fit an int"""
    with np.errstate(all="ignore"):
        p = np.float32(v) * np.float32(size)
        if half:
            p = np.float32(p + np.float32(0.5))
    if not math.isfinite(p):
        return None
    f = math.floor(float(p))
    return f if -2 ** 31 <= f < 2 ** 31 else None


def _bucket_codes(kp1, size1, kp2, size2, q, t, sizes):
    """per match: the four left cells (grid types 1-4) and one right cell per right-grid size; >= 0 a cell, -1 dropped as the reference
    drops it, -2 dropped by the library's out-of-bounds rule.  Scalar code, sharing nothing with left_codes / right_codes."""
    kp1, kp2 = np.asarray(kp1, np.float32).reshape(-1, 2), np.asarray(kp2, np.float32).reshape(-1, 2)
    one = np.float32(1.0)
    wi1, hi1, wi2, hi2 = one / np.float32(size1[0]), one / np.float32(size1[1]), one / np.float32(size2[0]), one / np.float32(size2[1])
    left = np.empty((4, len(q)), np.int64)
    right = np.empty((len(sizes), len(q)), np.int64)
    for i, (a, b) in enumerate(zip(q.tolist(), t.tolist())):
        with np.errstate(all="ignore"):
            xn, yn, xr, yr = kp1[a, 0] * wi1, kp1[a, 1] * hi1, kp2[b, 0] * wi2, kp2[b, 1] * hi2
        for g, (hx, hy) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            x, y = _bucket_cell(xn, 20, hx), _bucket_cell(yn, 20, hy)
            if x is None or y is None:
                left[g, i] = -2
            elif x >= 20 or y >= 20 or x + 20 * y < 0:
                left[g, i] = -1
            else:
                left[g, i] = x + 20 * y
        for k, w in enumerate(sizes):
            x, y = _bucket_cell(xr, w, False), _bucket_cell(yr, w, False)
            if x is None or y is None:
                right[k, i] = -2
            else:
                c = x + w * y
                right[k, i] = -1 if c < 0 else (-2 if c >= w * w else c)
    return left, right


def gms_buckets(kp1, size1, kp2, size2, matches, use_scale=False, use_rotation=False):
    q, t = _match_arrays(matches)
    n = len(q)
    sizes = [int(20 * r) for r in (1.0, 0.5, 0.5 ** 0.5, 2.0 ** 0.5, 2.0)][: 5 if use_scale else 1]
    pattern = _bucket_pattern()
    lcs, rcs = _bucket_codes(kp1, size1, kp2, size2, q, t, sizes)
    n_rot = 8 if use_rotation else 1
    best = dict(keep=np.zeros(n, bool), n_keep=0, scale=-1, rotation=-1, dropped=0)
    for scale, w in enumerate(sizes):
        big = w * w
        rc = rcs[scale]
        flags = np.zeros((n_rot, n), bool)
        alive = np.ones(n, bool)
        dev = 0
        for lc in lcs:
            fail = alive & ((lc < 0) | (rc < 0))
            dev += int((fail & ((lc == -2) | (rc == -2))).sum())
            alive &= ~fail
            ids = np.nonzero(alive)[0]
            keys, cnt = np.unique(lc[ids] * big + rc[ids], return_counts=True)
            kl, kr = keys // big, keys % big
            table = dict(zip(keys.tolist(), cnt.tolist()))
            pts = {}
            for a, c in zip(kl.tolist(), cnt.tolist()):
                pts[a] = pts.get(a, 0) + c
            partner = {}
            for a, b, c in zip(kl.tolist(), kr.tolist(), cnt.tolist()):   # keys ascend: the first of equal counts stays
                if a not in partner or c > partner[a][1]:
                    partner[a] = (b, c)
            accept = {}
            for a, (b, _) in partner.items():
                ax, ay, bx, by = a % 20, a // 20, b % w, b // w
                for rot in range(n_rot):
                    score = total = pairs = 0
                    for j in range(9):
                        k = pattern[rot][j]
                        lx, ly, rx, ry = ax + j % 3 - 1, ay + j // 3 - 1, bx + k % 3 - 1, by + k // 3 - 1
                        if not (0 <= lx < 20 and 0 <= ly < 20 and 0 <= rx < w and 0 <= ry < w):
                            continue
                        la = lx + 20 * ly
                        score += table.get(la * big + rx + w * ry, 0)
                        total += pts.get(la, 0)
                        pairs += 1
                    lhs, rhs = score * score * pairs, 36 * total
                    reject = lhs < rhs if lhs != rhs else score < 6.0 * math.sqrt(total / pairs)
                    accept[(a, rot)] = not reject
            for i in ids.tolist():
                a = int(lc[i])
                if partner[a][0] == rc[i]:
                    for rot in range(n_rot):
                        if accept[(a, rot)]:
                            flags[rot, i] = True
        for rot in range(n_rot):
            c = int(flags[rot].sum())
            if c > best["n_keep"]:
                best = dict(keep=flags[rot].copy(), n_keep=c, scale=scale, rotation=rot, dropped=dev)
    return best
