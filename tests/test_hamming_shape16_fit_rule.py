"""CPU-only: the two rules the 16x16x128 throughput instance of the Hamming LDS-ring kernel (knn_hamming_mfma_lds16_kernel in knn_hamming_mfma.hip)
rests on, restated in Python / numpy float32 and checked by brute force.

1. The block of eight.  A query's candidates of a 32-row tile sit in the four lanes with equal lane & 15: lane group g holds the local rows
   16 h + 4 g + i (h < 2, i < 4) -- its eight accumulator registers, ONE block.  Per tile a lane folds only the block's maximum g into its running
   pair: m2 = med3(m1, m2, g), m1 = max(m1, g).  m1 is then the exact best of the lane's rows and m2 at least the best of every block but the one
   holding m1's row.  The four lanes are merged, and the seven other rows of the block that holds the best row are scored again (block_rescan8:
   lane group g takes rows base + g and base + 16 + g, the best row itself and rows >= nt excluded).  The result must be the two smallest
   (distance, row) keys of the whole train set.

2. The absolute row in C.  The accumulators of the tile that starts at row 32 t of a split start at kAccBias - (32 t + lr) * 2^-14, formed from
   kAccBias - lr * 2^-14 by one float32 add of -32 * 2^-14 per tile, so a value -- final or a partial sum of a chain -- is
   v = kAccBias + I - r * 2^-14 with |I| <= 256 and r the row within the split, r <= kMaxRowsPerSplit - 1.  The running pairs are never re-based;
   the decode reads d = (256 - (rint(v) - kAccBias)) >> 1 and r = -(v - rint(v)) * 2^14.  Checked over every (I, r) for the constants parsed from
   the source: representable, rint, decode, and the order (distance ascending, row ascending) as a plain float, largest first."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "matchinglib_poselib_amd", "csrc", "knn_hamming_mfma.hip")

NONE = 1 << 30
SHIFT = 14


# ---- 1. the block of eight ------------------------------------------------------------------------------------------------------------------

def lane_block(tile, g, nt):
    """rows of tile `tile` in lane group g: one block"""
    return [32 * tile + 16 * h + 4 * g + i for h in (0, 1) for i in range(4) if 32 * tile + 16 * h + 4 * g + i < nt]


def rescan_rows(best):
    """the rows block_rescan8 looks at, two per lane of the query"""
    return [(best & ~19) + 16 * h + g for g in range(4) for h in (0, 1)]


def block8_top2(d):
    nt = len(d)
    key = lambda r: (int(d[r]) << SHIFT) | r
    lanes = []
    for g in range(4):
        m1 = m2 = NONE
        for tile in range((nt + 31) // 32):
            blk = lane_block(tile, g, nt)
            gmax = min(key(r) for r in blk) if blk else NONE   # (rows >= nt start at -inf and stay there)
            m2 = sorted([m1, m2, gmax])[1]
            m1 = min(m1, gmax)
        lanes += [m1, m2]
    k0, k1 = sorted(lanes)[:2]
    if k0 != NONE:
        best = k0 & ((1 << SHIFT) - 1)
        for r in rescan_rows(best):
            if r != best and r < nt:
                k1 = min(k1, key(r))
    return k0, k1


def exact_top2(d):
    keys = sorted((int(d[r]) << SHIFT) | r for r in range(len(d))) + [NONE]
    return keys[0], keys[1]


def test_the_rescan_covers_exactly_the_block_of_the_best_row():
    for best in range(0, 8192):
        tile, g = best >> 5, (best >> 2) & 3
        assert sorted(rescan_rows(best)) == lane_block(tile, g, 1 << 20)
        assert best in rescan_rows(best)


def test_block_maxima_plus_rescan_is_the_exact_top2_random_and_ties():
    rng = np.random.default_rng(16)
    for case in range(8000):
        nt = 1 + case % 130
        d = rng.integers(0, (1, 2, 3, 40)[case % 4] + 1, nt)
        assert block8_top2(d) == exact_top2(d), (nt, d.tolist())


@pytest.mark.parametrize("off", [1, 2, 3, 16, 17, 18, 19, 4])
def test_planted_second(off):
    """The second neighbour at each of the seven other rows of the best row's block (+1, +2, +3, +16 ... +19 from the block's first row), and
    outside it (+4: the next lane group); either of the two is the best.  Everything else is far away or -- second loop -- ties with the second."""
    rng = np.random.default_rng(off)
    for nt in (32, 33, 52, 64, 100, 130):
        for base in range(0, nt, 32):
            for g in range(4):
                a, b = base + 4 * g, base + 4 * g + off
                if b >= nt:
                    continue
                for first, second in ((a, b), (b, a)):
                    d = rng.integers(50, 200, nt)
                    d[first], d[second] = 0, 1
                    assert block8_top2(d) == ((0 << SHIFT) | first, (1 << SHIFT) | second), (nt, first, second)
                    d[:] = 1           # ties within the block and across blocks: the smallest row wins
                    d[first] = 0
                    assert block8_top2(d) == exact_top2(d), (nt, first)
                    d[:] = 0           # all equal
                    assert block8_top2(d) == exact_top2(d)


@pytest.mark.parametrize("nt", [1, 2, 31, 33, 48, 52, 63, 65, 100])
def test_best_row_in_a_ragged_tile(nt):
    """The best row in the last, ragged tile, whose block is cut by nt in either row half; the second in the block, in the tile, or before it."""
    rng = np.random.default_rng(nt)
    last0 = (nt - 1) & ~31
    for best in range(last0, nt):
        for second in list(range(last0, nt)) + [0, max(0, last0 - 1)]:
            d = rng.integers(50, 200, nt)
            d[second] = 1
            d[best] = 0
            assert block8_top2(d) == exact_top2(d), (nt, best, second)


# ---- 2. the absolute row in C ---------------------------------------------------------------------------------------------------------------

EPS = np.float32(2.0 ** -14)
NBITS = 256


def _constants():
    text = open(SRC).read()
    b = re.findall(r"constexpr\s+float\s+kAccBias\s*=\s*([0-9.]+)f\s*;", text)
    r = re.findall(r"constexpr\s+int\s+kMaxRowsPerSplit\s*=\s*(\d+)\s*;", text)
    e = re.findall(r"constexpr\s+float\s+kEps\s*=\s*1\.0f\s*/\s*([0-9.]+)f\s*;", text)
    assert len(b) == 1 and len(r) == 1 and len(e) == 1, (b, r, e)
    return float(b[0]), int(r[0]), float(e[0])


@pytest.fixture(scope="module")
def grid():
    """Every (I, r): float32 values formed as the kernel forms them -- C of tile 0, -32 eps per tile, then integers added -- and the exact values."""
    bias, rows, inv_eps = _constants()
    assert inv_eps == 16384.0 and rows % 32 == 0
    lr = np.arange(32, dtype=np.float32)
    c = np.float32(bias) - lr * EPS
    cs = []
    for _ in range(rows // 32):
        cs.append(c)
        c = c + np.float32(-32.0) * EPS
        assert c.dtype == np.float32
    c_all = np.concatenate(cs)[None, :]                         # [1][rows]: C of row r
    ip = np.arange(-NBITS, NBITS + 1, dtype=np.int64)[:, None]
    r = np.arange(rows, dtype=np.int64)[None, :]
    exact = (np.float64(bias) + ip) - r.astype(np.float64) / 16384.0
    v = c_all + ip.astype(np.float32)
    assert v.dtype == np.float32
    return bias, rows, ip, r, exact, v


def test_bounds_of_the_absolute_form():
    bias, rows, _ = _constants()
    assert bias == int(bias)
    assert bias + NBITS < 1024.0 and bias - NBITS - (rows - 1) / 16384.0 > -1024.0
    assert (rows - 1) / 16384.0 < 0.5
    assert bias - 64 - (rows - 1) / 16384.0 >= 512 and bias + 64 < 1024      # typical data inside one binade


def test_every_value_is_a_float32(grid):
    bias, rows, ip, r, exact, v = grid
    assert np.array_equal(v.astype(np.float64), exact)
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    # a chain adds its integer in two parts (two MFMAs of 128 products): any split of I
    for part in (-128, -1, 1, 128):
        v2 = (v[0:1] + np.float32(NBITS + part)) + np.float32(-part)       # I = -256 + (256 + part) - part
        assert np.array_equal(v2, v[NBITS:NBITS + 1])
    assert np.abs(exact).max() < 1024.0


def test_rint_returns_bias_plus_integer_part(grid):
    bias, rows, ip, r, exact, v = grid
    assert np.array_equal(np.rint(v), np.broadcast_to((bias + ip).astype(np.float32), v.shape))


def test_decode_returns_distance_and_row(grid):
    bias, rows, ip, r, exact, v = grid
    ipb = np.rint(v)
    got_ip = (ipb - np.float32(bias)).astype(np.int32)
    assert np.array_equal(got_ip, np.broadcast_to(ip, v.shape))
    row = (np.float32(0.0) - (v - ipb) * np.float32(16384.0)).astype(np.int32)
    assert np.array_equal(row, np.broadcast_to(r, v.shape))
    even = (ip[:, 0] & 1) == 0
    d = (NBITS - got_ip[even]) >> 1
    assert np.array_equal(d[:, 0], np.arange(NBITS, -1, -1))


def test_order_is_distance_then_row(grid):
    bias, rows, ip, r, exact, v = grid
    # (I ascending, row descending) is strictly increasing as floats: a smaller distance beats any row, and at equal distance the smaller row
    flat = v[:, ::-1].reshape(-1)
    assert (flat[1:] > flat[:-1]).all()
    assert np.array_equal(v[:, :-1] - v[:, 1:], np.full((v.shape[0], v.shape[1] - 1), EPS, np.float32))
    assert np.float32(-np.inf) < flat[0]
