"""The exactness rule of the accumulator bias of the in-kernel-expansion instances of the Hamming LDS-ring kernel (kAccBias in
knn_hamming_mfma.hip), restated in numpy float32 for the constant the library ships.

A value of those instances is  v = B + ip + f * 2^-14  with B = kAccBias, ip the integer part (256 - 2 d for a final value, any integer of
magnitude <= 256 for a partial sum of the four-MFMA chain) and f = frame - local row, where the frame is the first row of the last tile
folded: f lies in [-31, 8160] over a split of at most 8192 rows.  The kernel needs
  * every such v to be a float32 (then every MFMA accumulation and every +32 * 2^-14 re-base on the way is exact),
  * rint(v) = B + ip,
  * the decode  d = (256 - (rint(v) - B)) >> 1,  row = frame - (v - rint(v)) * 2^14  to return what went in, and
  * v to order candidates by (distance ascending, row ascending) as a plain float, largest first.
No GPU: the constant is parsed from the source file."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "matchinglib_poselib_amd", "csrc", "knn_hamming_mfma.hip")

EPS = np.float32(2.0 ** -14)
NBITS = 256
ROWS_PER_SPLIT = 8192
F_MIN, F_MAX = -31, ROWS_PER_SPLIT - 32


def _constants():
    text = open(SRC).read()
    b = re.findall(r"constexpr\s+float\s+kAccBias\s*=\s*([0-9.]+)f\s*;", text)
    r = re.findall(r"constexpr\s+int\s+kMaxRowsPerSplit\s*=\s*(\d+)\s*;", text)
    e = re.findall(r"constexpr\s+float\s+kEps\s*=\s*1\.0f\s*/\s*([0-9.]+)f\s*;", text)
    assert len(b) == 1 and len(r) == 1 and len(e) == 1, (b, r, e)
    return float(b[0]), int(r[0]), float(e[0])


@pytest.fixture(scope="module")
def grid():
    """Every (ip, f): float32 values formed as the kernel forms them (C = B - row * eps, then integers added), and the exact values."""
    bias, rows, inv_eps = _constants()
    assert rows == ROWS_PER_SPLIT and inv_eps == 16384.0
    ip = np.arange(-NBITS, NBITS + 1, dtype=np.int64)[:, None]
    f = np.arange(F_MIN, F_MAX + 1, dtype=np.int64)[None, :]
    exact = (np.float64(bias) + ip) + f.astype(np.float64) / 16384.0          # (exact in float64: 10 + 14 bits)
    v = (np.float32(bias) + (f.astype(np.float32) * EPS)) + ip.astype(np.float32)
    assert v.dtype == np.float32
    return bias, ip, f, exact, v


def test_the_bias_is_an_integer_inside_the_stated_bound():
    bias, rows, _ = _constants()
    assert bias == int(bias) and bias > 0
    assert bias + NBITS + (rows - 32) / 16384.0 < 1024.0
    assert bias - NBITS - 31 / 16384.0 > -1024.0
    assert bias - 64 >= 512 and bias + 64 < 1024      # typical data inside one binade


def test_every_value_is_a_float32(grid):
    bias, ip, f, exact, v = grid
    assert np.array_equal(v.astype(np.float64), exact)
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    # ... in whichever order the parts are added, and through the re-base: (v - 32 eps) + 32 eps
    v2 = (np.float32(bias) + ip.astype(np.float32)) + f.astype(np.float32) * EPS
    assert np.array_equal(v2, v)
    rebased = exact[:, : F_MAX - F_MIN + 1 - 32].astype(np.float32) + np.float32(32.0) * EPS
    assert np.array_equal(rebased, v[:, 32:])
    assert np.abs(exact).max() < 1024.0


def test_rint_returns_bias_plus_integer_part(grid):
    bias, ip, f, exact, v = grid
    assert np.array_equal(np.rint(v), np.broadcast_to((bias + ip).astype(np.float32), v.shape))


def test_decode_returns_distance_and_local_row(grid):
    bias, ip, f, exact, v = grid
    frame = np.float32(ROWS_PER_SPLIT - 32)                       # the last tile of a full split; local row = frame - f in [0, 8191]
    ipb = np.rint(v)
    got_ip = (ipb - np.float32(bias)).astype(np.int32)
    assert np.array_equal(got_ip, np.broadcast_to(ip, v.shape))
    lrow = (frame - (v - ipb) * np.float32(16384.0)).astype(np.int32)
    assert np.array_equal(lrow, np.broadcast_to(int(frame) - f, v.shape))
    assert lrow.min() == 0 and lrow.max() == ROWS_PER_SPLIT - 1
    even = (ip[:, 0] & 1) == 0                                    # final values: ip = 256 - 2 d
    d = (NBITS - got_ip[even]) >> 1
    assert np.array_equal(d[:, 0], np.arange(NBITS, -1, -1))
    # an earlier frame (a split of one tile): frame 0, rows 0..31
    sub = v[:, (f[0] >= -31) & (f[0] <= 0)]
    lrow0 = (np.float32(0.0) - (sub - np.rint(sub)) * np.float32(16384.0)).astype(np.int32)
    assert np.array_equal(lrow0[0], np.arange(31, -1, -1))


def test_order_is_distance_then_row(grid):
    bias, ip, f, exact, v = grid
    # lexicographic (ip ascending, f ascending) = (distance descending, row descending): strictly increasing as floats, neighbours included
    flat = v.reshape(-1)
    assert (flat[1:] > flat[:-1]).all()
    # the same distance: the smaller row is the larger value, by exactly one eps
    assert np.array_equal(v[:, 1:] - v[:, :-1], np.full((v.shape[0], v.shape[1] - 1), EPS, np.float32))
    # a smaller distance beats any row: the last row at distance d against the first row at distance d + 1
    assert (v[2:, 0] > v[:-2, -1]).all()
    assert np.float32(-np.inf) < flat[0]                          # "no candidate" stays below everything
