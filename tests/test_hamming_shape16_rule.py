"""The placement rules and the value range of the 16x16x128 form of the Hamming LDS-ring kernel (knn_hamming_mfma_lds16_kernel in
knn_hamming_mfma.hip), restated in numpy.  No GPU.

Placement.  v_mfma_f32_16x16x128_f8f6f4 with fp4 operands: for A and B alike lane l holds row / column l & 15 and the 32 K-elements of lane
group g = l >> 4 (four registers of eight nibbles); D puts column l & 15, rows 4 g + 0..3 into a lane's four registers.  The kernel uses
  * expansion wave w (word w: K-half kh = w >> 2, lane group g = w & 3), lane l: row l >> 1, plane pair l & 1, 8 bytes at
    (2 (row >> 4) + kh) * 1024 + (16 g + (row & 15)) * 16 + (l & 1) * 8  of the tile's 4 KiB fragment slot;
  * fragment s = 2 rh + kh (read by ds_read_b128 at s * 1024 + 16 l): lane l holds row 16 rh + (l & 15), word 4 kh + (l >> 4), registers =
    planes 0, 2, 1, 3 of that word;
  * query group u, K-half kh: lane l holds query 16 u + (l & 15), word 4 kh + (l >> 4), the same planes;
  * chain rh of group u: D = A[2 rh] x bq[u][0] + A[2 rh + 1] x bq[u][1] + C; register i of lane l is row 16 rh + 4 (l >> 4) + i.
The test builds a fragment slot through the expansion rule, reads it through the fragment rule, multiplies as the opcode does and checks
256 - 2 d for every (row, query) of a tile.

Values.  A value is B + I + f * 2^-14 with B = kAccBias; over the period of two tiles the chains of a pair's first tile start at
B + (32 - lr) * 2^-14, those of its second at B - lr * 2^-14, and the running pairs move by 64 * 2^-14 per pair (32 per tile in the rolled
tail): f still lies in [-31, 8160] for everything folded and in [1, 32] at most for a chain start.  Every (I, f) is enumerated as in
test_hamming_acc_bias_rule.py: a float32 (24-bit significand), fraction inside (-1/2, 1/2), exact through both re-base steps."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "matchinglib_poselib_amd", "csrc", "knn_hamming_mfma.hip")

PLANES = (0, 2, 1, 3)   # plane held by register j of an operand
FP4 = {0x2: 1, 0xA: -1}


def expand_plane(x, p):
    """nibble j of the result carries bit 4 j + p of the word: 0x2 | bit << 3"""
    x = np.asarray(x, dtype=np.uint64)
    return (((x & np.uint64(0x11111111 << p)) << np.uint64(3 - p)) | np.uint64(0x22222222)).astype(np.uint32)


def fragment_slot(t):
    """The 4 KiB fragment slot of a 32-row tile t[32][8] (uint32 words), written by the eight expansion waves."""
    slot = np.full(1024, 0xDEADBEEF, np.uint32)
    written = np.zeros(1024, bool)
    for w in range(8):
        kh, g = w >> 2, w & 3
        for l in range(64):
            row, pair = l >> 1, l & 1
            byte = (2 * (row >> 4) + kh) * 1024 + (16 * g + (row & 15)) * 16 + pair * 8
            y = int(t[row, w]) >> pair                      # planes 0, 2 of the shifted word = planes pair, pair + 2
            for j, p in enumerate((0, 2)):
                assert not written[byte // 4 + j]
                slot[byte // 4 + j] = expand_plane(y, p)
                written[byte // 4 + j] = True
    assert written.all()
    return slot


def nibbles(regs):
    """[..., 4] uint32 registers -> [..., 32] values in {-1, +1}"""
    n = (regs[..., :, None] >> (4 * np.arange(8, dtype=np.uint32))) & np.uint32(0xF)
    n = n.reshape(regs.shape[:-1] + (32,))
    assert np.isin(n, list(FP4)).all()
    return np.where(n == 0x2, 1, -1).astype(np.int64)


def mfma16(a, b, c):
    """a, b: [64 lanes][4 registers]; c: [64][4].  D[row][col] = sum over lane groups and their 32 K-elements of A[row] * B[col] + C."""
    av, bv = nibbles(a), nibbles(b)                        # [64][32]
    d = np.zeros((16, 16), np.int64)
    for g in range(4):
        d += av[16 * g:16 * g + 16] @ bv[16 * g:16 * g + 16].T
    out = np.empty((64, 4), np.int64)
    for l in range(64):
        for i in range(4):
            out[l, i] = d[4 * (l >> 4) + i, l & 15] + c[l, i]
    return out


def tile_distances(t, q):
    """t[32][8], q[128][8] raw words -> [32 rows][128 queries] of the accumulator's integer part, by the kernel's rules"""
    slot = fragment_slot(t)
    lanes = np.arange(64)
    frag = [slot[s * 256:(s + 1) * 256].reshape(64, 4) for s in range(4)]
    # what a fragment lane must hold, stated independently of the expansion
    for s in range(4):
        rh, kh = s >> 1, s & 1
        for j, p in enumerate(PLANES):
            want = expand_plane(t[16 * rh + (lanes & 15), 4 * kh + (lanes >> 4)], p)
            assert np.array_equal(frag[s][:, j], want), (s, j)
    got = np.empty((32, 128), np.int64)
    zero = np.zeros((64, 4), np.int64)
    for u in range(8):
        bq = [np.stack([expand_plane(q[16 * u + (lanes & 15), 4 * kh + (lanes >> 4)], p) for p in PLANES], axis=1) for kh in range(2)]
        for rh in range(2):
            c = mfma16(frag[2 * rh + 1], bq[1], mfma16(frag[2 * rh], bq[0], zero))
            for l in range(64):
                for i in range(4):
                    got[16 * rh + 4 * (l >> 4) + i, 16 * u + (l & 15)] = c[l, i]
    return got


def popcount_distance(t, q):
    x = t[:, None, :] ^ q[None, :, :]
    return np.unpackbits(x.view(np.uint8), axis=-1).sum(-1).astype(np.int64)


@pytest.mark.parametrize("kind", ["random", "zeros", "ones", "complement", "identical", "one_bit_per_word"])
def test_products_over_the_k_positions_give_256_minus_2d(kind):
    rng = np.random.default_rng(16128)
    t = rng.integers(0, 2 ** 32, (32, 8), dtype=np.uint64).astype(np.uint32)
    q = rng.integers(0, 2 ** 32, (128, 8), dtype=np.uint64).astype(np.uint32)
    if kind == "zeros":
        t[:] = 0
        q[::2] = 0
    elif kind == "ones":
        t[:] = 0xFFFFFFFF
        q[::2] = 0
    elif kind == "complement":
        q[:32] = ~t
    elif kind == "identical":
        q[:32] = t
        q[32:64] = t[::-1]
    elif kind == "one_bit_per_word":
        t[:] = 0
        q[:] = 0
        for r in range(32):
            t[r, r % 8] = np.uint32(1) << np.uint32(r)   # every bit position of a word, every word
    got = tile_distances(t, q)
    assert np.array_equal(got, 256 - 2 * popcount_distance(t, q))


# ---- the value range of the period of two tiles ------------------------------------------------------------------------------------------

EPS = np.float32(2.0 ** -14)
NBITS = 256
ROWS_PER_SPLIT = 8192
F_MIN, F_MAX = -31, ROWS_PER_SPLIT - 32


def _constants():
    text = open(SRC).read()
    b = re.findall(r"constexpr\s+float\s+kAccBias\s*=\s*([0-9.]+)f\s*;", text)
    r = re.findall(r"constexpr\s+int\s+kMaxRowsPerSplit\s*=\s*(\d+)\s*;", text)
    assert len(b) == 1 and len(r) == 1, (b, r)
    return float(b[0]), int(r[0])


def test_chain_starts_of_a_pair_are_floats_32_eps_apart():
    bias, rows = _constants()
    assert rows == ROWS_PER_SPLIT
    lr = np.arange(32, dtype=np.float32)
    first = np.float32(bias) + (np.float32(32.0) - lr) * EPS     # as the kernel forms cinit[0]
    second = np.float32(bias) + (np.float32(0.0) - lr) * EPS     # cinit[1]
    assert np.array_equal(first.astype(np.float64), bias + (32.0 - np.arange(32)) / 16384.0)
    assert np.array_equal(second.astype(np.float64), bias - np.arange(32) / 16384.0)
    assert np.array_equal(first - second, np.full(32, 32.0 / 16384.0, np.float32))
    assert bias + NBITS + 32.0 / 16384.0 < 1024.0


def test_every_value_of_the_two_tile_period():
    bias, _ = _constants()
    ip = np.arange(-NBITS, NBITS + 1, dtype=np.int64)[:, None]
    f = np.arange(F_MIN, F_MAX + 1, dtype=np.int64)[None, :]
    exact = (np.float64(bias) + ip) + f.astype(np.float64) / 16384.0
    v = (np.float32(bias) + f.astype(np.float32) * EPS) + ip.astype(np.float32)
    # 24-bit significand: a multiple of 2^-14 of magnitude below 2^10
    assert np.array_equal(v.astype(np.float64), exact) and np.abs(exact).max() < 1024.0
    # the fraction stays inside (-1/2, 1/2): rint() returns B + I
    frac = exact - (bias + ip)
    assert frac.min() > -0.5 and frac.max() < 0.5
    assert np.array_equal(np.rint(v), np.broadcast_to((bias + ip).astype(np.float32), v.shape))
    # the re-base of a pair (64 eps) and of a tail tile (32 eps) is exact wherever its result is inside the range
    for step in (32, 64):
        moved = v[:, : v.shape[1] - step] + np.float32(step) * EPS
        assert np.array_equal(moved, v[:, step:])
    # the order is (distance ascending, row ascending), largest first, across the two tiles of a pair too
    flat = v.reshape(-1)
    assert (flat[1:] > flat[:-1]).all()


def test_frames_of_pairs_and_tail_tiles():
    """Fractions (in eps) as the kernel moves them: a pair re-bases by 64 and starts its tiles at 32 - lr and -lr, a tail tile re-bases by
    32 and starts at -lr.  After any number of tiles every row folded reads frame - row with frame = the first row of the last tile."""
    for ntiles in range(1, 12):
        frac = {}                                        # row -> fraction of its value
        it = 0
        while it + 3 < ntiles:                           # the unrolled pairs
            frac = {r: f + 64 for r, f in frac.items()}
            for J, start in ((0, 32), (1, 0)):
                frac.update({32 * (it + J) + lr: start - lr for lr in range(32)})
            it += 2
        while it < ntiles:                               # the rolled tail (the ragged tile included)
            frac = {r: f + 32 for r, f in frac.items()}
            frac.update({32 * it + lr: -lr for lr in range(32)})
            it += 1
        frame = 32 * (ntiles - 1)
        assert frac == {r: frame - r for r in range(32 * ntiles)}
        assert min(frac.values()) == -31 and max(frac.values()) == frame <= F_MAX
