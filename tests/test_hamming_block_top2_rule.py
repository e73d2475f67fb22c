"""CPU-only: the rule behind the block form of the running top-2 (knn_hamming_mfma.hip, option hamming_block_top2), restated in Python and
checked by brute force.  A lane of half h holds the rows of a 32-row tile with (row >> 2) & 1 == h; it folds only block maxima into its
running pair, the two halves are merged, and the rows of the one block that holds the best row -- the best itself excluded -- are looked
at again.  A block is an aligned group of four train rows.  The result must be the two smallest (distance, row) keys of the whole train
set, for every train size 1 ... 130 (ragged last tiles) and heavy ties."""
import numpy as np

NONE = 1 << 30


def lane_rows(tile, h, nt):
    return [32 * tile + lr for lr in range(32) if (lr >> 2) & 1 == h and 32 * tile + lr < nt]


def blocks_of(rows):
    groups = {}
    for r in rows:
        groups.setdefault(r >> 2, []).append(r)
    return list(groups.values())


def rescan_rows(best):
    """the rows knn_hamming_mfma.hip's block_rescan looks at: two per lane of the query"""
    return [(best & ~3) + 2 * he + i for he in (0, 1) for i in range(2)]


def block_top2(d):
    nt = len(d)
    key = lambda r: (int(d[r]) << 14) | r
    halves = []
    for h in (0, 1):
        m1 = m2 = NONE
        for tile in range((nt + 31) // 32):
            maxima = [min(key(r) for r in b) for b in blocks_of(lane_rows(tile, h, nt))]
            m1, m2 = sorted([m1, m2] + maxima)[:2]
        halves += [m1, m2]
    k0, k1 = sorted(halves)[:2]
    if k0 != NONE:
        best = k0 & 16383
        for r in rescan_rows(best):
            if r != best and r < nt:
                k1 = min(k1, key(r))
    return k0, k1


def test_block_maxima_plus_rescan_is_the_exact_top2():
    rng = np.random.default_rng(4)
    for case in range(8000):
        nt = 1 + case % 130
        d = rng.integers(0, (1, 2, 3, 40)[case % 4] + 1, nt)
        keys = sorted((int(d[r]) << 14) | r for r in range(nt)) + [NONE]
        assert block_top2(d) == (keys[0], keys[1]), (nt, d.tolist())
