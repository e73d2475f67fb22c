"""Test helper (not a fixture file): the shape / tie / extremes list every Hamming kernel instance is checked on against the oracle,
shared by test_gpu_matching.py and test_gpu_hamming_instances.py."""
import numpy as np

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import synth

# (nq, nt, descriptor bytes, k): around the tile sizes (32-row MFMA tiles, 128-row LDS tiles), descriptor widths around the K-step
# (8 bytes), ragged last tiles, k = 1
HAMMING_SHAPES = [(1, 2, 32, 2), (15, 15, 32, 2), (64, 1000, 32, 1), (300, 129, 32, 2), (1000, 5000, 32, 2),
                  (77, 333, 64, 2), (50, 200, 16, 2), (40, 90, 61, 2), (33, 70, 24, 2), (20, 40, 1, 2),
                  (10, 600, 128, 2), (31, 33, 8, 2), (129, 4097, 32, 2), (513, 31, 32, 2), (2048, 2048, 32, 2),
                  (100, 9000, 64, 2), (640, 96, 9, 2)]


def check_hamming_cases(ctx, oracle, tag, after_call=None, shapes=HAMMING_SHAPES):
    """knn_hamming on every shape, on heavy ties and on the extremes of the distance range, then the fused getMatches path: the oracle's
    (distance, index) pairs bit for bit.  after_call(nq, nt, nbytes) runs after every knn_hamming call (instance checks)."""
    for nq, nt, nbytes, k in shapes:
        q, t = synth.orb_pair(nq, nt, nbytes=nbytes, seed=2000 + nq + nt + nbytes)
        idx, dist = mpa.knn_hamming(q, t, k=k, ctx=ctx)
        if after_call:
            after_call(nq, nt, nbytes)
        oi, od = oracle.knn_hamming(q, t, k=k)
        assert np.array_equal(dist, od), (tag, nq, nt, nbytes, k)
        assert np.array_equal(idx, oi), (tag, nq, nt, nbytes, k)
    # ties everywhere: 5 distinct descriptors, the smaller train index must win in every merge level
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    t = base[rng.integers(0, 5, 3000)]
    q = base[rng.integers(0, 5, 500)]
    idx, dist = mpa.knn_hamming(q, t, ctx=ctx)
    if after_call:
        after_call(500, 3000, 32)
    oi, od = oracle.knn_hamming(q, t)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od), (tag, "ties")
    # extremes of the distance range: all-equal and all-different bits
    z = np.zeros((70, 32), np.uint8)
    o = np.full((90, 32), 255, np.uint8)
    for a, b in ((z, o), (z, z[:40]), (o, np.concatenate([z[:45], o[:3]]))):
        idx, dist = mpa.knn_hamming(a, b, ctx=ctx)
        if after_call:
            after_call(len(a), len(b), 32)
        oi, od = oracle.knn_hamming(a, b)
        assert np.array_equal(idx, oi) and np.array_equal(dist, od), (tag, "extremes", len(a), len(b))
    # the fused getMatches path
    q, t = synth.orb_pair(700, 900, seed=31)
    err, m = mpa.getMatches([None] * 700, [None] * 900, q, t, matcher_name="LINEAR", ctx=ctx)
    rc, om = oracle.get_matches_linear(700, 900, q, t)
    assert err == rc == 0 and m.tobytes() == om.tobytes(), (tag, "getMatches")
