"""GPU: pre/post steps of the pose path (ImgToCamCoordTrans, Remove_LensDist, getInliers) vs the oracle, bit-exact."""
import numpy as np
import pytest

from matchinglib_poselib_amd import pose, synth

pytestmark = pytest.mark.gpu


def distort(p, d):
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    r2 = x * x + y * y
    rc = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    dx = p1 * 2 * x * y + p2 * (r2 + 2 * x * x)
    dy = p1 * (r2 + 2 * y * y) + p2 * 2 * x * y
    return np.stack([x * rc + dx, y * rc + dy], axis=1).astype(np.float32)


def test_img_to_cam(ctx, oracle):
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 1200, (5000, 2)).astype(np.float32)
    K4 = np.array([812.3, 807.9, 611.2, 377.7])
    g = pose.ImgToCamCoordTrans(pts, K4, ctx=ctx)
    assert g.tobytes() == oracle.img_to_cam(pts, K4).tobytes()


def test_remove_lens_dist(ctx, oracle):
    p1, p2, *_ = synth.pose_scene(3000, seed=9)
    d1 = np.array([-0.28, 0.09, 1e-3, -5e-4, -0.012, 0.0, 0.0, 0.0])
    d2 = np.array([-0.31, 0.11, -8e-4, 7e-4, 0.0, 0.01, -0.002, 0.0])
    a, b = distort(p1 * 1.6, d1), distort(p2 * 1.6, d2)
    a[17] = [9.0, 9.0]      # far outside the model's valid range: must be dropped, order of the rest kept
    b[400] = [-7.0, 8.0]
    ok_o, ao, bo = oracle.remove_lens_dist(a, b, d1, d2)
    ok_g, ag, bg = pose.Remove_LensDist(a, b, d1, d2, ctx=ctx)
    assert ok_o and ok_g and len(ag) == len(ao) < 3000
    assert ag.tobytes() == ao.tobytes() and bg.tobytes() == bo.tobytes()
    # undistortion really inverts the model
    keep = np.ones(3000, bool)
    # zero coefficients: untouched
    ok_g, ag, bg = pose.Remove_LensDist(a, b, np.zeros(8), np.zeros(8), ctx=ctx)
    assert ok_g and ag.tobytes() == a.tobytes()
    # fewer than 16 survivors -> false
    bad = np.full((20, 2), 30.0, np.float32)
    ok_o, _, _ = oracle.remove_lens_dist(bad, bad, d1, d2)
    ok_g, _, _ = pose.Remove_LensDist(bad, bad, d1, d2, ctx=ctx)
    assert not ok_o and not ok_g


def test_get_inliers_strict(ctx, oracle):
    p1, p2, R, t, mask, th = synth.pose_scene(4000, seed=10)
    o = oracle.ransac_essential(p1, p2, th, max_iters=200, seed=1)
    cnt_o, m_o, e_o = oracle.get_inliers_strict(p1, p2, o["E"], th * th)
    cnt_g, m_g, e_g = pose.getInliers(o["E"], p1, p2, th * th, ctx=ctx)
    assert cnt_g == cnt_o and np.array_equal(m_g, m_o) and e_g.tobytes() == e_o.tobytes()
    # strictness: a threshold equal to one of the errors excludes that point here, includes it in RANSAC's <=
    k = int(np.argsort(e_o)[1000])
    cnt2, m2, _ = pose.getInliers(o["E"], p1, p2, e_o[k], ctx=ctx)
    assert m2[k] == 0 and cnt2 == int((e_o < e_o[k]).sum())


# ---- edge sizes and drop patterns ------------------------------------------------------------------------------------------------------
# undistort_kernel counts the survivors of every 64 rows (one wave = one group), compact_pairs_kernel puts four groups into a 256-thread block
# and sums the counts of all groups before its own (256 per trip: a second trip from 16641 rows on).

D1 = np.array([-0.28, 0.09, 1e-3, -5e-4, -0.012, 0.0, 0.0, 0.0])
D2 = np.array([-0.31, 0.11, -8e-4, 7e-4, 0.0, 0.01, -0.002, 0.0])
FAIL1, FAIL2 = (9.0, 9.0), (-7.0, 8.0)   # far outside either model's valid range
LENS_SIZES = (16, 17, 63, 64, 65, 255, 256, 257, 1000, 16705)   # 16705 = 262 groups, 66 blocks: the prefix loop's second trip
PATTERNS = ("none", "ends", "lanes_0_63", "first_group", "last_group", "middle_block", "every_second", "view2_only", "view1_only")


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257))
def test_img_to_cam_edge_sizes(ctx, oracle, n):
    rng = np.random.default_rng(n)
    pts = rng.uniform(-1200, 1200, (n, 2)).astype(np.float32)
    special = np.array([[0.0, 0.0], [-0.0, 611.2], [1e4, -1e4], [9999.5, 10000.25], [-3.5, 0.0], [812.3, 377.7]], np.float32)
    rows = rng.permutation(n)[:len(special)]
    pts[rows] = special[:len(rows)]
    K4 = np.array([812.3, 807.9, 611.2, 377.7])
    g = pose.ImgToCamCoordTrans(pts, K4, ctx=ctx)
    assert g.shape == (n, 2) and g.tobytes() == oracle.img_to_cam(pts, K4).tobytes()
    if n >= 255:
        assert (pts < 0).any() and (pts == 0).any() and (np.abs(pts) >= 9999).any()


_lens = {}


def _lens_points(n):
    if n not in _lens:
        p1, p2, *_ = synth.pose_scene(n, seed=9 + n)
        _lens[n] = (distort(p1 * 1.4, D1), distort(p2 * 1.4, D2))   # (at 1.4 no row fails on its own at any size used here: _check_lens)
    return _lens[n]


def _planted(n, pattern):
    """-> rows that fail in view 1, rows that fail in view 2 (planted by index).  `middle_block`: one whole 256-row block of
    compact_pairs_kernel, the one in the middle (the first where there are fewer than three)."""
    last = (n - 1) // 64 * 64
    rows = {"none": [], "ends": [0, n - 1], "lanes_0_63": [i for i in range(n) if i % 64 in (0, 63)], "first_group": range(min(64, n)),
            "last_group": range(last, n), "middle_block": range(n // 512 * 256, min(n, n // 512 * 256 + 256)), "every_second": range(0, n, 2),
            "view2_only": range(1, n, 3), "view1_only": range(2, n, 3)}[pattern]
    rows = np.array(sorted(set(rows)), np.int64)
    if pattern == "view2_only":
        return rows[:0], rows
    if pattern == "view1_only":
        return rows, rows[:0]
    return rows[::2], rows[1::2]


def _check_lens(ctx, oracle, a, b, d1, d2, survivors):
    """Byte equality of the flag and of both arrays; `survivors` (or None) is what the planted rows leave."""
    ok_o, ao, bo = oracle.remove_lens_dist(a, b, d1, d2)
    ok_g, ag, bg = pose.Remove_LensDist(a, b, d1, d2, ctx=ctx)
    if survivors is not None:
        assert ok_o == (survivors >= 16) and len(ao) == (survivors if ok_o else len(a)), "the planted rows, and only they, fail"
    assert ok_g == ok_o and ag.shape == ao.shape and bg.shape == bo.shape
    assert ag.tobytes() == ao.tobytes() and bg.tobytes() == bo.tobytes()
    return ok_g, ag, bg


@pytest.mark.parametrize("n", LENS_SIZES)
def test_remove_lens_dist_drop_patterns(ctx, oracle, n):
    for pattern in PATTERNS:
        a, b = (x.copy() for x in _lens_points(n))
        r1, r2 = _planted(n, pattern)
        a[r1], b[r2] = FAIL1, FAIL2
        ok, ag, bg = _check_lens(ctx, oracle, a, b, D1, D2, n - len(r1) - len(r2))
        if not ok:   # the uncompacted values: view 2 of a pair that failed in view 1 as it came in
            assert bg[r1].tobytes() == b[r1].tobytes() and len(ag) == n
            keep = np.setdiff1d(np.arange(n), np.concatenate([r1, r2]))
            assert len(keep) < 16 and (len(keep) == 0 or not np.array_equal(ag[keep], a[keep]))


def test_remove_lens_dist_sixteen_survivors(ctx, oracle):
    """Exactly 16 survivors: true; exactly 15: false."""
    for n, drop in ((16, 0), (16, 1), (17, 1), (17, 2), (80, 64), (80, 65), (300, 284), (300, 285)):
        a, b = (x.copy() for x in _lens_points(n))
        rows = np.random.default_rng(n + drop).permutation(n)[:drop]
        a[rows[::2]], b[rows[1::2]] = FAIL1, FAIL2
        ok, ag, bg = _check_lens(ctx, oracle, a, b, D1, D2, n - drop)
        assert ok == (n - drop == 16) and len(ag) == (16 if ok else n)
    # the whole first 256-thread block and every row but 500 .. 515 dropped: the survivors straddle two blocks behind an empty one
    n = 600
    a, b = (x.copy() for x in _lens_points(n))
    a[:500] = FAIL1
    b[516:] = FAIL2
    ok, ag, bg = _check_lens(ctx, oracle, a, b, D1, D2, 16)
    assert ok and len(ag) == 16


def test_remove_lens_dist_near_zero_coefficient_sums(ctx, oracle):
    """Nonzero coefficients whose sum lies inside +-1e-3 (nearZero(sum), pose_helper.cpp:1176-1178): both sums inside leave the input
    untouched, planted rows included; one inside and one outside undistorts both views."""
    n = 257
    a, b = (x.copy() for x in _lens_points(n))
    a[3], b[200] = FAIL1, FAIL2
    z1 = np.array([0.3, -0.3, 4e-4, 0.0, 0.1, -0.1, 2e-4, 0.0])       # sum 6e-4
    z2 = np.array([-0.25, 0.25, 0.0, -9e-4, 0.0, 0.0, 0.0, 0.0])      # sum -9e-4
    assert abs(z1.sum()) < 1e-3 and abs(z2.sum()) < 1e-3
    ok, ag, bg = _check_lens(ctx, oracle, a, b, z1, z2, None)
    assert ok and ag.tobytes() == a.tobytes() and bg.tobytes() == b.tobytes()
    for d1, d2 in ((z1, D2), (D1, z2)):
        ok, ag, bg = _check_lens(ctx, oracle, a, b, d1, d2, None)
        assert len(ag) < n or not ok or ag.tobytes() != a.tobytes()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 1000))
def test_get_inliers_edge_sizes_and_thresholds(ctx, oracle, n):
    p1, p2, R, t, mask, th = synth.pose_scene(n, 0.8, seed=10 + n)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R / np.linalg.norm(tx @ R)
    _, _, e = oracle.get_inliers_strict(p1, p2, E, th * th)
    assert e.min() > 0
    k = int(np.argsort(e)[n // 2])
    for th2, want in ((e.min() / 2, 0), (e.max() * 2, n), (e[k], int((e < e[k]).sum())), (e.min(), 0), (e.max(), n - int((e == e.max()).sum()))):
        cnt_o, m_o, e_o = oracle.get_inliers_strict(p1, p2, E, th2)
        cnt_g, m_g, e_g = pose.getInliers(E, p1, p2, th2, ctx=ctx)
        assert cnt_o == want and cnt_g == cnt_o and m_g.tobytes() == m_o.tobytes() and e_g.tobytes() == e_o.tobytes()
        assert cnt_g == np.count_nonzero(m_g) and e_o.tobytes() == e.tobytes()
    assert pose.getInliers(E, p1, p2, e[k], ctx=ctx)[1][k] == 0   # strict: the point whose error is the threshold is out
