"""CPU only: the restatement of recover_pose_oracle.py is pinned by the C oracle on every case of recover_pose_scenes.py, and every case is
decidable -- no compared quantity within 1e-9 of its threshold, a strict winner among the four candidates wherever the case is not a tie on
purpose, at most 5 % of the rows outside the point comparison -- so that test_gpu_recover_pose.py may compare counts and mask bytes exactly.
A case that fails here gets another seed, never an exclusion."""
import numpy as np
import pytest

import recover_pose_oracle as RPO
import recover_pose_scenes as S

CASES = [(name, n) for name in S.MOTIONS for n in S.sizes(name)]


def _same(o, good, R, t, Q, m, what):
    assert good == o["n_good"], what
    assert R.tobytes() == o["R"].tobytes() and t.tobytes() == o["t"].tobytes(), what
    assert Q.tobytes() == o["Q"].tobytes(), what
    if m is not None:
        assert m.tobytes() == o["mask"].tobytes(), what


@pytest.mark.parametrize("name,n", CASES)
def test_restatement_equals_the_c_oracle(oracle, name, n):
    """Return value, R and t to the byte, mask bytes and Q bytes."""
    for variant in S.variants(name, n):
        scale, dist, coincident = variant
        p1, p2 = S.scene(name, n, coincident)
        for kind in S.MASKS:
            o = S.expected(oracle, name, n, variant, kind)
            _same(o, *oracle.recover_pose(S.E_of(name, scale), p1, p2, dist, S.mask(n, kind)), (variant, kind))
            assert o["n_good"] == (o["counts"][o["pick"]] if o["pick"] >= 0 else 0) == np.count_nonzero(o["mask"])


def _all_zero_is_expected(n, dist, m):
    """No row to test (n = 0, or an incoming mask without a nonzero byte: `zero`, `first256` up to 256 rows), or a single one (n = 1, or
    `first256` at 257 rows) at dist 9, which a scene 4 .. 12 deep need not pass."""
    live = n if m is None else int(np.count_nonzero(m))
    return live == 0 or (live == 1 and dist == 9.0)


@pytest.mark.parametrize("name,n", CASES)
def test_cases_are_decidable(oracle, name, n):
    for variant in S.variants(name, n):
        scale, dist, coincident = variant
        none = S.expected(oracle, name, n, variant, "none")
        assert none["margin"] > S.MARGIN, "pick another seed"
        assert np.count_nonzero(~S.comparable(none["Q"])) <= 0.05 * n, "pick another seed"
        for kind in S.MASKS:
            o, m = S.expected(oracle, name, n, variant, kind), S.mask(n, kind)
            top, second = sorted(o["counts"])[::-1][:2]
            if top == 0:
                assert _all_zero_is_expected(n, dist, m), "pick another seed"
                assert o["pick"] == 0 and o["n_good"] == 0
            else:
                assert top > second, "pick another seed"
            assert np.count_nonzero(~S.comparable(o["Q"])) <= 0.05 * n, "pick another seed"
            if m is not None:
                assert np.array_equal(o["mask"], m & none["masks"][o["pick"]])
        assert set(np.unique(S.expected(oracle, name, n, variant, "ones")["mask"])) <= {0, 1}
        if n >= 1000:
            f = S.expected(oracle, name, n, variant, "first256")
            assert not f["mask"][:256].any() and f["n_good"] > 0


def test_margin_and_excluded_share_of_the_committed_cases(oracle, capsys):
    """The figures the exact comparisons on the GPU rest on (printed; run with -s to see them)."""
    margin, share, picks = np.inf, 0.0, set()
    for name, n in CASES:
        for variant in S.variants(name, n):
            for kind in S.MASKS:
                o = S.expected(oracle, name, n, variant, kind)
                margin = min(margin, o["margin"])
                if n:
                    share = max(share, np.count_nonzero(~S.comparable(o["Q"])) / n)
                if max(o["counts"]) > 0:
                    picks.add(o["pick"])
    for tie in S.TIES:
        margin = min(margin, RPO.decide(S.cand(oracle, "forward", S.TIE_N, "pos"), S.tie_mask(oracle, tie)[0], 50.0)["margin"])
    for scale in S.TRANS_PICKS:
        for n in S.TRANS_SIZES:
            margin = min(margin, RPO.decide(S.cand(oracle, "norot", n, scale, translation=True), None, 50.0)["margin"])
    with capsys.disabled():
        print(f"\nrecover-pose cases: smallest margin {margin:.3e}, largest share of rows outside the point comparison {share:.4f}")
    assert margin > S.MARGIN and share <= 0.05
    assert picks == {0, 1, 2, 3}, "each candidate wins a case that is not a tie"


def test_motions_pick_every_candidate(oracle):
    """E / -E: 0 / 1 for the sideways, forward and rotation-free motions, 1 / 0 for the rolls of 90 and 170 degrees, 3 / 2 for the rest."""
    want = dict(side5=(0, 1), side05=(0, 1), forward=(0, 1), norot=(0, 1), roll90=(1, 0), roll170=(1, 0), backward=(3, 2), vertical=(3, 2),
                roll30=(3, 2), yaw20=(3, 2))
    for name in S.MOTIONS:
        for n in S.SHORT:
            got = tuple(S.expected(oracle, name, n, (scale, 50.0, False), "none")["pick"] for scale in ("pos", "neg"))
            assert got == want[name], (name, n)
    counts = S.expected(oracle, "forward", S.TIE_N, ("pos", 50.0, False), "none")["counts"]
    assert min(counts) > 0, "forward: all four candidates get points"


@pytest.mark.parametrize("tie", S.TIES, ids=str)
def test_tie_cases_are_tied(oracle, tie):
    base = S.expected(oracle, "forward", S.TIE_N, ("pos", 50.0, False), "none")
    assert not ((base["masks"] != 0).sum(0) > 1).any(), "every point is good under at most one candidate"
    assert [len(e) for e in S.exclusive(base["masks"])] == base["counts"]
    m, k = S.tie_mask(oracle, tie)
    p1, p2 = S.scene("forward", S.TIE_N)
    o = RPO.decide(S.cand(oracle, "forward", S.TIE_N, "pos"), m, 50.0)
    who = (0, 1, 2, 3) if tie == "all" else (3,) if tie == "only3" else tie
    assert k > 0 and o["counts"] == [k if c in who else 0 for c in range(4)], "the constructed counts are tied"
    assert o["pick"] == S.tie_expected_pick(tie) and o["n_good"] == k and o["margin"] > S.MARGIN
    _same(o, *oracle.recover_pose(S.E_of("forward", "pos"), p1, p2, 50.0, m), tie)


def test_norot_with_coincident_rows_is_not_decidable(oracle):
    """Why `norot` has no coincident variant: without a rotation the rays of p2 = p1 are parallel under every candidate and the predicates
    are decided by rounding."""
    n = 257
    p1, p2 = S.scene("norot", n, coincident=True)
    assert S.coincident_rows(n) > 0 and np.count_nonzero((p1 == p2).all(axis=1)) == S.coincident_rows(n)
    o = RPO.recover_pose(oracle, S.E_of("norot", "pos"), p1, p2, None, 50.0)
    assert o["margin"] < S.MARGIN
    assert all(v[2] is False for v in S.variants("norot", n)) and any(v[2] for v in S.variants("side5", n))


@pytest.mark.parametrize("n", S.TRANS_SIZES)
def test_translation_form_equals_the_c_oracle(oracle, n):
    for scale, pick in S.TRANS_PICKS.items():
        Et = S.E_of("norot", scale)
        p1, p2 = S.scene("norot", n)
        cand = S.cand(oracle, "norot", n, scale, translation=True)
        for kind in ("none", "half", "ones"):
            for dist in (50.0, 9.0):
                o = RPO.decide(cand, S.mask(n, kind), dist)
                _same(o, *oracle.recover_pose_translation(Et, p1, p2, dist, S.mask(n, kind)), (scale, kind, dist))
                assert o["margin"] > S.MARGIN and o["counts"][1] == o["counts"][3] == 0 and np.array_equal(o["R"], np.eye(3))
                if max(o["counts"]) > 0:
                    assert o["pick"] == pick and sorted(o["counts"])[-1] > sorted(o["counts"])[-2], "pick another seed"
        assert RPO.decide(cand, None, 50.0)["pick"] == pick
    m, k = S.tie_mask(oracle, (0, 2), "norot", translation=True)
    o = RPO.decide(S.cand(oracle, "norot", S.TIE_N, "pos", translation=True), m, 50.0)
    assert k > 0 and o["counts"] == [k, 0, k, 0] and o["pick"] == 0
    _same(o, *oracle.recover_pose_translation(S.E_of("norot", "pos"), *S.scene("norot", S.TIE_N), 50.0, m), "tie")


@pytest.mark.parametrize("kind", S.BATCH_MASKS)
def test_batch_problems_cover_every_pick(oracle, kind):
    assert max(S.BATCH_COUNTS) <= S.BATCH_STRIDE and len(S.BATCH_COUNTS) == len(S.BATCH_MOTIONS) == 8
    picks = set()
    for n, (name, scale) in zip(S.BATCH_COUNTS, S.BATCH_MOTIONS):
        o = S.expected(oracle, name, n, (scale, 50.0, False), kind)
        top, second = sorted(o["counts"])[::-1][:2]
        assert o["margin"] > S.MARGIN and (top > second or top == 0), "pick another seed"
        if top > 0:
            picks.add(o["pick"])
        p1, p2 = S.scene(name, n)
        _same(o, *oracle.recover_pose(S.E_of(name, scale), p1, p2, 50.0, S.mask(n, kind)), (name, n))
    assert picks == {0, 1, 2, 3}
