"""refineEssentialLinear with PR_KNEIP on the MI355X (mlpl_refine_essential_linear_rt, its batch form and the C++ drop-in) against the
float64 restatement in kneip_refine_oracle.py.  The device accumulates the solver's summation terms with the bits of the host's
dgm::eig_sums and the solve itself is the same host code, so everything -- R, t and E included -- is compared to the bit; the scenes keep
every evaluated error well away from its threshold (`margin`)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import kneip_refine_oracle as KRO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "kneip_refine_facade")
SIZES = (6, 64, 65, 300)  # one chunk of the sums kernel not full, exactly full, one entry over, several
MARGIN = 1e-6             # relative; rounding differences of an error are ~1e-15

_scenes, _oracle = {}, {}


def _scene(key):
    """key = (n_list, seed, keyword pairs of KRO.make_scene)"""
    if key not in _scenes:
        _scenes[key] = KRO.make_scene(key[0], seed=key[1], **dict(key[2:]))
    return _scenes[key]


def _ora(key, method, with_R, seed, mask=None, R=None, **kw):
    k = (key, method, with_R, seed, None if mask is None else mask.tobytes(), None if R is None else R.tobytes(), tuple(sorted(kw.items())))
    if k not in _oracle:
        p1, p2, E0, m0, Rt, th = _scene(key)
        _oracle[k] = KRO.refine_essential_linear_rt(p1, p2, E0, m0 if mask is None else mask, method, R=(Rt if R is None else R) if with_R else None,
                                                    th=th, seed=seed, **kw)
    return _oracle[k]


def _single(ctx, p1, p2, E, mask, method, R, th, seed, **kw):
    from matchinglib_poselib_amd import pose

    return pose.refine_essential_linear_rt(p1, p2, E, mask, method, R=R, th=th, seed=seed, ctx=ctx, **kw)


def _equal_to_oracle(g, o, E0, m0):
    assert g["ok"] == (o["rc"] == 0)
    assert g["attempts_used"] == o["attempts_used"]
    if not g["ok"]:
        assert g["E"].tobytes() == np.asarray(E0, np.float64).tobytes() and g["mask"].tobytes() == np.asarray(m0, np.uint8).tobytes()
        return
    assert g["steps_done"] == o["steps_done"] and g["n_inliers"] == o["n_inliers"] and g["rt_valid"] == o["rt_valid"]
    assert g["mask"].tobytes() == o["mask"].tobytes()
    assert g["E"].tobytes() == o["E"].tobytes()
    if o["rt_valid"]:
        assert g["R"].tobytes() == o["R"].tobytes() and g["t"].tobytes() == o["t"].tobytes()
    else:
        assert g["R"] is None and g["t"] is None


@pytest.mark.parametrize("with_R", (True, False), ids=("start", "retry"))
@pytest.mark.parametrize("method", (0x04, 0x24))
@pytest.mark.parametrize("n_list", SIZES)
def test_single_equals_restatement(ctx, n_list, method, with_R):
    key = (n_list, 41)
    p1, p2, E0, m0, Rt, th = _scene(key)
    o = _ora(key, method, with_R, seed=n_list + 3)
    assert o["rc"] == 0 and o["steps_done"] >= 1 and o["rt_valid"] and o["margin"] > MARGIN, "pick another scene"
    g = _single(ctx, p1, p2, E0, m0, method, Rt if with_R else None, th, n_list + 3)
    _equal_to_oracle(g, o, E0, m0)
    assert (g["attempts_used"] == 0) == with_R


def test_several_attempts_and_no_steps(ctx):
    key = (150, 44, ("rot_deg", 25.0))
    p1, p2, E0, m0, Rt, th = _scene(key)
    o = _ora(key, 0x24, False, seed=44)
    assert o["rc"] == 0 and o["attempts_used"] > 1 and o["margin"] > MARGIN
    _equal_to_oracle(_single(ctx, p1, p2, E0, m0, 0x24, None, th, 44), o, E0, m0)
    # another seed, other starts
    o2 = _ora(key, 0x24, False, seed=45)
    assert o2["margin"] > MARGIN
    _equal_to_oracle(_single(ctx, p1, p2, E0, m0, 0x24, None, th, 45), o2, E0, m0)
    # no steps: true, the mask made 0 / 1, no pose; fewer than 6 flagged: false
    m7 = (m0 * 7).astype(np.uint8)
    o = _ora(key, 0x24, True, seed=1, mask=m7, steps=0)
    g = _single(ctx, p1, p2, E0, m7, 0x24, Rt, th, 1, num_iterative_steps=0)
    assert o["rc"] == 0 and not o["rt_valid"]
    _equal_to_oracle(g, o, E0, m7)
    few = np.zeros_like(m0)
    few[np.flatnonzero(m0)[:5]] = 1
    for steps in (0, 4):
        g = _single(ctx, p1, p2, E0, few, 0x24, Rt, th, 1, num_iterative_steps=steps)
        assert not g["ok"] and g["mask"].tobytes() == few.tobytes() and g["E"].tobytes() == E0.tobytes()


def _ragged_batch():
    """Six problems, stride 400 > every count: a plain one; fewer than 6 inliers; one that loses too many at step 0; a retry problem that
    needs several attempts; a mask with values other than 0 / 1 and a passed R that is no rotation; twelve failed attempts."""
    stride, rng = 400, np.random.default_rng(5)
    probs = []
    p1, p2, E0, m0, Rt, th = _scene((300, 42))
    probs.append(dict(p1=p1, p2=p2, E=E0, m=m0, R=Rt, valid=1, th=th, seed=1))
    few = np.zeros_like(m0)
    few[np.flatnonzero(m0)[:5]] = 1
    probs.append(dict(p1=p1, p2=p2, E=E0, m=few, R=Rt, valid=1, th=th, seed=2))
    q1, q2, F0, _, Rq, thq = _scene((120, 43, ("extra", 1.0)))
    probs.append(dict(p1=q1, p2=q2, E=F0, m=np.ones(q1.shape[0], np.uint8), R=Rq, valid=1, th=thq, seed=3))
    r1, r2, G0, mr, Rr, thr = _scene((150, 44, ("rot_deg", 25.0)))
    probs.append(dict(p1=r1, p2=r2, E=G0, m=mr, R=np.zeros((3, 3)), valid=0, th=thr, seed=44))
    s1, s2, H0, ms, Rs, ths = _scene((65, 41))
    probs.append(dict(p1=s1, p2=s2, E=H0, m=(ms * 7).astype(np.uint8), R=2.0 * np.eye(3), valid=1, th=ths, seed=9))
    u1, u2 = rng.uniform(-0.4, 0.4, (200, 2)), rng.uniform(-0.4, 0.4, (200, 2))
    probs.append(dict(p1=u1, p2=u2, E=KRO.essential_from_pose(np.eye(3), [1.0, 0, 0]), m=(rng.random(200) < 0.7).astype(np.uint8), R=np.zeros((3, 3)),
                      valid=0, th=0.001, seed=6))
    return stride, probs


def test_ragged_batch_equals_single(ctx):
    import torch
    from matchinglib_poselib_amd import pose

    stride, probs = _ragged_batch()
    B = len(probs)
    P1, P2, M = np.zeros((B, stride, 2)), np.zeros((B, stride, 2)), np.full((B, stride), 5, np.uint8)
    for b, q in enumerate(probs):
        n = q["p1"].shape[0]
        assert n < stride
        P1[b, :n], P2[b, :n], M[b, :n] = q["p1"], q["p2"], q["m"]
    counts = np.array([q["p1"].shape[0] for q in probs], np.int32)
    E = np.stack([q["E"].reshape(9) for q in probs])
    R = np.stack([q["R"].reshape(9) for q in probs])
    valid = np.array([q["valid"] for q in probs], np.int32)
    d1, d2, dm = torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda(), torch.from_numpy(M).cuda()
    res = pose.refine_essential_linear_rt_batch(d1, d2, counts, E, dm, [q["th"] for q in probs], 0x24, R=R, rt_valid=valid,
                                                seeds=[q["seed"] for q in probs], ctx=ctx)
    torch.cuda.synchronize()
    masks = dm.cpu().numpy()
    kinds = []
    for b, q in enumerate(probs):
        n = counts[b]
        g = _single(ctx, q["p1"], q["p2"], q["E"], q["m"], 0x24, q["R"] if q["valid"] else None, q["th"], q["seed"])
        assert (res["status"][b] == 0) == g["ok"]
        assert res["E"][b].tobytes() == g["E"].tobytes() and masks[b, :n].tobytes() == g["mask"].tobytes()
        assert res["n_inliers"][b] == g["n_inliers"] and res["steps_done"][b] == g["steps_done"] and res["attempts_used"][b] == g["attempts_used"]
        assert masks[b, n:].tobytes() == M[b, n:].tobytes()
        if g["ok"]:
            assert bool(res["rt_valid"][b]) == g["rt_valid"]
            if g["rt_valid"]:
                assert res["R"][b].tobytes() == g["R"].tobytes() and res["t"][b].tobytes() == g["t"].tobytes()
        if not g["ok"] or not g["rt_valid"]:  # nothing of the pose is touched
            assert res["R"][b].reshape(9).tobytes() == R[b].tobytes() and not res["t"][b].any()
        if not g["ok"]:
            assert res["E"][b].reshape(9).tobytes() == E[b].tobytes() and masks[b, :n].tobytes() == q["m"].tobytes() and res["rt_valid"][b] == valid[b]
        kinds.append(("failed" if not g["ok"] else "refined" if g["steps_done"] else "unchanged", g["attempts_used"]))
    assert [k for k, _ in kinds] == ["refined", "failed", "failed", "refined", "refined", "unchanged"], kinds
    assert kinds[3][1] > 1 and kinds[4][1] >= 1 and kinds[5][1] == 12 and kinds[0][1] == 0
    # the single results above are the restatement's
    for b in (0, 3, 4, 5):
        q = probs[b]
        o = KRO.refine_essential_linear_rt(q["p1"], q["p2"], q["E"], q["m"], 0x24, R=q["R"] if q["valid"] else None, th=q["th"], seed=q["seed"])
        assert o["margin"] > MARGIN
        assert res["E"][b].tobytes() == o["E"].tobytes() and masks[b, :counts[b]].tobytes() == o["mask"].tobytes()


def test_other_solvers_through_the_new_entries(ctx):
    """0x21 through the new entries is the existing kernel: equal to the existing entries to the bit, rt_valid cleared, R and t untouched."""
    import torch
    from matchinglib_poselib_amd import pose

    p1, p2, E0, m0, Rt, th = _scene((300, 42))
    ref = pose.refine_essential_linear(p1, p2, E0, m0, 0x21, th=th, ctx=ctx)
    g = _single(ctx, p1, p2, E0, m0, 0x21, Rt, th, 1)
    assert ref["ok"] and g["ok"] and ref["steps_done"] >= 1 and not g["rt_valid"] and g["attempts_used"] == 0
    assert g["E"].tobytes() == ref["E"].tobytes() and g["mask"].tobytes() == ref["mask"].tobytes()
    assert g["n_inliers"] == ref["n_inliers"] and g["steps_done"] == ref["steps_done"]
    n = p1.shape[0]
    d1, d2 = torch.from_numpy(p1[None].copy()).cuda(), torch.from_numpy(p2[None].copy()).cuda()
    dm = torch.from_numpy(m0[None].copy()).cuda()
    res = pose.refine_essential_linear_rt_batch(d1, d2, [n], E0.reshape(1, 9), dm, th, 0x21, R=Rt.reshape(1, 9), ctx=ctx)
    torch.cuda.synchronize()
    assert res["status"][0] == 0 and res["rt_valid"][0] == 0 and res["R"][0].tobytes() == Rt.tobytes() and not res["t"].any()
    assert res["E"][0].tobytes() == ref["E"].tobytes() and dm.cpu().numpy()[0].tobytes() == ref["mask"].tobytes()


def test_facade(ctx, tmp_path):
    assert os.path.exists(FACADE_EXE), "built by the facade Makefile's check target"
    p1, p2, E0, m0, Rt, th = _scene((150, 44, ("rot_deg", 25.0)))
    n, seed = p1.shape[0], 44
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<idI", n, th, seed) + p1.tobytes() + p2.tobytes() + np.asarray(E0, np.float64).tobytes() + m0.astype(np.uint8).tobytes()
                    + np.ascontiguousarray(Rt, np.float64).tobytes())
    subprocess.run([FACADE_EXE, str(src), str(dst)], check=True, timeout=120)
    raw = dst.read_bytes()
    recs, at = [], 0
    for _ in range(3):
        ok, nr = struct.unpack_from("<iq", raw, at)
        at += 12
        E = np.frombuffer(raw, np.float64, 9, at)
        at += 72
        mask = np.frombuffer(raw, np.uint8, n, at)
        at += n
        (r_empty,) = struct.unpack_from("<i", raw, at)
        at += 4
        rt = np.frombuffer(raw, np.float64, 12, at)
        at += 96
        recs.append((ok, nr, E, mask, r_empty, rt))
    assert at == len(raw)
    with_R = _single(ctx, p1, p2, E0, m0, 0x24, Rt, th, 1)
    retry = _single(ctx, p1, p2, E0, m0, 0x24, 2.0 * np.eye(3), th, seed)
    assert with_R["ok"] and with_R["rt_valid"] and retry["ok"] and retry["rt_valid"] and retry["attempts_used"] > 1
    for (ok, nr, E, mask, r_empty, rt), g in zip(recs, (with_R, retry, retry)):
        assert bool(ok) and nr == g["n_inliers"] and not r_empty
        assert E.tobytes() == g["E"].tobytes() and mask.tobytes() == g["mask"].tobytes()
        assert rt[:9].tobytes() == g["R"].tobytes() and rt[9:].tobytes() == g["t"].tobytes()
    assert raw[len(raw) // 3:2 * len(raw) // 3] == raw[2 * len(raw) // 3:], "the same seed, the same result"
