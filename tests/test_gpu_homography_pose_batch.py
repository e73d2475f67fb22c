"""GPU: mlpl_pose_homographies_batch_dev -- every problem of a batch is byte for byte what the single entry mlpl_pose_homographies_dev
returns for it alone with the same stream states: result code, R, t, E, inlier count and mask, planes, labels, the alignment's info
block and both stream states.  The alignment kernel and the final mask run MERGED over the cohort here and alone in the single entry,
so this is also the test that their results do not depend on how they were launched.  The batch mixes camera-unit and wide-field
scenes; it runs once per threshold, as tests/test_gpu_homography_batch.py does."""
import numpy as np
import pytest

import homography_pose_scenes as S
from homography_scenes import TH_CAM
from matchinglib_poselib_amd import MlplError, _lib, pose

pytestmark = pytest.mark.gpu

FRESH = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)
STRIDE = 520


def problems():
    """16 problems: 2- and 3-plane scenes of both units, one plane only (-3), no plane (-1), weak planes, fewer than 4 rows."""
    out = []
    for name in ("full_two", "full_three", "full_wide", "full_one", "full_weak"):
        sc = S.full_scene(name)
        out.append((sc["p1"], sc["p2"]))
    for counts, n_out, units, seed in (((150, 90), 60, "cam", 35), ((200, 120, 80), 100, "cam", 247), ((150, 90), 60, "wide", 30),
                                       ((120, 80), 40, "cam", 13), ((140, 100, 60), 80, "wide", 69), ((60, 40), 10, "cam", 35),
                                       ((100, 70), 330, "cam", 7)):
        sc = S.pose_scene(counts, n_out, seed, units, 1.0)
        out.append((sc["p1"], sc["p2"]))
    p1, p2, _ = S.noise_scene()
    out += [(p1, p2), (p1[:3], p2[:3]), (p1[:0], p2[:0]), (p1[:40], p2[:40])]
    assert len(out) == 16 and max(len(p[0]) for p in out) <= STRIDE
    return out


@pytest.mark.parametrize("th,check", [(TH_CAM, False), (S.TH_WIDE, False), (TH_CAM, True)])
def test_batch_equals_the_single_entry_by_bytes(ctx, th, check):
    import torch
    probs = problems()
    B = len(probs)
    counts = np.array([len(p[0]) for p in probs], np.int32)
    assert (counts < STRIDE).any() and (counts < 4).sum() >= 1
    h1, h2 = np.zeros((B, STRIDE, 2)), np.zeros((B, STRIDE, 2))
    for b, (p1, p2) in enumerate(probs):
        h1[b, :len(p1)], h2[b, :len(p2)] = p1, p2
    d1, d2 = torch.from_numpy(h1).cuda(), torch.from_numpy(h2).cuda()
    st = np.tile(FRESH, (B, 1))
    st[:, 0] += np.arange(B, dtype=np.uint64) * np.uint64(977)              # a different stream state per problem
    st_single = st.copy()
    masks = torch.full((B, STRIDE), 7, dtype=torch.uint8, device="cuda")
    labels = torch.full((B, STRIDE), -5, dtype=torch.int32, device="cuda")
    got = pose.pose_homographies_batch(d1, d2, counts, th, check_plane_strength=check, rng_states=st, masks_out=masks, labels_out=labels, ctx=ctx)
    masks, labels = masks.cpu().numpy(), labels.cpu().numpy()
    seen = set()
    for b in range(B):
        n = int(counts[b])
        g = got[b]
        if n < 1:       # the single entry refuses n < 1; the batch's answer for an empty problem is the reference's for no plane
            assert g["result"] == (-2 if check else -3) and st[b].tolist() == st_single[b].tolist() and (masks[b] == 7).all()
            continue
        o = pose.pose_homographies_device(d1[b, :n].contiguous(), d2[b, :n].contiguous(), th, check_plane_strength=check, rng_state=st_single[b], ctx=ctx)
        seen.add(o["result"])
        assert g["result"] == o["result"] and g["n_planes"] == o["n_planes"], b
        assert st[b].tobytes() == st_single[b].tobytes(), b
        for k in ("H", "num_inl", "strength", "info"):
            assert np.ascontiguousarray(g[k]).tobytes() == np.ascontiguousarray(o[k]).tobytes(), (b, k)
        if o["n_planes"] > 0:
            assert np.array_equal(labels[b, :n], o["labels"].cpu().numpy()), b
        if o["result"] == 0:
            for k in ("R", "t", "E"):
                assert g[k].tobytes() == o[k].tobytes(), (b, k)
            assert g["n_inliers"] == o["n_inliers"] and np.array_equal(masks[b, :n], o["mask"].cpu().numpy()), b
        else:
            assert (masks[b] == 7).all() and not g["R"].any() and not g["t"].any() and g["n_inliers"] == 0      # untouched
        assert (masks[b, n:] == 7).all()
    if th == TH_CAM:
        assert seen >= ({0, -1, -2, -3} if check else {0, -1, -3}), seen


def test_batch_malformed_calls(ctx):
    import torch
    d = torch.zeros((2, 8, 2), dtype=torch.float64, device="cuda")
    for counts, th in (([9, 3], 1e-3), ([-1, 3], 1e-3), ([4, 4], 0.0), ([4, 4], float("nan"))):
        st = np.tile(FRESH, (2, 1))
        with pytest.raises(MlplError) as e:
            pose.pose_homographies_batch(d, d, np.array(counts, np.int32), th, rng_states=st, ctx=ctx)
        assert e.value.code == _lib.MLPL_E_BAD_INPUT and st.tolist() == np.tile(FRESH, (2, 1)).tolist()
