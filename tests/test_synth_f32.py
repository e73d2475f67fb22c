"""CPU-only: the float-descriptor image pair generator (synth.stereo_pair_f32) against the oracle pipeline, and the float entries of the
C ABI (mlpl_match_l2_dev, the four mlpl_pair_pose*_f32_dev) in the library and in the ctypes table.  No compute call on a device.
Reference: the CV_32F half of getMatches "LINEAR", matchinglib/source/matchers.cpp:632-707."""
import ctypes

import numpy as np
import pytest

import matchinglib_poselib_amd as mpa
from matchinglib_poselib_amd import _lib, synth

F32_ENTRIES = ("mlpl_match_l2_dev", "mlpl_pair_pose_f32_dev", "mlpl_pair_pose_batch_f32_dev", "mlpl_pair_pose_batch_usac_f32_dev",
               "mlpl_pair_pose_batch_arrsac_f32_dev")


def _cam(p, K):
    return np.stack([((p[:, 0].astype(np.float64) - K[2]) / K[0]).astype(np.float32),
                     ((p[:, 1].astype(np.float64) - K[3]) / K[1]).astype(np.float32)], axis=1).astype(np.float64)


@pytest.mark.parametrize("rootsift", [False, True])
def test_generator_is_deterministic_and_the_oracle_pipeline_recovers_the_pose(oracle, rootsift):
    """Same seed, same bytes; the dict has stereo_pair's keys; on a 2048-keypoint pair with 30 % unmatched queries the ratio test keeps at
    least 95 % of the true neighbours and at most 1 % of the unmatched queries, and get_matches_linear -> ImgToCamCoordTrans ->
    ransac_essential -> recover_pose returns the ground-truth rotation."""
    n, seed = 2048, 20260400
    a = synth.stereo_pair_f32(n, seed, unmatched_frac=0.3, rootsift=rootsift)
    b = synth.stereo_pair_f32(n, seed, unmatched_frac=0.3, rootsift=rootsift)
    assert set(a) == set(synth.stereo_pair(64, seed=1))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    c = synth.stereo_pair_f32(n, seed + 1, unmatched_frac=0.3, rootsift=rootsift)
    assert a["desc1"].tobytes() != c["desc1"].tobytes()
    assert a["desc1"].dtype == np.float32 and a["desc1"].shape == (n, 128) and a["desc2"].shape == (n, 128) and a["kp1"].dtype == np.float32
    integer = bool(np.all(a["desc1"] == np.rint(a["desc1"])) and np.all(a["desc2"] == np.rint(a["desc2"])))
    assert integer == (not rootsift)    # RootSIFT rows are not integer-valued: the exact / fp16 paths, not the int8 one
    if rootsift:
        assert np.allclose((a["desc2"].astype(np.float64) ** 2).sum(1), 1.0, atol=1e-5)

    rc, mm = oracle.get_matches_linear(n, n, a["desc1"], a["desc2"])
    assert rc == 0
    truth = a["train_of_query"]
    right = mm["trainIdx"] == truth[mm["queryIdx"]]
    # the unmatched queries: rows far from their true neighbour in the integer-valued form of the same pair (same seed, same stream; a
    # perturbed row is ~sqrt(128) * 6 = 68 away from its neighbour, a fresh row several hundred)
    base = a if not rootsift else synth.stereo_pair_f32(n, seed, unmatched_frac=0.3)
    gap = np.linalg.norm(base["desc1"].astype(np.float64) - base["desc2"][truth].astype(np.float64), axis=1)
    lost = gap > 200.0
    assert 0.2 * n < lost.sum() < 0.4 * n and gap[~lost].max() < 120.0
    n_true = int((~lost).sum())
    kept_true = int((right & ~lost[mm["queryIdx"]]).sum())
    kept_lost = int(lost[mm["queryIdx"]].sum())
    print(f"rootsift={rootsift}: {len(mm)} matches, {kept_true} of {n_true} true neighbours kept, {kept_lost} of {int(lost.sum())} unmatched kept")
    assert kept_true >= 0.95 * n_true
    assert kept_lost <= 0.01 * lost.sum()

    K = a["K"]
    p1, p2 = _cam(a["kp1"][mm["queryIdx"]], K), _cam(a["kp2"][mm["trainIdx"]], K)
    th = 0.8 * 4.0 / (np.sqrt(2.0) * (2 * K[0] + 2 * K[1]))
    o = oracle.ransac_essential(p1, p2, th, seed=7)
    assert o["ok"] and o["n_inliers"] >= 0.4 * len(mm)
    good, R, t, Q, mk = oracle.recover_pose(o["E"], p1, p2, 50.0, o["mask"])
    assert good > 0
    ang = np.degrees(np.arccos(np.clip((np.trace(R @ a["R"].T) - 1) / 2, -1, 1)))
    tt = np.asarray(t).ravel()
    tang = np.degrees(np.arccos(np.clip(abs(tt @ a["t"]) / np.linalg.norm(tt), -1, 1)))
    print(f"rotation error {ang:.4f} deg, translation direction error {tang:.4f} deg")
    # The model is RANSAC's best MINIMAL sample (no refit) at a 0.8 px threshold: its rotation is good to a few threshold widths over the
    # image (0.8 px at f = 800 is 0.06 deg per point), not to the noise floor.  1 deg against the scene's 5 deg rotation still tells the
    # true pose from any other decomposition candidate (those differ by the full rotation or a half turn); t is a direction, 5 deg likewise.
    assert ang < 1.0 and tang < 5.0


def test_float_entries_are_exported_and_bound():
    lib = ctypes.CDLL(mpa.library_path())
    for name in F32_ENTRIES + ("mlpl_debug_last_l2_match",):
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES, name
    # the f32 pair entries take what their uint8 forms take (`dim` floats per row where those have `nbytes` bytes)
    for name in F32_ENTRIES[1:]:
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[name.replace("_f32", "")], name
    assert _lib._SIGNATURES["mlpl_match_l2_dev"] == _lib._SIGNATURES["mlpl_match_hamming_dev"]
    from matchinglib_poselib_amd import matching
    assert callable(matching.match_l2_device)
