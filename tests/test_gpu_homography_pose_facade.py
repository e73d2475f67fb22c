"""GPU: poselib::estimatePoseHomographies through the C++ drop-in (tests/cpp/homography_pose_facade.cpp) -- the reference's signature
and defaults, optional outputs omitted, -4 without R or t, the input-mask path, -3 with outputs untouched -- equals the C entry
mlpl_pose_homographies called with the same stream states."""
import os
import subprocess

import numpy as np
import pytest

import homography_pose_scenes as S
from matchinglib_poselib_amd import pose

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRESH = np.array(pose.ARRSAC_RNG_FRESH, np.uint64)


def test_cpp_facade_equals_the_c_entry(ctx, tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "homography_pose_facade")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    sc = S.full_scene("full_two")
    p1, p2, th = sc["p1"], sc["p2"], sc["th"]
    n = len(p1)
    mask_in = S.full_mask(n)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.int32(n).tobytes() + np.float64(th).tobytes() + p1.tobytes() + p2.tobytes() + mask_in.tobytes())
    subprocess.run([exe, str(inp), str(out)], check=True, timeout=120)
    buf = open(out, "rb").read()
    at = [0]

    def take(dtype, count=1):
        a = np.frombuffer(buf, dtype, count, at[0])
        at[0] += a.nbytes
        return a if count > 1 else a[0]

    st = FRESH.copy()
    g = pose.pose_homographies(p1, p2, th, rng_state=st, ctx=ctx)
    assert g["result"] == 0
    # A
    assert take(np.int32) == 0
    assert take(np.float64, 9).tobytes() == g["R"].tobytes() and take(np.float64, 3).tobytes() == g["t"].tobytes()
    assert take(np.float64, 9).tobytes() == g["E"].tobytes()
    assert take(np.int32) == g["n_inliers"] and np.array_equal(take(np.uint8, n), g["mask"])
    planes = take(np.int32)
    assert planes == g["n_planes"] >= 2                    # assigned: the element the vectors held before is gone
    for k in range(planes):
        assert take(np.uint32) == g["num_inl"][k] and take(np.float64) == g["strength"][k]
        assert take(np.float64, 9).tobytes() == g["H"][k].tobytes()
        assert take(np.int32) == (g["labels"] == k).sum() == g["num_inl"][k]
    assert take(np.uint64, 2).tolist() == st.tolist()
    # B
    assert take(np.int32) == 0 and take(np.float64, 9).tobytes() == g["R"].tobytes() and take(np.float64, 3).tobytes() == g["t"].tobytes()
    assert take(np.int32) == g["n_inliers"] and take(np.uint64, 2).tolist() == st.tolist()
    # C
    assert take(np.int32) == -4 and take(np.int32) == 1 and take(np.int32) == -4 and take(np.int32) == 1
    # D
    st_m = FRESH.copy()
    gm = pose.pose_homographies(p1, p2, th, mask=mask_in, rng_state=st_m, ctx=ctx)
    assert gm["result"] == 0
    assert take(np.int32) == 0 and take(np.float64, 9).tobytes() == gm["R"].tobytes() and take(np.float64, 3).tobytes() == gm["t"].tobytes()
    assert take(np.int32) == gm["n_inliers"] and np.array_equal(take(np.uint8, n), gm["mask"]) and take(np.uint64, 2).tolist() == st_m.tolist()
    # E
    assert take(np.int32) == -3 and take(np.int32) == 1
    assert at[0] == len(buf)
