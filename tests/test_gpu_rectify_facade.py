"""GPU: the C++ drop-in of the stereo rectification (include/matchinglib_poselib/pose_helper.h) through tests/cpp/rectify_facade.cpp: the
reference's signatures and defaults, the same bytes as the C entries and the restatement, the refusals, and the extension names."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rectify_oracle as O
import rectify_scenes as S
from matchinglib_poselib_amd import pose

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_EXE = os.path.join(ROOT, "tests", "cpp", "rectify_facade")


class Reader:
    def __init__(self, blob):
        self.blob, self.pos = blob, 0

    def take(self, dtype, n, shape=None):
        a = np.frombuffer(self.blob, dtype, n, self.pos)
        self.pos += a.nbytes
        return a if shape is None else a.reshape(shape)

    def i32(self):
        return int(self.take(np.int32, 1)[0])


def run_facade(tmp_path, name, step):
    assert os.path.exists(FACADE_EXE), "run __graft_entry__.build() first"
    s = S.SCENES[name]
    w, h = s["size"]
    imgs = []
    for seed in (6, 7):
        buf = np.full((h, step), 255, np.uint8)
        buf[:, :w] = S.image(w, h, seed)
        imgs.append(buf)
    d1 = np.zeros(0) if s["dist1"] is None else np.asarray(s["dist1"], np.float64)
    d2 = np.zeros(0) if s["dist2"] is None else np.asarray(s["dist2"], np.float64)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<8i", w, h, step, s["new_size"][0], s["new_size"][1], d1.size, d2.size, 0))
        f.write(struct.pack("<d", s["alpha"]))
        for k in ("R", "t", "K1", "K2"):
            f.write(np.ascontiguousarray(s[k], np.float64).tobytes())
        f.write(d1.tobytes() + d2.tobytes() + imgs[0].tobytes() + imgs[1].tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "matchinglib_poselib_amd", "lib") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([FACADE_EXE, str(fin), str(fout)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout
    rd = Reader(open(fout, "rb").read())
    out = dict(text=r.stdout, imgs=[b[:, :w] for b in imgs])
    out["rc_full"] = rd.i32()
    for k, shape in (("Rect1", (3, 3)), ("Rect2", (3, 3)), ("K1new", (3, 3)), ("K2new", (3, 3)), ("P1", (3, 4)), ("P2", (3, 4))):
        out[k] = rd.take(np.float64, shape[0] * shape[1], shape)
    out["roi1"], out["roi2"] = list(rd.take(np.int32, 4)), list(rd.take(np.int32, 4))
    out["rc_default"] = rd.i32()
    out["default"] = [rd.take(np.float64, 9, (3, 3)) for _ in range(3)]
    out["rc_false"], out["untouched"] = rd.i32(), rd.i32()
    ow, oh = rd.i32(), rd.i32()
    out["out_size"] = (ow, oh)
    out["maps"] = [rd.take(np.float32, ow * oh, (oh, ow)) for _ in range(4)]
    out["rc_get"] = rd.i32()
    out["get"] = [rd.take(np.uint8, ow * oh, (oh, ow)) for _ in range(2)]
    out["rc_fused"] = rd.i32()
    out["fused"] = [rd.take(np.uint8, ow * oh, (oh, ow)) for _ in range(2)]
    out["refused"] = list(rd.take(np.int32, 4))
    assert rd.pos == len(rd.blob)
    return out


@pytest.mark.parametrize("name,step", [("small", 112), ("small_resized", 97), ("vertical", 64)])
def test_cpp_facade(ctx, tmp_path, name, step):
    s, o = S.SCENES[name], S.oracle_parameters(name)
    g = run_facade(tmp_path, name, step)
    # ---- the parameters: the C entry's doubles, bit for bit
    c = pose.rectification_parameters(*S.call_args(name))
    assert g["rc_full"] == 0
    for k, ck in (("Rect1", "Rect1"), ("Rect2", "Rect2"), ("K1new", "Knew"), ("K2new", "Knew"), ("P1", "P1"), ("P2", "P2")):
        assert g[k].tobytes() == c[ck].tobytes(), k
    assert g["roi1"] == c["roi"] == o["roi"] and g["roi2"] == [7, 7, 7, 7]       # the reference never writes roi2 on this branch
    # ---- the defaults: alpha = -1, globRectFunct = true, newImgSize = Size()
    d = pose.rectification_parameters(s["R"], s["t"], s["K1"], s["K2"], s["dist1"], s["dist2"], s["size"])
    assert g["rc_default"] == 0 and all(a.tobytes() == d[k].tobytes() for a, k in zip(g["default"], ("Rect1", "Rect2", "Knew")))
    assert d["info"][3] == 1.0
    # ---- globRectFunct = false: -1, a message, nothing written
    assert g["rc_false"] == -1 and g["untouched"] == 1 and "stereoRectify2" in g["text"] and "not built" in g["text"]
    # ---- maps and images: the restatement's, and the fused extension equals them
    w, h = S.out_size(name)
    assert g["out_size"] == (w, h)
    for side in (0, 1):
        ox, oy = S.oracle_maps(name, side)
        assert g["maps"][2 * side].tobytes() == ox.tobytes() and g["maps"][2 * side + 1].tobytes() == oy.tobytes()
        want = O.remap(g["imgs"][side], ox, oy)
        assert g["rc_get"] == 0 and g["get"][side].tobytes() == want.tobytes()
        assert g["rc_fused"] == 0 and g["fused"][side].tobytes() == want.tobytes()
        assert want.any()
    # ---- refused types: a CV_32F image (twice), CV_64F maps, a map type other than CV_32FC1
    assert g["refused"] == [-1, -1, -1, 1]


def test_facade_header_names():
    text = open(os.path.join(ROOT, "include", "matchinglib_poselib", "pose_helper.h")).read()
    for name in ("getRectificationParameters", "GetRectifiedImages", "initUndistortRectifyMap", "rectifyImages"):
        assert f" {name}(" in text
    assert "double alpha = -1, bool globRectFunct = true" in text and "const cv::Size &newImgSize = cv::Size()" in text
    assert "cv::Rect *roi1 = nullptr, cv::Rect *roi2 = nullptr" in text and text.count("cv::noArray()") >= 2
    assert "struct Rect" in open(os.path.join(ROOT, "include", "matchinglib_poselib", "cv_compat.h")).read()
