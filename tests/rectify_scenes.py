"""Scenes shared by tests/test_oracle_rectify.py, tests/test_gpu_rectify.py and tests/test_gpu_rectify_facade.py, and their oracle results
(computed once per process and handed out unchanged)."""
import functools
import math

import numpy as np

import rectify_oracle as O


def rodrigues(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


_SMALL = dict(size=(97, 61), K1=np.array([[90, 0, 47.5], [0, 92, 30.2], [0, 0, 1.0]]), K2=np.array([[88, 0, 49], [0, 89, 29], [0, 0, 1.0]]),
              R=rodrigues((0.2, 0.9, 0.1), 4.0), t=_unit((-0.98, 0.05, 0.12)), dist1=np.array([-0.12, 0.03, 1e-3, -5e-4, 0.002]),
              dist2=np.array([-0.1, 0.02, -8e-4, 6e-4, 0, 0.01, 0.002, 5e-4]), alpha=0.2, new_size=(0, 0))

SCENES = {
    # takes the dk1 < 0 focal-length branch
    "small": _SMALL,
    # a second output size: newImgSize differs from the image size
    "small_resized": dict(_SMALL, new_size=(80, 50)),
    "kitti": dict(size=(1242, 375), K1=np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1.0]]),
                  K2=np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]]), R=rodrigues((0.1, 1.0, 0.3), 1.5),
                  t=_unit((-0.999, 0.012, 0.02)), dist1=None, dist2=None, alpha=0.2, new_size=(0, 0)),
    # idx = 1: |t.y| > |t.x|; default scaling; the inner rectangle comes out negative, as the reference's own comment predicts
    "vertical": dict(size=(64, 80), K1=np.array([[70, 0, 31.2], [0, 71, 40.3], [0, 0, 1.0]]), K2=np.array([[69, 0, 32.4], [0, 70, 39.1], [0, 0, 1.0]]),
                     R=rodrigues((0.8, 0.1, 0.3), 3.0), t=_unit((0.05, -0.99, 0.03)), dist1=np.array([-0.05, 0.01, 0, 0]),
                     dist2=np.array([-0.04, 0.0, 1e-4, -1e-4]), alpha=-1.0, new_size=(0, 0)),
    # k1 = -1.5: the image corners (normalised radius 0.63) have no preimage, the distortion's maximum is 0.31 and 0.63 - 0.31 > 0.25: the
    # reduction loops run, and all four run to reduction >= 0.25 (24 steps) and take the coefficient-free pass; s is clamped to 1
    "strong": dict(_SMALL, dist1=np.array([-1.5, 0, 0, 0, 0.0]), dist2=np.array([-1.5, 0, 0, 0, 0.0])),
    # k1 = -0.9: the loops run and end on their own (14, 18, 14 and 16 steps); s = 1.70 stays inside [0.5, 2]
    "strong_partial": dict(_SMALL, dist1=np.array([-0.9, 0, 0, 0, 0.0]), dist2=np.array([-0.9, 0, 0, 0, 0.0])),
}


def call_args(name):
    s = SCENES[name]
    return (s["R"], s["t"], s["K1"], s["K2"], s["dist1"], s["dist2"], s["size"], s["alpha"], s["new_size"])


@functools.lru_cache(maxsize=None)
def oracle_parameters(name, inverse="cof"):
    return O.parameters(*call_args(name), inverse=inverse)


def out_size(name):
    s = SCENES[name]
    return s["size"] if s["new_size"][0] * s["new_size"][1] == 0 else s["new_size"]


@functools.lru_cache(maxsize=None)
def oracle_maps(name, side, width=None, height=None):
    """the restatement's maps of image `side` (0 / 1) of a scene at its output size (or the one given)"""
    s, p = SCENES[name], oracle_parameters(name)
    w, h = out_size(name)
    w, h = (w if width is None else width), (h if height is None else height)
    mx, my = O.maps(s["K1" if side == 0 else "K2"], s["dist1" if side == 0 else "dist2"], p["Rect1" if side == 0 else "Rect2"], p["Knew"], w, h)
    mx.setflags(write=False)
    my.setflags(write=False)
    return mx, my


def map_args(name, side):
    s, p = SCENES[name], oracle_parameters(name)
    return (s["K1" if side == 0 else "K2"], s["dist1" if side == 0 else "dist2"], p["Rect1" if side == 0 else "Rect2"], p["Knew"])


@functools.lru_cache(maxsize=None)
def image(width, height, seed):
    """a textured 8-bit image: smooth blobs plus noise, every grey level in reach"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    v = 120 + 60 * np.sin(x / 5.3 + seed) * np.cos(y / 4.1) + 40 * np.sin((x + 2 * y) / 9.0) + rng.normal(0, 12, (height, width))
    img = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def hostile_maps(width, height, out_w=40, out_h=9):
    """map values that must never reach an address: NaN, infinities, huge values, the borders, exact ties of the x 32 rounding"""
    special = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.5, width - 1.0, width - 0.5, -1e-3, 3e9, -3e9, 2147483648.0 / 32, -2147483648.0 / 32,
               67108860.0, -67108864.0, 1e-45, 32767.5, -32768.5, 16384.0, 1e9]
    ties = [k + 1 / 64 for k in (0, 1, 2, 5, 10)] + [k + 3 / 64 for k in (0, 3, 7)] + [-1 + 1 / 64, -1 / 64]
    vals = np.array(special + ties, np.float32)
    rng = np.random.default_rng(11)
    mx = rng.uniform(-2, width + 1, (out_h, out_w)).astype(np.float32)
    my = rng.uniform(-2, height + 1, (out_h, out_w)).astype(np.float32)
    n = len(vals)
    mx[0, :n] = vals                                      # hostile x, ordinary y
    my[1, :n] = vals                                      # hostile y, ordinary x
    mx[2, :n] = vals                                      # both
    my[2, :n] = vals[::-1]
    mx[3, :n] = vals
    my[3, :n] = np.float32(height - 1)                    # the last row: the tap below is outside
    mx[4, :] = np.float32(width - 1)                      # the last column: the tap to the right is outside
    return mx, my
