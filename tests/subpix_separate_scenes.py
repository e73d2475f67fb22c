"""Scenes shared by tests/test_oracle_subpix_separate.py and tests/test_gpu_subpix_separate.py, and their oracle results (computed once per
session).  Two checkerboards with known corners stand for an image pair with a large rotation between the views."""
import functools

import numpy as np

import subpix_separate_oracle as O

W, H = 320, 240
N_LIST = (0, 1, 2, 3, 5, 6, 7, 63, 64, 65, 257, 1025)
SCRAMBLES = (0.0, 0.7, 1.0)


@functools.lru_cache(maxsize=None)
def boards():
    from matchinglib_poselib_amd import synth

    return synth.corner_scene(W, H), synth.corner_scene(W, H, angle=-0.47, origin=(11.6, 3.2))


def oracle(s):
    return O.subpix(s["img1"], s["img2"], s["kp1"], s["kp2"], s.get("size1"), s.get("size2"))


def with_points(s, kp1, kp2, size1=None, size2=None):
    """the scene's images with other keypoints; size None = no size array"""
    kp1, kp2 = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2), np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
    out = dict(s, kp1=kp1, kp2=kp2)
    out["size1"] = None if size1 is None else np.ascontiguousarray(size1, np.float32)
    out["size2"] = None if size2 is None else np.ascontiguousarray(size2, np.float32)
    return out


def corner_points(n, seed=0, jitter=2.0, scramble=0.0, size1=9.5, size2=9.5):
    """n matched points on the two boards: corner i mod m of each, moved by up to `jitter` px a coordinate; a share `scramble` of the
    points 2 is moved by 2.7 to 3.3 px in BOTH coordinates instead: more than sqrt(12) from the corner, yet within a window of w >= 5"""
    b1, b2 = boards()
    rng = np.random.default_rng(977 * seed + n)
    t1 = b1["corners"][np.arange(n) % len(b1["corners"])]
    t2 = b2["corners"][(np.arange(n) * 7) % len(b2["corners"])]
    kp1 = t1 + rng.uniform(-jitter, jitter, (n, 2))
    kp2 = t2 + rng.uniform(-jitter, jitter, (n, 2))
    scr = np.zeros(n, bool)
    scr[rng.permutation(n)[: int(round(scramble * n))]] = True
    off = rng.uniform(2.7, 3.3, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    kp2[scr] = (t2 + off)[scr]
    s = with_points(dict(img1=b1["img"], img2=b2["img"]), kp1, kp2, None if size1 is None else np.full(n, size1), None if size2 is None else np.full(n, size2))
    return dict(s, truth1=t1.astype(np.float32), truth2=t2.astype(np.float32), scrambled=scr)


@functools.lru_cache(maxsize=None)
def corners(n, seed=0, jitter=2.0, scramble=0.0, size1=9.5, size2=9.5):
    s = corner_points(n, seed, jitter, scramble, size1, size2)
    return s, oracle(s)


@functools.lru_cache(maxsize=None)
def texture(n=200):
    """the smooth texture of the template-matching tests: no corners, most points wander off and are reset"""
    from matchinglib_poselib_amd import synth

    t = synth.subpix_scene("texture", n)
    s = with_points(t, t["kp1"], t["kp2"], np.full(n, 6.0), np.full(n, 6.0))
    return s, oracle(s)


@functools.lru_cache(maxsize=None)
def constant(n=6):
    rng = np.random.default_rng(3)
    img = np.full((H, W), 93, np.uint8)
    kp = rng.random((n, 2)) * np.array([W - 1.0, H - 1.0])
    s = with_points(dict(img1=img, img2=img.copy()), kp, kp[::-1].copy(), None, np.full(n, 6.0))
    return s, oracle(s)


def count_cases():
    return [(n, sc) for n in N_LIST for sc in SCRAMBLES]
