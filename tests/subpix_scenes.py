"""Scenes shared by tests/test_oracle_subpix.py and tests/test_gpu_subpix.py, and their oracle results (computed once per session)."""
import functools

import numpy as np

import subpix_oracle as O

W, H = 320, 240
ROUNDING_SEEDS = (1, 3, 5)     # chosen with the oracle: each holds inliers whose float32 first minimum is not the exact-integer minimum
N_LIST = (0, 1, 2, 3, 5, 6, 7, 63, 64, 65, 257, 1025)


def oracle(s, tables=False):
    return O.subpix(s["img1"], s["img2"], s["kp1"], s["kp2"], s.get("size1"), s.get("size2"), tables=tables)


@functools.lru_cache(maxsize=None)
def texture(n, seed=0, scramble=0.0, noise=0.0, side=0.0):
    from matchinglib_poselib_amd import synth

    s = synth.subpix_scene("texture", n, seed=seed, width=W, height=H, scramble=scramble, noise=noise, side=side)
    return s, oracle(s, tables=True)


@functools.lru_cache(maxsize=None)
def rounding(seed):
    from matchinglib_poselib_amd import synth

    s = synth.subpix_scene("rounding", 8, seed=seed)
    return s, oracle(s, tables=True)


@functools.lru_cache(maxsize=None)
def constant(n=6):
    from matchinglib_poselib_amd import synth

    s = synth.subpix_scene("constant", n, width=W, height=H)
    return s, oracle(s, tables=True)


def count_cases():
    """(n, scramble) pairs of the list-length test: every n with all keypoints good, with 70 % and with all of them scrambled"""
    return [(n, sc) for n in N_LIST for sc in (0.0, 0.7, 1.0)]


def with_points(s, kp1, kp2, size1=None, size2=None):
    """the scene's images with other keypoints"""
    kp1, kp2 = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2), np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
    n = len(kp1)
    out = dict(s, kp1=kp1, kp2=kp2)
    out["size1"] = np.zeros(n, np.float32) if size1 is None else np.ascontiguousarray(size1, np.float32)
    out["size2"] = np.zeros(n, np.float32) if size2 is None else np.ascontiguousarray(size2, np.float32)
    return out
