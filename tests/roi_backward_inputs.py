"""Shared corpus of tests/test_roi_backward_host.py and tests/test_gpu_roi_backward.py: inputs of the backward passes of
ROIWarping, MAX 2x2/2, MaskResize and MaskPooling (mnc_amd/backward.py), and their statements' results, computed once."""
import functools

import numpy as np

from mnc_amd import backward as B

H, W, SCALE = 9, 13, 0.0625                       # a 144 x 208 image at stride 16

# (batch index, x1, y1, x2, y2) in image coordinates
ROIS = np.array([
    [0, 0.0, 0.0, 207.0, 143.0],                  # the whole map
    [0, 10.3, 20.7, 10.9, 21.2],                  # sub-pixel: every sample inside one cell
    [0, 192.0, 128.0, 192.0, 128.0],              # bottom-right corner cell, width and height exactly 1: the tied clamp, taps off the map
    [0, 120.5, 60.2, 90.1, 100.3],                # malformed x2 < x1: the width is clamped, the height is free
    [0, -30.2, -20.4, 230.6, 160.8],              # partly outside on every side
    [0, 400.5, 300.5, 460.2, 350.1],              # wholly outside
    [0, 33.7, 17.2, 150.4, 99.8],                 # ordinary
    [0, 66.1, 40.9, 121.3, 130.6],                # ordinary
], np.float32)
CHANNELS = (8, 64, 320)
GRIDS = ((7, 7), (14, 14), (3, 5))
WARP_CASES = [(C, PH, PW) for C in CHANNELS for PH, PW in GRIDS]


def _case(feat, rois, PH, PW, scale, dtop):
    return {"feat": feat, "rois": rois, "PH": PH, "PW": PW, "scale": scale, "dtop": dtop}


@functools.lru_cache(maxsize=None)
def warp_case(C, PH, PW):
    rng = np.random.default_rng(1000 * C + 10 * PH + PW)
    return _case(rng.standard_normal((C, H, W)).astype(np.float32), ROIS, PH, PW, SCALE,
                 rng.standard_normal((len(ROIS), C, PH, PW)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def empty_case():
    rng = np.random.default_rng(5)
    return _case(rng.standard_normal((8, H, W)).astype(np.float32), np.zeros((0, 5), np.float32), 7, 7, SCALE,
                 np.zeros((0, 8, 7, 7), np.float32))


@functools.lru_cache(maxsize=None)
def head_case():
    """The head's width: C = 512 on the 38 x 63 map of a 600 x 1000 image, 64 RoIs, 14 x 14."""
    rng = np.random.default_rng(6)
    R, C, Hh, Wh = 64, 512, 38, 63
    x1, y1 = rng.uniform(-20, 900, R), rng.uniform(-20, 520, R)
    rois = np.stack([np.zeros(R), x1, y1, x1 + rng.uniform(4, 600, R), y1 + rng.uniform(4, 400, R)], 1).astype(np.float32)
    return _case(rng.standard_normal((C, Hh, Wh)).astype(np.float32), rois, 14, 14, SCALE,
                 rng.standard_normal((R, C, 14, 14)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def dyadic_case(C=16):
    """Every product and sum exact in float32: small integers, boxes of 96 x 96 at multiples of 16 with P = 14, so the bins are
    0.5 cells, the fractions 0 or 0.5 and the weights 0, 0.25, 0.5 or 1.  Two boxes reach off the map."""
    rng = np.random.default_rng(7)
    xy = np.array([[0, 0], [16, 32], [112, 48], [-32, -16], [64, 16]], np.float32)
    rois = np.concatenate([np.zeros((len(xy), 1), np.float32), xy, xy + 96], 1)
    return _case(rng.integers(-4, 5, (C, H, W)).astype(np.float32), rois, 14, 14, SCALE,
                 rng.integers(-3, 4, (len(xy), C, 14, 14)).astype(np.float32))


def args(case):
    return case["feat"], case["rois"], case["PH"], case["PW"], case["scale"], case["dtop"]


_refs = {}


def warp_ref(key, case):
    """(float32 statement, float64 form) of a case, computed once per process and never changed."""
    if key not in _refs:
        f32, f64 = B.roi_warp_backward_numpy(*args(case)), B.roi_warp_backward_f64(*args(case))
        for a in f32 + f64:
            a.setflags(write=False)
        _refs[key] = (f32, f64)
    return _refs[key]


# ---- MAX 2x2/2: integers from a small range (most windows hold a tie), one constant window, one constant negative window
POOL_CASES = ((2, 4, 6, 10), (3, 68, 4, 2), (2, 320, 2, 6))


@functools.lru_cache(maxsize=None)
def pool_case(R, C, PH, PW):
    rng = np.random.default_rng(R + C + PH + PW)
    x = rng.integers(-2, 3, (R, C, PH, PW)).astype(np.float32)
    x[0, 0, :2, :2] = 1.5                          # a constant window: the gradient goes to (0, 0)
    x[-1, -1, -2:, -2:] = -7.0
    return x, rng.standard_normal((R, C, PH // 2, PW // 2)).astype(np.float32)


# ---- MaskResize: (IH, IW, OH, OW); the second and third hit the edge rule (IH = OH: ratio 1, the last row / column is nearest)
RESIZE_CASES = ((21, 21, 14, 14), (14, 14, 14, 14), (5, 7, 9, 7), (28, 28, 14, 14), (3, 2, 5, 11))


@functools.lru_cache(maxsize=None)
def resize_case(IH, IW, OH, OW, R=3):
    return np.random.default_rng(IH * 31 + OW).standard_normal((R, 1, OH, OW)).astype(np.float32)


# ---- MaskPooling: (R, C, PH, PW); 320 channels = more than one pass of a wave's 256
MASKPOOL_CASES = ((3, 4, 3, 5), (2, 64, 14, 14), (2, 320, 7, 7))


@functools.lru_cache(maxsize=None)
def maskpool_case(R, C, PH, PW):
    rng = np.random.default_rng(R * 7 + C + PH)
    return (rng.standard_normal((R, C, PH, PW)).astype(np.float32), rng.uniform(0, 1, (R, 1, PH, PW)).astype(np.float32),
            rng.standard_normal((R, C, PH, PW)).astype(np.float32))


def bound(terms, abs_sum):
    """The worst-case distance of any float32 evaluation of a sum of `terms` addends from its exact value."""
    return (np.asarray(terms, np.float64) + 32.0) * 2.0 ** -24 * np.asarray(abs_sum, np.float64)
