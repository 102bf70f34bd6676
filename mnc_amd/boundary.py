"""The boundary bands of packed instance masks (include/mnc_hip.h n11, csrc/mask_boundary.hip): the rule of the published
mask_to_boundary of Boundary IoU (Cheng et al., CVPR 2021; iouType="boundary" of the COCO toolkit, the measure of LVIS) on
mnc_amd.masks.PackedMasks.

    boundary_distance(H, W, ratio=0.02)   d = max(1, int(round(ratio * sqrt(H*H + W*W)))), Python 3's round: half to even
    boundary_numpy(pm, H, W, d)           the CPU statement: per instance unpack, crop to the image, pad with d zeros, AND the
                                          (2d+1)^2 window, B = M & ~E, repack
    boundary(pm, H, W, d=None, ...)       the same PackedMasks through mnc_mask_boundary (the GPU); PackedMasks.boundary is the method

The boundary of a mask M in an H x W image at distance d >= 1: M is first cropped to the image; E is the set of pixels p of M for
which every q with |qx - px| <= d and |qy - py| <= d lies inside the image and in M; B = M \\ E.  (mask_to_boundary adds a one-pixel
zero border, runs cv2.erode with a 3 x 3 kernel of ones d times, removes the border and subtracts: the same set.)  The result has
the input's layout: instance i has the input bounds intersected with the image, not tightened; an instance without rows or outside
the image gets (0, 0, -1, -1), no rows and area 0; offsets are multiples of 8, in order, without gaps; areas are the true bit
counts; padding bits are 0; classes and scores are carried over.  There is no fallback: without the library or a GPU boundary()
raises."""
import ctypes
import math

import numpy as np

from . import _lib
from .masks import MAX_SIDE, PackedMasks, _device_id, _set_args, sized_then_filled

MAX_N = 2048
MAX_D = 1024


def boundary_distance(H, W, ratio=0.02):
    """The dilation distance of an H x W image: ratio times the diagonal, rounded half to even, at least 1."""
    return max(1, int(round(float(ratio) * math.sqrt(int(H) * int(H) + int(W) * int(W)))))


def _distance(who, H, W, d, ratio):
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("%s: image %d x %d not in [1, %d]" % (who, H, W, MAX_SIDE))
    d = boundary_distance(H, W, ratio) if d is None else int(d)
    if not 1 <= d <= MAX_D:
        raise ValueError("%s: d=%d not in [1, %d]" % (who, d, MAX_D))
    return H, W, d


def clipped_bounds(bounds, H, W):
    """The bounds of the result: each input bound intersected with the image, (0, 0, -1, -1) where nothing is left.  -> int32 [n, 4]"""
    b = np.asarray(bounds, np.int64).reshape(-1, 4)
    out = np.stack((np.maximum(b[:, 0], 0), np.maximum(b[:, 1], 0), np.minimum(b[:, 2], W - 1), np.minimum(b[:, 3], H - 1)), axis=1)
    gone = (b[:, 2] < b[:, 0]) | (b[:, 3] < b[:, 1]) | (out[:, 2] < out[:, 0]) | (out[:, 3] < out[:, 1])
    out[gone] = (0, 0, -1, -1)
    return out.astype(np.int32)


def erode_numpy(m, d):
    """bool [h, w] -> the pixels whose whole (2d+1)^2 window is set, everything outside the array counting as unset."""
    h, w = m.shape
    p = np.zeros((h + 2 * d, w + 2 * d), bool)
    p[d:d + h, d:d + w] = m
    rows = np.ones((h + 2 * d, w), bool)
    for s in range(2 * d + 1):                                   # along the row
        rows &= p[:, s:s + w]
    out = np.ones((h, w), bool)
    for s in range(2 * d + 1):                                   # down the column
        out &= rows[s:s + h]
    return out


def boundary_numpy(pm, H, W, d):
    """The rule as a plain loop on the host -- the specification csrc/mask_boundary.hip is tested against.  -> PackedMasks.
    Raises ValueError where mnc_mask_boundary returns MNC_ERR_INVALID for H, W or d."""
    H, W, d = _distance("boundary_numpy", H, W, d, None)
    bounds = clipped_bounds(pm.bounds, H, W)
    dense = [None] * len(bounds)
    for i in range(len(bounds)):
        x1, y1, x2, y2 = (int(v) for v in bounds[i])
        if x2 < x1 or y2 < y1:
            continue
        ax, ay = int(pm.bounds[i][0]), int(pm.bounds[i][1])
        m = pm.dense(i)[y1 - ay:y2 - ay + 1, x1 - ax:x2 - ax + 1]
        # (the clipped box ends where the image does or where the mask's bounds do, and the mask is 0 beyond those: zeros all round)
        dense[i] = m & ~erode_numpy(m, d)
    return PackedMasks.from_dense(bounds, dense, pm.classes, pm.scores)


def boundary_call(pm, H, W, d, bits=None, device_id=0):
    """mnc_mask_boundary as it is: bits None asks for bounds, offsets and the size only (nothing is launched).  -> (bounds,
    offsets, areas, bytes needed)."""
    n = len(pm)
    bounds, offsets, areas = np.zeros((n, 4), np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    need = ctypes.c_size_t(0)
    _lib.call("mnc_mask_boundary", *(_set_args(pm, areas=False) + (
        int(H), int(W), int(d), _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits),
        bits.nbytes if bits is not None else 0, ctypes.addressof(need), int(device_id))))
    return bounds, offsets, areas, int(need.value)


def boundary(pm, H, W, d=None, ratio=0.02, device_id=None):
    """boundary_numpy on the GPU (mnc_mask_boundary, csrc/mask_boundary.hip): the same PackedMasks field by field.  d None: the
    distance of the image at `ratio`.  Invalid sets and sizes raise ValueError or _lib.MncError (MNC_ERR_INVALID) before anything
    is launched."""
    H, W, d = _distance("boundary", H, W, d, ratio)
    dev = _device_id(device_id)
    bounds, offsets, areas, bits = sized_then_filled(lambda bits: boundary_call(pm, H, W, d, bits, dev))
    return PackedMasks(bounds, offsets, areas, pm.classes, pm.scores, bits)
