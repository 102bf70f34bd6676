"""Inputs shared by tests/test_mask_distance_host.py and tests/test_gpu_mask_distance.py: packed mask sets placed where
csrc/mask_distance.hip can go wrong -- widths around the 64-column word crossed with heights from one row on (random blobs, all-ones
masks, all-ones masks with one unset pixel inside a middle word), masks three words wide for discs of a whole word's reach, all-ones
rectangles whose nearest unset pixel lies 130 columns or rows away, tall narrow masks, bounds that are negative, leave an image or
have no rows, more than one wave of instances, and one set at real size.  Every set is seeded; every reference (the numpy
statements of mnc_amd.distance) is computed once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_overlap_inputs as MI  # noqa: E402  (pack; sets up the reference-shaped import paths)
import mask_boundary_inputs as BI  # noqa: E402  (blob, real_set)
from mnc_amd import distance as DT  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 191, 193]
HEIGHTS = [1, 2, 7, 33]
R2S = [0, 1, 2, 5, 9]
HOST_R2S = [0, 1, 2, 4, 5, 8, 9, 13, 50, 4096]
WORD_R2S = [63 * 63, 64 * 64, 65 * 65]
OPS = DT.OPS


def _place(dense, dirty=False, bounds=None, x0=3, y0=5):
    """Dense masks -> PackedMasks: side by side from (x0, y0) on unless bounds are given; classes 1 .. 3, scores in (0, 1)."""
    if bounds is None:
        bounds, x = [], x0
        for m in dense:
            h, w = m.shape
            bounds.append([x, y0, x + w - 1, y0 + h - 1])
            x += w + 2
    n = len(dense)
    return MI.pack(bounds, dense, np.arange(n) % 3 + 1, ((np.arange(n) + 1) / (n + 1.0)).astype(np.float32), dirty)


def word_set(dirty=False):
    """WIDTHS x HEIGHTS, three masks each: a random blob, all ones, and all ones with one unset pixel inside the middle word (the
    lowest word of a mask one word wide).  120 instances, from x = -40 on: the first bounds are negative."""
    rng = np.random.default_rng(1500)
    dense = []
    for w in WIDTHS:
        for h in HEIGHTS:
            dense.append(BI.blob(rng, h, w))
            dense.append(np.ones((h, w), bool))
            hole = np.ones((h, w), bool)
            word = ((w + 63) // 64) // 2
            hole[h // 2, min(word * 64 + int(rng.integers(1, 63)), w - 1)] = False
            dense.append(hole)
    return _place(dense, dirty, x0=-40, y0=-3)


def reach_set():
    """Masks three and four words wide (129 .. 256 columns, 70 .. 140 rows) for discs of radius 63, 64 and 65: blobs, a full one,
    and two dots 150 columns apart, whose dilations meet the unaligned source shift and a walk past a whole word."""
    rng = np.random.default_rng(1501)
    dense = [BI.blob(rng, 70, 129, 6), BI.blob(rng, 140, 200, 9), np.ones((135, 256), bool), BI.blob(rng, 90, 193, 2)]
    dots = np.zeros((3, 200), bool)
    dots[1, 10] = dots[1, 160] = True
    dense.append(dots)
    return _place(dense, dirty=True)


def far_set():
    """All-ones rectangles of 260 x 600 and 600 x 260 (h x w): the nearest unset pixel of the middle lies 130 columns away across
    three full words, resp. 130 rows away."""
    return _place([np.ones((260, 600), bool), np.ones((600, 260), bool)], dirty=True)


def tall_set():
    """Widths 1 to 3 at height 300: all ones, and a blob of each width."""
    rng = np.random.default_rng(1502)
    dense = []
    for w in (1, 2, 3):
        dense += [np.ones((300, w), bool), BI.blob(rng, 300, w, 20)]
    return _place(dense, dirty=True)


BOUNDS_H, BOUNDS_W = 60, 150


def bounds_set(dirty=True):
    """In and around a 60 x 150 image: negative and unclipped bounds, instances without rows, one with rows and no set pixel, one
    so far outside that even its dilation by 5 misses the image."""
    rng = np.random.default_rng(1503)
    bounds = [[-1, 5, 80, 40], [-63, 10, 30, 50], [-65, -4, 70, 30], [100, 10, 170, 40], [20, -9, 90, 20], [-5, -5, BOUNDS_W + 4, BOUNDS_H + 4],
              [40, 10, 39, 20],                                           # no rows
              [10, 10, 80, 30],                                           # rows, no set pixel
              [-80, 10, -3, 30],                                          # outside; a dilation by rho >= 3 reaches the image
              [200, 100, 230, 130],                                       # far outside
              [50, 30, 60, 29],                                           # no rows
              [0, 0, BOUNDS_W - 1, BOUNDS_H - 1], [149, 59, 200, 90]]
    dense = []
    for k, b in enumerate(bounds):
        h, w = max(b[3] - b[1] + 1, 0), max(b[2] - b[0] + 1, 0)
        m = rng.random((h, w)) < 0.9 if h * w else np.zeros((h, w), bool)
        if k == 7:
            m[:] = False
        dense.append(m)
    n = len(bounds)
    return MI.pack(bounds, dense, np.arange(n) % 3 + 1, np.linspace(0.1, 0.9, n).astype(np.float32), dirty)


def many_set(n):
    """n small blobs (more than one wave of instances at n = 65 and 130), 5 .. 40 pixels a side."""
    rng = np.random.default_rng(1504 + n)
    return _place([BI.blob(rng, int(rng.integers(5, 41)), int(rng.integers(5, 41)), 1) for _ in range(n)], dirty=True)


def empty_set():
    return PackedMasks(np.zeros((0, 4), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), None, None, np.zeros(0, np.uint64))


def real_set():
    """Ten voted-style instances of the 600 x 1000 synthetic image (bounds not clipped)."""
    return BI.real_set().pm


SETS = {"word": word_set, "reach": reach_set, "far": far_set, "tall": tall_set, "bounds": bounds_set, "many65": lambda: many_set(65),
        "many130": lambda: many_set(130), "empty": empty_set, "real": real_set}
_SETS, _REFERENCE = {}, {}


def get(name):
    if name not in _SETS:
        _SETS[name] = SETS[name]()
    return _SETS[name]


def reference(name, what, *args):
    """distance_numpy / inscribed_numpy / morph_numpy(op, r2, H, W) of that set, computed once per key."""
    key = (name, what) + args
    if key not in _REFERENCE:
        pm = get(name)
        _REFERENCE[key] = (DT.distance_numpy(pm) if what == "distance" else DT.inscribed_numpy(pm) if what == "inscribed"
                           else DT.morph_numpy(pm, what, *args))
    return _REFERENCE[key]


def same_masks(got, want):
    for f in PackedMasks.FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
    return True


def same_arrays(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    return True


def disc(r2):
    """bool [2 rho + 1, 2 rho + 1]: the structuring element, and rho."""
    rho = int(np.floor(np.sqrt(r2)))
    while (rho + 1) ** 2 <= r2:
        rho += 1
    while rho * rho > r2:
        rho -= 1
    yy, xx = np.mgrid[-rho:rho + 1, -rho:rho + 1]
    return yy * yy + xx * xx <= r2, rho
