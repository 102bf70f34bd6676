"""Inputs shared by tests/test_mask_shape_host.py and tests/test_gpu_mask_shape.py: packed mask sets placed where
csrc/mask_shape.hip can go wrong -- widths around the 64-column word crossed with heights that cross a wave, a workgroup and a
second scan tile of candidates (random blobs, negative bounds, padding bits set), a diagonal staircase whose candidates are all
collinear, digital discs with as many hull vertices as a wave has lanes, more, and more than a workgroup has, two specks in opposite corners, empty rows above, below
and between, an empty instance between two full ones, no instance at all, 130 small ones, a hundred instances of a 375 x 500
image, and one instance 4097 rows tall.  Every set is seeded; every reference (the numpy statements of mnc_amd.shape) is computed
once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_overlap_inputs as MI  # noqa: E402  (pack; sets up the reference-shaped import paths)
import mask_boundary_inputs as BI  # noqa: E402  (blob)
import render_inputs as RI  # noqa: E402
from mnc_amd import shape as SH  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

WIDTHS = [1, 63, 64, 65, 128, 129]
HEIGHTS = [1, 2, 63, 64, 65, 257, 1025]
STAIR = 40
DISC_R = 60
DISC_RADII = (60, 300, 800)
TALL = 4097


def _place(dense, dirty=True, bounds=None, x0=3, y0=5):
    """Dense masks -> PackedMasks: side by side from (x0, y0) on unless bounds are given; classes 1 .. 3, scores in (0, 1)."""
    if bounds is None:
        bounds, x = [], x0
        for m in dense:
            h, w = m.shape
            bounds.append([x, y0, x + w - 1, y0 + h - 1])
            x += w + 2
    n = len(dense)
    return MI.pack(bounds, dense, np.arange(n) % 3 + 1, ((np.arange(n) + 1) / (n + 1.0)).astype(np.float32), dirty)


def sizes_set(dirty=True):
    """WIDTHS x HEIGHTS random blobs, from x = -300, y = -700 on: the first bounds are negative in both coordinates."""
    rng = np.random.default_rng(1600)
    return _place([BI.blob(rng, h, w) for w in WIDTHS for h in HEIGHTS], dirty, x0=-300, y0=-700)


def staircase(steps=STAIR):
    m = np.zeros((steps, steps), bool)
    m[np.arange(steps), np.arange(steps)] = True
    return m


def disc(r=DISC_R):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


def gaps():
    """Empty rows above, below and between: rows 3 .. 5 and 12 .. 13 of 20 are set, in columns that differ."""
    m = np.zeros((20, 90), bool)
    m[3:6, 10:70] = True
    m[12:14, 40:85] = True
    return m


def shapes_set():
    """One pixel; a 37 x 11 rectangle (w x h); the staircase; the disc; two specks in opposite corners; the gaps; a full
    instance, one with rows and no set pixel, one without rows, a full one; a blob whose first and last rows are empty."""
    rng = np.random.default_rng(1601)
    specks = np.zeros((50, 70), bool)
    specks[0, 69] = specks[49, 0] = True
    inner = np.zeros((30, 66), bool)
    inner[1:-1] = BI.blob(rng, 28, 66)
    dense = [np.ones((1, 1), bool), np.ones((11, 37), bool), staircase(), disc(), specks, gaps(), np.ones((4, 5), bool),
             np.zeros((6, 70), bool), np.zeros((0, 0), bool), np.ones((3, 130), bool), inner]
    bounds, x = [], -50
    for k, m in enumerate(dense):
        h, w = m.shape
        bounds.append([x, -7, x + w - 1, -7 + h - 1] if k != 8 else [x, 4, x - 1, 9])
        x += w + 3
    return _place(dense, bounds=bounds)


def discs_set():
    """Digital discs {x^2 + y^2 <= r^2} of radius 60, 300 and 800: 64, 144 and 288 hull vertices -- one wave of edges, more than
    one wave, and more edges than a workgroup has lanes."""
    return _place([disc(r) for r in DISC_RADII], x0=-900, y0=-850)


def many_set(n=130):
    rng = np.random.default_rng(1602)
    return _place([BI.blob(rng, int(rng.integers(1, 41)), int(rng.integers(1, 41)), 1) for _ in range(n)])


def empty_set():
    return PackedMasks(np.zeros((0, 4), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), None, None, np.zeros(0, np.uint64))


def real_set():
    """A hundred voted-style instances of a 375 x 500 image: five per class, bounds clipped to the image."""
    from mnc_amd.masks import from_lists, instance_masks_numpy
    rng = np.random.default_rng(1603)
    list_mask, list_box = RI.class_lists(rng, 500, 375, 0.0, per_class=(5, 5))
    boxes, masks, classes = from_lists(list_mask, list_box, 0.0)
    return instance_masks_numpy(boxes, masks, 375, 500, clip=True, binarize_thresh=0.4, classes=classes)


def tall_set():
    """4097 rows, 3 columns: a zigzag, whose candidates are not collinear and almost all inside the hull, and a straight line
    beside it."""
    y = np.arange(TALL)
    zig = np.zeros((TALL, 3), bool)
    zig[y, (y // 400) % 3] = True
    zig[0, 0] = zig[-1, 2] = True
    return _place([zig, np.ones((TALL, 1), bool)])


def wide_row():
    """Two rows of 32768 columns at x1 = -2^24 + 1, y1 = 2^24 - 3: every third pixel and the last one set."""
    m = np.zeros((2, 32768), bool)
    m[:, ::3] = True
    m[:, -1] = True
    return _place([m], bounds=[[-2 ** 24 + 1, 2 ** 24 - 3, -2 ** 24 + 32768, 2 ** 24 - 2]])


SETS = {"sizes": sizes_set, "shapes": shapes_set, "discs": discs_set, "many130": many_set, "empty": empty_set, "real": real_set, "tall": tall_set,
        "wide": wide_row}
WHAT = {"moments": SH.moments_numpy, "hull": SH.hull_numpy}
_SETS, _REFERENCE = {}, {}


def get(name):
    if name not in _SETS:
        _SETS[name] = SETS[name]()
    return _SETS[name]


def reference(name, what):
    """moments_numpy / hull_numpy / oriented_numpy (over the cached hull) of that set, computed once per key."""
    key = (name, what)
    if key not in _REFERENCE:
        _REFERENCE[key] = (SH.oriented_numpy(get(name), reference(name, "hull")) if what == "oriented" else WHAT[what](get(name)))
    return _REFERENCE[key]


def same_arrays(got, want):
    assert type(got) is type(want) and len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    return True


def corners_of(m):
    """bool [h, w] -> int [k, 2]: the distinct corners (x, y) of the set pixels' unit squares."""
    ys, xs = np.nonzero(m)
    return np.unique(np.concatenate([np.stack([xs + a, ys + b], 1) for a in (0, 1) for b in (0, 1)]), axis=0)
