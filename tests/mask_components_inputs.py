"""Inputs shared by tests/test_mask_components_host.py and tests/test_gpu_mask_components.py: packed mask sets placed where
csrc/mask_components.hip can go wrong -- widths around the 64-column word with many runs and merges, the word seam, the checkerboard
(the run maximum), a spiral (the longest parent chains), a comb (every merge at the end), rings, a C-shape, holes that touch the box
edge, nested rings, full and empty masks, instances without rows, dirty padding, 300 small instances, one set at real size -- and, outside SETS (the GPU tests name the operations they run on it), `stripes`: one instance
whose runs, roots and boundary edges fill more than the 256 scan tiles that the scan over the tiles takes in one pass.  Every
reference (the numpy statements of mnc_amd.components) is computed once per key and shared."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_overlap_inputs as MI  # noqa: E402  (sets up the reference-shaped import paths)
import render_inputs as RI  # noqa: E402
from mnc_amd import components as CC  # noqa: E402

WIDTHS = [1, 63, 64, 65, 127, 128, 129, 200]
DENSITIES = [0.5, 0.6]
CONNECTIVITIES = [4, 8]
SELECTIONS = [(1, 0), (4, 0), (1, 1), (2, 3)]          # (min_area, keep)


def _place(dense, dirty=False, bounds=None):
    """Dense masks -> PackedMasks: side by side from (3, 5) on unless bounds are given; classes 1 .. 3, scores in (0, 1)."""
    if bounds is None:
        bounds, x = [], 3
        for m in dense:
            h, w = m.shape
            bounds.append([x, 5, x + w - 1, 5 + h - 1])
            x += w + 2
    n = len(dense)
    return MI.pack(bounds, dense, np.arange(n) % 3 + 1, (np.arange(n) + 1) / (n + 1.0), dirty)


def widths(dirty=False):
    """Every width of WIDTHS by 40 rows at both densities: many runs and many merges."""
    rng = np.random.default_rng(1200)
    return _place([rng.random((40, w)) < p for w in WIDTHS for p in DENSITIES], dirty=dirty)


def seam():
    """Bit 63 of word 0 in row y and bit 0 of word 1 in row y + 1: two components at 4, one at 8 -- alone, mirrored, and in the
    middle of longer runs; a run that spans three words above two runs that it joins; two rectangles that touch at a corner."""
    a = np.zeros((2, 128), bool)
    a[0, 63] = a[1, 64] = True
    b = a[::-1].copy()
    c = np.zeros((3, 200), bool)
    c[0, 60:64] = c[1, 64:70] = c[2, 63] = True
    d = np.zeros((3, 200), bool)
    d[1, 10:181] = True                                 # words 0, 1 and 2
    d[0, 5:12] = d[0, 100] = d[0, 181] = d[2, 0:10] = d[2, 150:200] = True
    e = np.zeros((8, 12), bool)
    e[0:4, 0:5] = e[4:8, 5:12] = True
    return _place([a, b, c, d, e])


def checker():
    """66 x 130: 4290 components of one pixel at 4, one component at 8; ceil(w / 2) runs in every row."""
    yy, xx = np.mgrid[0:66, 0:130]
    return _place([(yy + xx) % 2 == 0])


def spiral_mask(n=129):
    """A spiral of one-pixel walls in n x n, walls two pixels apart: one component, wound inwards."""
    m = np.zeros((n, n), bool)
    x0, y0, x1, y1 = 0, 0, n - 1, n - 1
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        m[y0, x0:x1 + 1] = True
        m[y0:y1 + 1, x1] = True
        m[y1, x0 + 2:x1 + 1] = True
        m[y0 + 2:y1 + 1, x0 + 2] = True
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
        m[y0, x0] = True                                # the joint to the next turn
    return m


def spiral():
    """The spiral, and a serpentine of the same size (rows joined at alternating ends)."""
    s = np.zeros((129, 129), bool)
    s[::2] = True
    s[1::4, -1] = True
    s[3::4, 0] = True
    return _place([spiral_mask(), s])


def comb():
    """65 teeth, 100 rows high, joined only by the last row; and the same upside down (joined by the first)."""
    m = np.zeros((100, 129), bool)
    m[:, ::2] = True
    m[-1] = True
    return _place([m, m[::-1].copy()])


def ring(h, w, t=2):
    m = np.ones((h, w), bool)
    m[t:h - t, t:w - t] = False
    return m


def holes(dirty=False):
    """A ring; a C-shape (the ring cut open); a hole that touches the box edge (no hole at either connectivity); a ring inside a
    ring's hole; a hole that meets the outside only across a corner (a hole of the 4-connected background alone); a ring 70 wide
    whose hole crosses the word seam; a pinhole at column 63 and one at column 64."""
    r = ring(12, 20)
    c = ring(12, 20)
    c[5:7, 18:] = False
    edge = np.ones((10, 15), bool)
    edge[0:4, 6:9] = False
    edge[4:7, 0:3] = False
    nested = ring(30, 40, 3)
    nested[8:22, 10:30] = ring(14, 20, 2)
    corner = np.ones((8, 8), bool)
    corner[0, 0] = corner[1, 1] = corner[2, 2] = False
    wide = ring(9, 70, 3)
    pins = np.ones((5, 130), bool)
    pins[2, 63] = pins[3, 64] = pins[1, 0] = pins[2, 129] = False
    return _place([r, c, edge, nested, corner, wide, pins], dirty=dirty)


def plain():
    """Full and empty masks of several widths, and instances without rows in the middle of the set."""
    dense = [np.ones((5, 70), bool), np.zeros((5, 70), bool), np.zeros((4, 0), bool), np.ones((1, 1), bool), np.zeros((0, 7), bool),
             np.ones((3, 64), bool), np.zeros((1, 1), bool), np.ones((2, 129), bool)]
    bounds = [[0, 0, 69, 4], [80, 0, 149, 4], [40, 10, 39, 13], [7, 7, 7, 7], [50, 30, 56, 29], [-10, -2, 53, 0], [9, 9, 9, 9],
              [100, 20, 228, 21]]
    return _place(dense, bounds=bounds, dirty=True)


def many():
    """300 instances of about 20 x 20 at mixed densities: more than any one workgroup's share."""
    rng = np.random.default_rng(1300)
    dense, bounds = [], []
    for k in range(300):
        h, w = int(rng.integers(15, 26)), int(rng.integers(15, 26))
        dense.append(rng.random((h, w)) < (0.3, 0.5, 0.7)[k % 3])
        x, y = int(rng.integers(0, 900)), int(rng.integers(0, 500))
        bounds.append([x, y, x + w - 1, y + h - 1])
    return _place(dense, bounds=bounds)


def real():
    """Ten instances of the 600 x 1000 synthetic image of render_inputs (bounds not clipped), as mask_boundary_inputs.real_set
    builds its own."""
    from mnc_amd.masks import instance_masks_numpy
    W, H, pred, _ = RI.random_case(RI.BIG_SIZES.index((600, 1000)))
    boxes = np.array([np.asarray(b, np.float64) for b in pred["boxes"][:10]])
    return instance_masks_numpy(boxes, np.array(pred["masks"][:10]), H, W, clip=False, binarize_thresh=0.4, classes=pred["cls_name"][:10])


def stripes():
    """520 x 1200, every other column set, one pixel in 100 of them cleared: 308 891 runs (302 scan tiles) in 3666 components at
    either connectivity, whose roots lie in all of the tiles; 625 114 boundary edges (611 tiles)."""
    m = np.zeros((520, 1200), bool)
    m[:, ::2] = True
    m[np.random.default_rng(1500).random(m.shape) < 0.01] = False
    return _place([m])


SETS = {"widths": widths, "widths_dirty": lambda: widths(True), "seam": seam, "checker": checker, "spiral": spiral, "comb": comb,
        "holes": holes, "holes_dirty": lambda: holes(True), "plain": plain, "many": many, "real": real}

_SETS, _REFERENCE = {}, {}


def get(name):
    """The set of that name, made once."""
    if name not in _SETS:
        _SETS[name] = stripes() if name == "stripes" else SETS[name]()
    return _SETS[name]


def reference(name, op, *args):
    """op in "components", "select", "fill_holes", "split" with the statement's arguments after the set -> its result, computed once
    per key and left unchanged."""
    key = (name, op) + args
    if key not in _REFERENCE:
        _REFERENCE[key] = getattr(CC, op + "_numpy")(get(name), *args)
    return _REFERENCE[key]


def same_array(got, want):
    """dtype, shape and bytes."""
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def same_masks(got, want):
    """Two PackedMasks field by field: dtype, shape and bytes."""
    return all(same_array(getattr(got, f), getattr(want, f)) for f in want.FIELDS)


def same_components(got, want):
    return all(same_array(g, w) for g, w in zip(got, want))
