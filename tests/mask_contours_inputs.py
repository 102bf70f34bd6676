"""Inputs shared by tests/test_mask_contours_host.py and tests/test_gpu_mask_contours.py: the packed mask sets of
tests/mask_components_inputs.py, which stand where csrc/mask_contours.hip can go wrong as well -- widths around the 64-column word
(a mask of width 63 has 64 lattice points a row, one of width 64 a second word of them), the saddle across the word seam, the
checkerboard (the most edges and loops per word), the spiral and the serpentine (loops of more than 2^14 edges: the most jumping
rounds), holes that touch the box edge, nested rings, full and empty masks, instances without rows, dirty padding, 300 small
instances, one set at real size -- and a set of its own: a single pixel, rows and columns of one pixel at those widths, two pixels
that touch diagonally both ways round, a rectangle flush with (0, 0), and rectangles whose loops are just below, at and above a
power of two of edges.  CI's `stripes` (625 114 edges: 611 scan tiles) stands outside SETS here as well.  Every reference (mnc_amd.contours.contours_numpy) is computed once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_components_inputs as CI  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402

CONNECTIVITIES = CI.CONNECTIVITIES
WIDTHS = CI.WIDTHS


def lines():
    """A single pixel; a 1 x w row and an h x 1 column of set pixels at every width of WIDTHS; the diagonal pairs; a rectangle
    flush with (0, 0); 1 x 15, 1 x 16 and 1 x 17 (32, 34 and 36 edges) and 1 x 510, 1 x 511 and 1 x 512 (1022, 1024 and 1026
    edges: around 2^10); all with dirty padding."""
    dense = [np.ones((1, 1), bool)]
    dense += [np.ones((1, w), bool) for w in WIDTHS] + [np.ones((w, 1), bool) for w in WIDTHS]
    dense += [np.eye(2, dtype=bool), np.eye(2, dtype=bool)[::-1].copy()]
    bounds, x = [], 2
    for m in dense:
        h, w = m.shape
        bounds.append([x, 7, x + w - 1, 7 + h - 1])
        x += w + 1
    dense.append(np.ones((4, 6), bool))
    bounds.append([0, 0, 5, 3])
    for k, w in enumerate((15, 16, 17, 510, 511, 512)):
        dense.append(np.ones((1, w), bool))
        bounds.append([1, 300 + 2 * k, w, 300 + 2 * k])
    n = len(dense)
    return CI.MI.pack(bounds, dense, np.arange(n) % 3 + 1, (np.arange(n) + 1) / (n + 1.0), True)


SETS = dict(CI.SETS)
SETS["lines"] = lines

_SETS, _REFERENCE = {}, {}


def get(name):
    """The set of that name, made once."""
    if name not in _SETS:
        _SETS[name] = lines() if name == "lines" else CI.get(name)
    return _SETS[name]


def reference(name, connectivity):
    """contours_numpy of that set, computed once per key and left unchanged."""
    key = (name, connectivity)
    if key not in _REFERENCE:
        _REFERENCE[key] = CT.contours_numpy(get(name), connectivity)
    return _REFERENCE[key]


same_array = CI.same_array


def same_contours(got, want):
    """Two Contours field by field: dtype, shape and bytes."""
    return all(same_array(getattr(got, f), getattr(want, f)) for f in CT.Contours.FIELDS)


def image_size(pm):
    """(H, W) of an image that holds every instance of the set (at least 1 x 1)."""
    rows = [i for i in range(len(pm)) if min(pm.size(i)) > 0]
    return (max([int(pm.bounds[i][3]) + 1 for i in rows] + [1]), max([int(pm.bounds[i][2]) + 1 for i in rows] + [1]))


def inside(pm):
    """The set moved so that no instance with rows begins left of or above the image -> (PackedMasks, dx, dy)."""
    from mnc_amd.masks import PackedMasks
    rows = [i for i in range(len(pm)) if min(pm.size(i)) > 0]
    dx = max([0] + [-int(pm.bounds[i][0]) for i in rows])
    dy = max([0] + [-int(pm.bounds[i][1]) for i in rows])
    bounds = pm.bounds + np.array([dx, dy, dx, dy], np.int32)
    return PackedMasks(bounds, pm.offsets.copy(), pm.areas.copy(), pm.classes.copy(), pm.scores.copy(), pm.bits.copy()), dx, dy
