"""Inputs shared by tests/test_contour_simplify_host.py and tests/test_gpu_contour_simplify.py: the outlines of the packed mask
sets of tests/mask_contours_inputs.py, and general loops where csrc/contour_simplify.hip can go wrong -- loops of 0 to 3 vertices,
one of equal vertices, staircases whose vertex counts stand around the 64 of a wave (62, 64, 66), the 256 threads of a workgroup
(254, 256, 258), a kilo (1022, 1024, 1026: one scan tile) and the 4096 vertices that are staged in LDS (4094, 4096, 4098), one of
40 000 vertices, a comb whose recursion is hundreds deep, 1000 random loops on a 4 x 4 lattice (ties, repeated vertices, the
L == 0 and clamped branches), the loop whose products need more than 64 bits, and 103 242 loops of 0 to 5 vertices whose 263 173
kept flags fill 258 scan tiles (more than the 256 that the scan over the tiles takes in one pass).  Every result of the statement
(mnc_amd.contours.simplify_numpy) is computed once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_contours_inputs as TI  # noqa: E402
import mask_overlap_inputs as MI  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402

CONNECTIVITIES = TI.CONNECTIVITIES
QS = (0, 8, 16, 40, 80)                     # sixteenths of a pixel: 0, 0.5, 1, 2.5 and 5 px
STAIR_SIZES = (62, 64, 66, 254, 256, 258, 1022, 1024, 1026, 4094, 4096, 4098)
LONG = 40000

_SIMPLIFIED, _GENERAL, _GENERAL_REFERENCE = {}, {}, {}


def reference(name, connectivity, q):
    """simplify_numpy of the outlines of that set at q sixteenths, computed once per key and left unchanged."""
    key = (name, connectivity, q)
    if key not in _SIMPLIFIED:
        _SIMPLIFIED[key] = CT.simplify_numpy(TI.reference(name, connectivity), q / 16.0)
    return _SIMPLIFIED[key]


def as_contours(loops):
    """A list of [k, 2] vertex lists as the loops of one instance (areas 0: they are carried over, not read)."""
    vert_ptr = np.concatenate([[0], np.cumsum([len(v) for v in loops])]).astype(np.int64)
    xy = np.concatenate([np.asarray(v, np.int32).reshape(-1, 2) for v in loops]) if loops else np.zeros((0, 2), np.int32)
    return CT.Contours([0, len(loops)], vert_ptr, np.zeros(len(loops), np.int64), xy)


def staircase(k, seed):
    """A closed staircase of k vertices (k even, >= 4) from (0, 0) down to the right and back along the bottom and the left side:
    treads and risers of 1 or 2, seeded, so that the deviations differ and the recursion has something to decide."""
    n = (k - 2) // 2
    rng = np.random.default_rng(seed)
    xs, ys = np.cumsum(1 + (rng.random(n) < 0.3)), np.cumsum(1 + (rng.random(n) < 0.3))
    v = [(0, 0)]
    for i in range(n):
        v += [(int(xs[i]), int(ys[i - 1]) if i else 0), (int(xs[i]), int(ys[i]))]
    v.append((0, int(ys[-1])))
    assert len(v) == k
    return v


def comb(teeth=600):
    """One instance of 2 * teeth x teeth pixels: a bottom row and a tooth on every other column, each one pixel shorter than the
    one before."""
    m = np.zeros((teeth, 2 * teeth), bool)
    m[-1, :] = True
    for t in range(teeth):
        m[t:, 2 * t] = True
    return MI.pack([[3, 2, 2 * teeth + 2, teeth + 1]], [m])


def ties():
    """1000 loops of 3 .. 40 vertices with coordinates in 0 .. 3."""
    rng = np.random.default_rng(14)
    return [rng.integers(0, 4, (int(k), 2)).tolist() for k in rng.integers(3, 41, 1000)]


TINY_VERTS = 256 * 1024 + 1025


def tiny():
    """Loops of 0 to 3 random vertices on a 50 x 50 lattice (7 in 10) or of one lattice point five times (kept as three), until
    there are more than TINY_VERTS vertices: 258 scan tiles, kept flags that are not uniform."""
    rng = np.random.default_rng(5)
    loops, verts = [], 0
    while verts <= TINY_VERTS:
        if rng.random() < 0.7:
            loops.append(rng.integers(0, 50, (int(rng.integers(0, 4)), 2)).tolist())
        else:
            loops.append([rng.integers(0, 50, 2).tolist()] * 5)
        verts += len(loops[-1])
    return loops


WIDE = [(-2 ** 24, 0), (0, 8), (2 ** 24, 0), (0, -8)]

GENERAL = {
    "short": lambda: as_contours([[], [(5, 5)], [(1, 2), (3, 4)], [(0, 0), (4, 0), (0, 4)], [(7, 7)] * 5, [], [(2, 2), (9, 2), (9, 3), (2, 3)]]),
    "stairs": lambda: as_contours([staircase(k, k) for k in STAIR_SIZES]),
    "long": lambda: as_contours([staircase(LONG, 1)]),
    "comb": lambda: CT.contours_numpy(comb(), 8),
    "ties": lambda: as_contours(ties()),
    "wide": lambda: as_contours([WIDE]),
    "tiny": lambda: as_contours(tiny()),
}


def general(name):
    """The Contours of that name, made once."""
    if name not in _GENERAL:
        _GENERAL[name] = GENERAL[name]()
    return _GENERAL[name]


def general_reference(name, q):
    key = (name, q)
    if key not in _GENERAL_REFERENCE:
        _GENERAL_REFERENCE[key] = CT.simplify_numpy(general(name), q / 16.0)
    return _GENERAL_REFERENCE[key]


same_array = TI.same_array


def same_simplified(got, want):
    """Two SimplifiedContours field by field: dtype, shape and bytes."""
    return all(same_array(getattr(got, f), getattr(want, f)) for f in CT.SimplifiedContours.FIELDS)


def deviation(a, b, p):
    """(N, D) of include/mnc_hip.h n14 for the point p and the segment a -> b, in Python integers: written out here once more, from
    the header, so that the tests do not take the statement's word for it."""
    ax, ay, bx, by, px, py = (int(v) for v in (a[0], a[1], b[0], b[1], p[0], p[1]))
    abx, aby, apx, apy = bx - ax, by - ay, px - ax, py - ay
    L, t = abx * abx + aby * aby, apx * abx + apy * aby
    if L == 0:
        return apx * apx + apy * apy, 1
    if t <= 0:
        return (apx * apx + apy * apy) * L, L
    if t >= L:
        return ((px - bx) ** 2 + (py - by) ** 2) * L, L
    return (abx * apy - aby * apx) ** 2, L
