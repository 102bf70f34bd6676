"""Inputs shared by tests/test_surface_dist_host.py and tests/test_gpu_surface_dist.py: pairs of packed mask sets placed where
csrc/mask_surface.hip can go wrong -- widths around the 64-column word crossed with heights 1, 2 and 65 at x1 = 0, 1 and 63 modulo
64 (padding bits set); single-pixel sources in the eight sectors around a 3 x 3 destination and inside it; a destination whose only
surface pixel of a row is at the far end; two blobs with empty rows between them; a ring with a dot in its hole; equal maxima
planted in different words, waves and workgroups; one source of more than one workgroup of words against a sparse destination;
130 small instances; bounds at the ends of the permitted span; instances without rows and without a bit; no instance.  Every set is
seeded; every reference (the numpy statements of mnc_amd.surface) is computed once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_overlap_inputs as MI  # noqa: E402  (pack; sets up the reference-shaped import paths)
from mnc_amd import surface as SF  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

WIDTHS = [1, 63, 64, 65, 129]
HEIGHTS = [1, 2, 65]
STARTS = [0, 1, 63]                                 # x1 modulo 64
TAU2 = [0, 1, 4, 25, 100, 2 ** 31 - 1]
TIE_W, TIE_H = 129, 65                              # 3 words a row, 195 words: four workgroups of 64 words, waves of 16
# (x, y) of the planted maxima: word 3 y + x // 64 of the instance -- wave 0 and wave 1 of workgroup 0, workgroup 1, workgroup 3
TIE_SPOTS = [(10, 2), (70, 8), (5, 40), (128, 64)]
TIE_D2 = 25                                         # every spot's partner stands (3, 4) away


def _random(rng, h, w, p=0.5):
    m = rng.random((h, w)) < p
    m[0, 0] = m[-1, -1] = True
    return m


def _box(x1, y1, m):
    return [x1, y1, x1 + m.shape[1] - 1, y1 + m.shape[0] - 1]


def _pack(items, dirty=True):
    """[(x1, y1, bool [h, w])] -> PackedMasks with classes 1 .. n and descending scores."""
    n = len(items)
    return MI.pack([_box(x1, y1, m) for x1, y1, m in items], [m for _, _, m in items], np.arange(1, n + 1),
                   np.linspace(0.9, 0.1, n) if n else None, dirty)


def word_edges_set(dirty=True):
    """WIDTHS x HEIGHTS x STARTS random masks, x1 = the start or the start plus 64, y1 = 0 .. 2."""
    rng = np.random.default_rng(2200)
    items = []
    for w in WIDTHS:
        for h in HEIGHTS:
            for s in STARTS:
                items.append((s + 64 * ((w + h) % 2), (w + s) % 3, _random(rng, h, w)))
    return _pack(items, dirty)


def word_edges_pairs():
    """Every instance with the next and with itself."""
    n = len(WIDTHS) * len(HEIGHTS) * len(STARTS)
    return np.array([[i, j] for i in range(n) for j in (i, (i + 1) % n)], np.int32)


def sectors_sets():
    """a: single pixels in the eight sectors around b's bounds and one at its centre; b: a solid 3 x 3 at (10, 10)."""
    one = np.ones((1, 1), bool)
    spots = [(5, 4), (11, 3), (20, 6), (2, 11), (17, 11), (6, 19), (11, 15), (14, 14), (11, 11)]
    return _pack([(x, y, one) for x, y in spots]), _pack([(10, 10, np.ones((3, 3), bool))])


def far_sets():
    """b: 200 columns of 6 rows whose only pixel of a row stands at the far end from the sources -- rows 0 .. 2 at x = 199, rows
    3 .. 5 at x = 0 -- ; a: pixels left of, right of, above and inside b's bounds."""
    m = np.zeros((6, 200), bool)
    m[:3, 199] = True
    m[3:, 0] = True
    one = np.ones((1, 1), bool)
    return _pack([(x, y, one) for x, y in [(-5, 1), (260, 4), (100, -7), (100, 2), (3, 0), (196, 5)]]), _pack([(0, 0, m)])


def empty_rows_sets():
    """b: two blobs in one bound of 41 x 31 with 19 empty rows between them; a: masks above, between and below the blobs."""
    rng = np.random.default_rng(2201)
    m = np.zeros((31, 41), bool)
    m[0:6, 3:20] = _random(rng, 6, 17, 0.7)
    m[25:31, 22:41] = _random(rng, 6, 19, 0.7)
    a = [(5, 10, _random(rng, 9, 30, 0.3)), (-8, -9, _random(rng, 4, 70, 0.4)), (30, 14, np.ones((1, 1), bool)),
         (0, 33, _random(rng, 3, 41, 0.5))]
    return _pack(a), _pack([(0, 0, m)])


def ring_sets():
    """a: a ring of outer radius 12 and inner radius 7 about (20, 20); b: the dot at its centre."""
    y, x = np.mgrid[0:41, 0:41]
    r2 = (x - 20) ** 2 + (y - 20) ** 2
    return _pack([(0, 0, (r2 <= 144) & (r2 >= 49))]), _pack([(20, 20, np.ones((1, 1), bool))])


def tie_sets():
    """a: isolated pixels in a TIE_W x TIE_H bound -- the TIE_SPOTS, whose nearest pixel of b stands (3, 4) away, and fillers
    that b repeats in place; b: the partners, in a bound shifted by (3, 4)."""
    rng = np.random.default_rng(2202)
    a, b = np.zeros((TIE_H, TIE_W), bool), np.zeros((TIE_H, TIE_W), bool)
    for x, y in TIE_SPOTS:                                  # b's bound starts at (3, 4): its pixel (x, y) is image pixel (x + 3, y + 4)
        a[y, x] = b[y, x] = True
    near = TIE_SPOTS + [(x + 3, y + 4) for x, y in TIE_SPOTS]
    for _ in range(60):                                     # fillers more than 8 away from every spot and partner
        x, y = int(rng.integers(3, TIE_W)), int(rng.integers(4, TIE_H))
        if all(abs(x - sx) > 8 or abs(y - sy) > 8 for sx, sy in near):
            a[y, x] = b[y - 4, x - 3] = True
    return _pack([(0, 0, a)]), _pack([(3, 4, b)])


def large_sets():
    """a: one random 300 x 200 mask, 1000 words: sixteen workgroups; b: twenty pixels in a 400 x 300 bound about it."""
    rng = np.random.default_rng(2203)
    m = np.zeros((300, 400), bool)
    m[rng.integers(0, 300, 20), rng.integers(0, 400, 20)] = True
    return _pack([(37, 11, _random(rng, 200, 300))]), _pack([(-20, -40, m)])


def many_set(n=130):
    """130 random 5 x 5 instances in a 200 x 200 frame."""
    rng = np.random.default_rng(2204)
    return _pack([(int(rng.integers(-10, 190)), int(rng.integers(-10, 190)), _random(rng, 5, 5, 0.6)) for _ in range(n)])


def extreme_sets(reach=16000):
    """Single pixels at (-reach, -reach) and (reach, reach)."""
    one = np.ones((1, 1), bool)
    return _pack([(-reach, -reach, one)]), _pack([(reach, reach, one)])


def hollow_sets():
    """Either side holds an instance without rows, one with rows and no bit, and real ones."""
    rng = np.random.default_rng(2205)
    a = MI.pack([[0, 0, -1, -1], [3, 3, 70, 6], [5, 5, 40, 20], [7, 2, 6, 9]],
                [np.zeros((0, 0), bool), np.zeros((4, 68), bool), _random(rng, 16, 36), np.zeros((8, 0), bool)], None, None, True)
    b = MI.pack([[20, 1, 90, 30], [0, 0, -1, -1], [1, 1, 64, 2]],
                [_random(rng, 30, 71), np.zeros((0, 0), bool), np.zeros((2, 64), bool)], None, None, True)
    return a, b


def empty_set():
    return PackedMasks(np.zeros((0, 4), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), None, None, np.zeros(0, np.uint64))


def _same_set():
    pm = word_edges_set()
    return pm, pm


def _many():
    pm = many_set()
    return pm, pm


CASES = {"word_edges": (_same_set, word_edges_pairs), "sectors": (sectors_sets, None), "far": (far_sets, None),
         "empty_rows": (empty_rows_sets, None), "ring": (ring_sets, None), "ties": (tie_sets, None), "large": (large_sets, None),
         "many130": (_many, None), "extreme": (extreme_sets, None), "hollow": (hollow_sets, None)}
_cache = {}


def get(name):
    """-> (a, b, pairs or None) of a case, made once."""
    if name not in _cache:
        make, pairs = CASES[name]
        a, b = make()
        _cache[name] = (a, b, pairs() if pairs else None)
    return _cache[name]


def stats_ref(name):
    key = ("stats", name)
    if key not in _cache:
        a, b, pairs = get(name)
        _cache[key] = SF.surface_stats_numpy(a, b, pairs, TAU2)
    return _cache[key]


def dist_ref(name):
    key = ("dist", name)
    if key not in _cache:
        a, b, pairs = get(name)
        _cache[key] = SF.surface_distances_numpy(a, b, pairs)
    return _cache[key]


def same_fields(got, want):
    """Two results of one class: every field equal in dtype, shape and value."""
    return type(got) is type(want) and all(
        isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def same_set(got, want):
    """Two PackedMasks: every field equal in dtype, shape and value."""
    return all(getattr(got, f).dtype == getattr(want, f).dtype and np.array_equal(getattr(got, f), getattr(want, f))
               for f in PackedMasks.FIELDS)
