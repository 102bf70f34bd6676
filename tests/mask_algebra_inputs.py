"""Inputs shared by tests/test_mask_algebra_host.py and tests/test_gpu_mask_algebra.py: pairs of packed mask sets, groups and stacks
placed where csrc/mask_algebra.hip can go wrong -- widths around the 64-column word crossed with column offsets between the operands
that make the funnel shift 0, non-zero and negative, row offsets that overlap and miss, bounds that are disjoint, nested, touching,
without rows or without a pixel, windows that cut at and inside a word, groups of 0 to 200 members, a stack of 65 nested
rectangles, 300 overlapping blobs, and 1025 instances of a few words each.  Every set is seeded; every reference (the numpy
statements of mnc_amd.algebra) is computed once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_overlap_inputs as MI  # noqa: E402  (pack; sets up the reference-shaped import paths)
import mask_boundary_inputs as BI  # noqa: E402  (blob)
from mnc_amd import algebra as AL  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 193]
HEIGHTS = [1, 2, 7, 33]
DXS = [0, 1, 63, 64, 65, 127, -1, -63, -64, -65]
DYS = [0, 1, -1, 40]
BINARY = ("and", "or", "xor", "minus")
OPS = AL.OPS
IMAGE_H, IMAGE_W = 90, 260


def _pack(bounds, dense, dirty=False, scores=None):
    n = len(dense)
    scores = ((np.arange(n) * 7 % n + 1) / (n + 1.0)).astype(np.float32) if scores is None else scores
    return MI.pack(bounds, dense, np.arange(n) % 3 + 1, scores, dirty)


def _sparse(rng, h, w, kind):
    """bool [h, w]: kind 0 a blob that reaches all four sides; 1 random pixels inside a box with an empty margin on every side that
    has room for one (a side of 1 or 2 has none); 2 rows without a set pixel."""
    if kind == 2:
        return np.zeros((h, w), bool)
    if kind == 0:
        return BI.blob(rng, h, w)
    m = np.zeros((h, w), bool)
    y0, y1 = (int(rng.integers(1, (h + 1) // 2)), h - int(rng.integers(1, (h + 1) // 2))) if h >= 3 else (0, h)
    x0, x1 = (int(rng.integers(1, min((w + 1) // 2, 70))), w - int(rng.integers(1, min((w + 1) // 2, 70)))) if w >= 3 else (0, w)
    m[y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < 0.6
    m[y0, x0] = m[y1 - 1, x1 - 1] = True
    return m


def word_pairs(dirty=False):
    """(a, b): 180 pairs.  a's width runs over WIDTHS and b.x1 - a.x1 over DXS, twice; the heights (three in four are 7 or 33, so
    that most masks have room for an empty margin), b's width, b.y1 - a.y1 over DYS and the kind of mask cycle beside them.  a's
    x1 runs from -150 on, so a quarter of the bounds are negative."""
    rng = np.random.default_rng(1700)
    ab, bb, ad, bd = [], [], [], []
    k = 0
    for rep in range(2):
        for wa in WIDTHS:
            for dx in DXS:
                ha, hb = (7, 33, 1, 33, 7, 2, 33, 7)[k % 8], (33, 7, 33, 2, 7, 33, 1, 7)[(k + k // 8) % 8]
                wb = WIDTHS[(k * 5 + 3) % len(WIDTHS)]
                dy = DYS[(k + k // 4 + rep) % 4]
                ax, ay = -150 + 3 * k, -5 + k % 11
                ab.append([ax, ay, ax + wa - 1, ay + ha - 1])
                bb.append([ax + dx, ay + dy, ax + dx + wb - 1, ay + dy + hb - 1])
                ad.append(_sparse(rng, ha, wa, (1, 1, 0, 1, 1, 1, 2)[k % 7]))
                bd.append(_sparse(rng, hb, wb, (1, 1, 1, 0, 1, 1, 1, 2, 1, 1, 1)[k % 11]))
                k += 1
    return _pack(ab, ad, dirty), _pack(bb, bd, dirty)


def relation_pairs():
    """(a, b): bounds that are disjoint, nested either way, touching by one column and by one row, equal; an operand without rows
    ((0, 0, -1, -1), w == 0, h == 0) on either side and on both; an operand with rows and no set pixel on either side."""
    rng = np.random.default_rng(1701)
    none, thin, flat = [0, 0, -1, -1], [30, 4, 29, 20], [30, 4, 90, 3]
    pairs = [([0, 0, 70, 20], [100, 30, 170, 50]),          # disjoint
             ([0, 0, 70, 20], [80, 0, 150, 20]),            # disjoint, the same rows
             ([-10, -10, 140, 30], [20, 0, 90, 12]),        # b inside a
             ([20, 0, 90, 12], [-10, -10, 140, 30]),        # a inside b
             ([0, 0, 64, 20], [64, 5, 130, 25]),            # one column in common
             ([0, 0, 63, 20], [64, 5, 130, 25]),            # side by side
             ([5, 0, 100, 20], [40, 20, 120, 33]),          # one row in common
             ([-70, 3, 60, 30], [-70, 3, 60, 30]),          # equal
             (none, [3, 3, 80, 20]), ([3, 3, 80, 20], none), (none, none), (thin, [3, 3, 80, 20]), ([3, 3, 80, 20], flat),
             ([3, 3, 80, 20], [10, 5, 100, 25]),            # a without a pixel
             ([10, 5, 100, 25], [3, 3, 80, 20])]            # b without a pixel
    ab, bb, ad, bd = [], [], [], []
    for k, (p, q) in enumerate(pairs):
        for box, boxes, dense, blank in ((p, ab, ad, k == 13), (q, bb, bd, k == 14)):
            h, w = max(box[3] - box[1] + 1, 0), max(box[2] - box[0] + 1, 0)
            boxes.append(box)
            dense.append(np.zeros((h, w), bool) if blank or h * w == 0 else rng.random((h, w)) < 0.7)
    return _pack(ab, ad, True), _pack(bb, bd, True)


def broadcast_pair():
    """(a, b) with len(b) == 1: the word pairs' a against one blob of 193 x 33 at (-40, -2)."""
    rng = np.random.default_rng(1702)
    return word_pairs()[0], _pack([[-40, -2, 152, 30]], [BI.blob(rng, 33, 193)], True)


def window_set():
    """Six instances between x = -70 and x = 205 for the windows of WINDOWS, padding bits set."""
    rng = np.random.default_rng(1703)
    bounds = [[0, 0, 199, 29], [-70, -4, 60, 20], [5, 3, 68, 9], [64, 0, 127, 0], [10, 10, 205, 40], [0, 0, -1, -1]]
    dense = [rng.random((max(b[3] - b[1] + 1, 0), max(b[2] - b[0] + 1, 0))) < 0.8 for b in bounds]
    return _pack(bounds, dense, True)


# windows that cut inside a word, at bit 0, at bit 63 and at bit 64 of instance 0, that hold everything, and one pixel
WINDOWS = [(10, 2, 100, 20), (0, 0, 0, 29), (0, 0, 63, 29), (63, 0, 63, 29), (64, 0, 199, 29), (63, 5, 64, 6), (-1000, -1000, 1000, 1000),
           (-64, -4, -1, 3), (128, 29, 128, 29)]
NOT_WINDOWS = [(7, 3, 7, 3), (0, 5, 63, 5), (-3, 2, 61, 4), (0, 0, IMAGE_W - 1, IMAGE_H - 1)]    # 1 x 1, 64 x 1, 65 x 3, an image
FAR_WINDOW = (5000, 5000, 5100, 5100)


def crowd_set():
    """210 blobs of 5 .. 40 pixels a side scattered over 260 x 90 pixels, and five without rows or without a pixel."""
    rng = np.random.default_rng(1704)
    bounds, dense = [], []
    for k in range(215):
        h, w = int(rng.integers(5, 41)), int(rng.integers(5, 41))
        x, y = int(rng.integers(-20, IMAGE_W - 20)), int(rng.integers(-10, IMAGE_H - 10))
        if k % 43 == 42:
            bounds.append([x, y, x - 1, y + h - 1] if k % 2 else [x, y, x + w - 1, y + h - 1])
            dense.append(np.zeros((h, 0 if k % 2 else w), bool))
        else:
            bounds.append([x, y, x + w - 1, y + h - 1])
            dense.append(BI.blob(rng, h, w, 1))
    return _pack(bounds, dense, True)


def crowd_groups():
    """Groups of 0, 1, 2, 64, 65 and 200 members of crowd_set, one with repeats, one in reverse order, one of rowless members."""
    rng = np.random.default_rng(1705)
    pick = lambda k: rng.permutation(215)[:k].tolist()     # noqa: E731
    g64 = pick(64)
    return [[], pick(1), pick(2), g64, pick(65), pick(200), [7, 7, 3, 7, 3, 3], g64[::-1], [42, 85], list(range(214, -1, -1))]


def nested_set(ascending):
    """65 nested rectangles, all ones: rectangle k is the columns k .. 199 - k and the rows k // 4 .. 39 - k // 4, the innermost the
    last.  ascending: the scores rise with k (the innermost is the best), else they fall."""
    bounds = [[k, k // 4, 199 - k, 39 - k // 4] for k in range(65)]
    dense = [np.ones((b[3] - b[1] + 1, b[2] - b[0] + 1), bool) for b in bounds]
    s = (np.arange(65) + 1) / 70.0
    return _pack(bounds, dense, True, (s if ascending else s[::-1]).astype(np.float32))


def nested_areas():
    return np.array([(200 - 2 * k) * (40 - 2 * (k // 4)) for k in range(65)], np.int64)


def blobs_set():
    """300 blobs of 4 .. 40 rows and 4 .. 200 columns over 600 x 300 pixels, scores with ties, some instances without rows."""
    rng = np.random.default_rng(1706)
    bounds, dense = [], []
    for k in range(300):
        h, w = int(rng.integers(4, 41)), int(rng.integers(4, 201))
        x, y = int(rng.integers(-50, 550)), int(rng.integers(-20, 280))
        if k % 60 == 59:
            w = 0
        bounds.append([x, y, x + w - 1, y + h - 1])
        dense.append(BI.blob(rng, h, w, 2) if w else np.zeros((h, 0), bool))
    return _pack(bounds, dense, True, (rng.integers(0, 40, 300) / 40.0).astype(np.float32))


def equal_scores_set():
    """Eight overlapping blobs with one score."""
    rng = np.random.default_rng(1707)
    bounds = [[10 * k, 2 * k, 10 * k + 99, 2 * k + 29] for k in range(8)]
    return _pack(bounds, [BI.blob(rng, 30, 100) for _ in bounds], True, np.full(8, 0.5, np.float32))


def edge_pair():
    """(a, b) with len(a) == 1025 and len(b) == 1, for what is sized by the instances and not by their words: one instance past the
    1024 entries of a scan tile (csrc/scan.h) and past four blocks of 256 lanes of the size kernel (csrc/mask_tight.hip).  a's
    instances have 1 to 3 rows of 1 to 65 columns -- one word a row, two for every fifth -- between x = -30 and x = 235; every
    seventh has no rows, every eleventh of the others no pixel.  b is one blob of 2 x 65."""
    rng = np.random.default_rng(1708)
    bounds, dense = [], []
    for k in range(1025):
        h, w = int(rng.integers(1, 4)), 65 if k % 5 == 4 else int(rng.integers(1, 66))
        x, y = int(rng.integers(-30, 171)), int(rng.integers(-5, 30))
        if k % 7 == 6:
            h, w = (0, 0) if k % 2 else (h, 0)
            x, y = (0, 0) if k % 2 else (x, y)
        bounds.append([x, y, x + w - 1, y + h - 1])
        dense.append(np.zeros((h, w), bool) if k % 7 == 6 or k % 11 == 10 else rng.random((h, w)) < 0.5)
    return _pack(bounds, dense, True), _pack([[40, 8, 104, 9]], [BI.blob(rng, 2, 65)], True)


def empty_set():
    return PackedMasks(np.zeros((0, 4), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), None, None, np.zeros(0, np.uint64))


SETS = {"word": word_pairs, "word_dirty": lambda: word_pairs(True), "relation": relation_pairs, "broadcast": broadcast_pair,
        "window": window_set, "crowd": crowd_set, "nested_up": lambda: nested_set(True), "nested_down": lambda: nested_set(False),
        "blobs": blobs_set, "equal": equal_scores_set, "edge": edge_pair, "empty": empty_set}
_SETS, _REFERENCE = {}, {}


def get(name):
    if name not in _SETS:
        _SETS[name] = SETS[name]()
    return _SETS[name]


def reference(key, make):
    """make() computed once per key and left unchanged."""
    if key not in _REFERENCE:
        _REFERENCE[key] = make()
    return _REFERENCE[key]


def combined(name, op, window=None):
    """combine_numpy of the pair (or, for a single set, of the set alone) of that name."""
    def make():
        s = get(name)
        a, b = s if isinstance(s, tuple) else (s, None)
        return AL.combine_numpy(a, b, op, window)
    return reference((name, "combine", op, window), make)


def same_masks(got, want):
    for f in PackedMasks.FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
    return True


def canonical(pm):
    """What every result must be: offsets in order without gaps and multiples of 8, true areas, zero padding, tight bounds."""
    at = 0
    for i in range(len(pm)):
        h, w = pm.size(i)
        assert pm.offsets[i] == at and at % 8 == 0
        if h * w == 0:
            assert tuple(pm.bounds[i]) == (0, 0, -1, -1) and pm.areas[i] == 0
            continue
        m = pm.dense(i)
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and pm.areas[i] == m.sum()
        words = pm.bits[at // 8:at // 8 + h * ((w + 63) // 64)].reshape(h, -1)
        if w % 64:
            assert not (words[:, -1] >> np.uint64(w % 64)).any()
        at += words.size * 8
    assert pm.bits.size * 8 == at
    return True
