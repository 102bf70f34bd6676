"""Inputs shared by tests/test_mask_warp_host.py and tests/test_gpu_mask_warp.py: packed mask sets, maps and windows placed where
csrc/mask_warp.hip can go wrong -- widths around the 64-column word crossed with heights around the 64-row block of the transpose,
x1 at negative positions that are no multiple of 64, loose bounds with empty border rows and columns, instances without rows or
without a pixel, translations that move a result across zero, maps with negative coefficients, sources at negative coordinates,
denominators that are and are not powers of two, and windows that cut at and inside a word.  Every set is seeded; every reference
(the numpy statements of mnc_amd.warp) is computed once per key and left unchanged."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_algebra_inputs as AI  # noqa: E402  (_pack, _sparse, same_masks, canonical; sets up the import paths)
import mask_boundary_inputs as BI  # noqa: E402  (blob)
import mask_overlap_inputs as MI  # noqa: E402  (pack)
from mnc_amd import warp as WP  # noqa: E402

WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 193]
HEIGHTS = [1, 2, 7, 33, 64, 65, 130]
BLOCK_SHAPES = [(1, 130), (130, 1), (65, 65), (64, 64)]      # (h, w): the transpose's partial and full blocks
CODES = list(range(8))
# a translation per code that lays an instance of word_set (x from -150 on, y from -5 on) across zero in x, and one in y
SHIFTS = [(-300, -64), (-64, -300), (300, -64), (37, -300), (-300, 64), (-30, 300), (300, 63), (64, 300)]
IMAGES = [(37, 70), (33, 63)]                                # (H, W): neither side a multiple of 64

same_masks, canonical, reference = AI.same_masks, AI.canonical, AI.reference


def word_set(dirty=False):
    """40 instances: every width of WIDTHS with four heights of HEIGHTS (every height five times), then BLOCK_SHAPES.  x1 runs from
    -150 in steps of 37, so it is negative for some and a multiple of 64 for none but by chance; three masks in four have an empty
    margin inside their bounds, one in nine has no pixel at all."""
    rng = np.random.default_rng(1800)
    shapes = [(HEIGHTS[(4 * k + j) % 7], w) for k, w in enumerate(WIDTHS) for j in range(4)] + BLOCK_SHAPES
    bounds, dense = [], []
    for k, (h, w) in enumerate(shapes):
        x, y = -150 + 37 * k, -5 + k % 11
        bounds.append([x, y, x + w - 1, y + h - 1])
        dense.append(AI._sparse(rng, h, w, (1, 1, 0, 1, 1, 1, 0, 1, 2)[k % 9]))
    return AI._pack(bounds, dense, dirty)


def image_set(H, W):
    """Nine instances of an H x W image: blobs inside it, at its corners, across its borders, one of the whole image, one without
    rows and one without a pixel."""
    rng = np.random.default_rng(1801 + H)
    boxes = [[3, 2, 40, 20], [0, 0, 9, 9], [W - 12, H - 7, W - 1, H - 1], [-6, -4, 20, 11], [W - 20, 5, W + 8, H + 3],
             [0, 0, W - 1, H - 1], [0, 0, -1, -1], [10, 10, 30, 25], [W // 2, 0, W // 2, H - 1]]
    dense = []
    for k, b in enumerate(boxes):
        h, w = max(b[3] - b[1] + 1, 0), max(b[2] - b[0] + 1, 0)
        dense.append(np.zeros((h, w), bool) if k == 7 or h * w == 0 else BI.blob(rng, h, w, 2))
    return AI._pack(boxes, dense, True)


def negative_set():
    """Six blobs at negative coordinates, widths and heights on both sides of 64."""
    rng = np.random.default_rng(1802)
    boxes = [[-200, -90, -130, -60], [-64, -64, -1, -1], [-65, -130, 0, -1], [-300, -20, -108, 12], [-10, -200, 53, -71],
             [-129, -7, -129, -7]]
    return AI._pack(boxes, [BI.blob(rng, b[3] - b[1] + 1, b[2] - b[0] + 1, 2) for b in boxes], True)


def rectangle_set():
    """Three rectangles of ones for the closed form of the integer shear."""
    boxes = [[5, 3, 20, 9], [-70, -4, 60, 2], [64, 0, 127, 63]]
    return AI._pack(boxes, [np.ones((b[3] - b[1] + 1, b[2] - b[0] + 1), bool) for b in boxes])


def empty_set():
    return AI.empty_set()


def rotation_matrix(degrees, cx, cy):
    """cv2.getRotationMatrix2D((cx, cy), degrees, 1.0), from its published formula."""
    a, b = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


H0, W0 = IMAGES[0]
ROTATION = rotation_matrix(30.0, 34.25, 17.5)                # about a centre that is no pixel centre
SHEAR = np.array([[1.0, 0.5, -3.2], [0.25, 1.0, 2.7]], np.float64)
NEGATIVE_MAP = ((-3, 1, -500, 2, -5, -420), 7)                # negative coefficients, a denominator that is no power of two
INTEGER_SHEAR = ((1, 2, 0, 0, 1, 0), 1)                      # sx = x + 2 y, sy = y
# windows that hold everything, cut inside a word, at bits 63 / 64, one pixel, and one 64-pixel row
WINDOWS = [(-40, -30, 130, 80), (10, 2, 60, 20), (63, 5, 64, 6), (17, 9, 17, 9), (0, 11, 63, 11), (0, 0, W0 - 1, H0 - 1)]
FAR_WINDOW = (5000, 5000, 5100, 5100)
# (H2, W2) for the resize of an H x W image: integer factors up, odd factors down, the same size, non-integer factors both ways
RESIZES = {(37, 70): [(74, 140), (111, 210), (37, 70), (13, 24), (8, 14), (36, 69), (55, 105), (18, 35), (50, 61), (1, 1)],
           (33, 63): [(66, 126), (11, 21), (33, 63), (49, 94), (20, 100)]}

SETS = {"word": word_set, "word_dirty": lambda: word_set(True), "image0": lambda: image_set(*IMAGES[0]),
        "image1": lambda: image_set(*IMAGES[1]), "negative": negative_set, "rectangle": rectangle_set, "empty": empty_set,
        "edge": lambda: AI.get("edge")[0]}                   # 1025 instances of a few words each
_SETS = {}


def get(name):
    if name not in _SETS:
        _SETS[name] = SETS[name]()
    return _SETS[name]


def maps():
    """{name: (set name, coef, den)}: the gathers both test files run."""
    out = {"rotation16": ("image0",) + WP.affine_map(ROTATION, 16), "rotation10": ("image0",) + WP.affine_map(ROTATION, 10),
           "shear16": ("image0",) + WP.affine_map(SHEAR, 16), "shear10": ("image0",) + WP.affine_map(SHEAR, 10),
           "negative": ("negative",) + NEGATIVE_MAP, "integer_shear": ("rectangle",) + INTEGER_SHEAR}
    return out


def isometry_ref(name, code, tx, ty):
    return reference((name, "isometry", code, tx, ty), lambda: WP.isometry_numpy(get(name), code, tx, ty))


def warp_ref(name, coef, den, window):
    return reference((name, "warp", tuple(coef), den, tuple(window)), lambda: WP.warp_numpy(get(name), coef, den, window))


def brute_force(pm, coef, den, window):
    """The gather pixel by pixel in Python integers -> per instance the set of its destination pixels (x, y)."""
    c0, c1, c2, c3, c4, c5 = (int(v) for v in coef)
    out = []
    for i in range(len(pm)):
        h, w = pm.size(i)
        pixels = set()
        if h and w:
            x1, y1, x2, y2 = (int(v) for v in pm.bounds[i])
            m = pm.dense(i)
            for y in range(window[1], window[3] + 1):
                for x in range(window[0], window[2] + 1):
                    sx, sy = (c0 * x + c1 * y + c2) // den, (c3 * x + c4 * y + c5) // den
                    if x1 <= sx <= x2 and y1 <= sy <= y2 and m[sy - y1, sx - x1]:
                        pixels.add((x, y))
        out.append(pixels)
    return out


def pixels_of(pm):
    """Per instance the set of its pixels (x, y) in image coordinates."""
    out = []
    for i in range(len(pm)):
        h, w = pm.size(i)
        ys, xs = np.nonzero(pm.dense(i)) if h and w else ((), ())
        out.append({(int(x) + int(pm.bounds[i, 0]), int(y) + int(pm.bounds[i, 1])) for x, y in zip(xs, ys)})
    return out


def bound_bytes(frames):
    """The bytes of the loose frames: what *bits_bound must be."""
    return sum((f[3] - f[1] + 1) * ((f[2] - f[0] + 1 + 63) // 64) * 8 for f in frames if f is not None and f[2] >= f[0] and f[3] >= f[1])


def tta_sets():
    """(a, b, W): two sets of an image W wide with a class of its own per instance; b's instances lie apart from a's."""
    rng = np.random.default_rng(1803)
    W = 150
    ab = [[3, 2, 40, 20], [50, 5, 119, 30], [-5, 25, 30, 40]]
    bb = [[125, 3, 149, 20], [60, 35, 140, 44]]

    def make(boxes, first_class):
        n = len(boxes)
        dense = [BI.blob(rng, b[3] - b[1] + 1, b[2] - b[0] + 1, 2) for b in boxes]
        return MI.pack(boxes, dense, np.arange(n) + first_class, ((np.arange(n) * 3 % n + 1) / (n + 1.0)).astype(np.float32), True)
    return make(ab, 1), make(bb, 10), W
