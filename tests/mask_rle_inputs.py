"""Inputs shared by tests/test_mask_rle_host.py and tests/test_gpu_mask_rle.py: small packed mask sets placed where the run-length
encoder can go wrong (widths and heights around the 64-pixel tile, masks that touch the image's top and bottom, bounds that leave
the image, dirty padding), the hand cases of the rule, and a literal scalar transcription of maskApi.c's two string loops."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_overlap_inputs as MI  # noqa: E402  (pack; sets up the reference-shaped import paths)

WIDTHS = [1, 63, 64, 65, 128, 129]
HEIGHTS = [1, 63, 64, 65, 129]

# (rows of the mask, counts, string): worked by hand from the rule
HAND = [
    ([[0, 1], [1, 1], [0, 1]], [1, 1, 1, 3], "1112"),
    ([[1, 1], [1, 1]], [0, 4], "04"),
    ([[0, 0], [0, 0]], [4], "4"),
    ([[0], [0], [0], [1], [1], [0], [1]], [3, 2, 1, 1], "321O"),
    ([[0]] * 16 + [[1]], [16, 1], "`01"),
    ([[0]] * 40 + [[1]] * 2, [40, 2], "X12"),
]


def c_rle_to_string(counts):
    """maskApi.c rleToString, entry by entry and character by character."""
    out = []
    for i, x in enumerate(int(v) for v in counts):
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                           # Python's >> on a negative int is the arithmetic shift
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def c_rle_fr_string(s):
    """maskApi.c rleFrString."""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def whole(masks, classes=None, scores=None, dirty=False):
    """bool [H, W] masks, each with the whole image as its bounds -> PackedMasks."""
    H, W = masks[0].shape
    return MI.pack([[0, 0, W - 1, H - 1]] * len(masks), masks, classes, scores, dirty)


def size_set(H, W, seed=0):
    """Five instances of an H x W image: a random mask over the whole image, a sparser one, a random one in a random sub-box, an
    all-zero and an all-one mask over the whole image."""
    rng = np.random.default_rng(1000 * H + W + seed)
    x = np.sort(rng.integers(0, W, 2))
    y = np.sort(rng.integers(0, H, 2))
    sub = [int(x[0]), int(y[0]), int(x[1]), int(y[1])]
    full = [0, 0, W - 1, H - 1]
    dense = [rng.integers(0, 2, (H, W)).astype(bool), rng.random((H, W)) < 0.1, MI._random_dense(rng, sub), np.zeros((H, W), bool),
             np.ones((H, W), bool)]
    return MI.pack([full, full, sub, full, full], dense)


def checkerboard(n=65):
    yy, xx = np.mgrid[0:n, 0:n]
    return whole([(yy + xx) % 2 == 1, (yy + xx) % 2 == 0])


def column_join(H=65, W=140):
    """Masks whose runs go on from the bottom of one column into the top of the next: pixel (x, H-1) and (x+1, 0) set, bounds at the
    image's top and bottom; the same with the pixel at the top missing (the run then closes at row 0, above a bound that starts
    lower), at a strip boundary (x = 63) and in the image's last column."""
    rng = np.random.default_rng(7)
    bounds, dense = [], []
    for x in (0, 30, 63, W - 2):
        m = np.zeros((H, 2), bool)
        m[H - 1, 0] = m[0, 1] = True
        bounds.append([x, 0, x + 1, H - 1])
        dense.append(m)
        m = rng.integers(0, 2, (H, 2)).astype(bool)
        m[H - 1, 0] = m[0, 1] = True
        bounds.append([x, 0, x + 1, H - 1])
        dense.append(m)
    for x in (5, 63, W - 1):                                  # touches the bottom only: bounds start at row 3
        m = rng.integers(0, 2, (H - 3, 1)).astype(bool)
        m[-1, 0] = True
        bounds.append([x, 3, x, H - 1])
        dense.append(m)
    bounds.append([5, 3, W - 6, H - 1])                       # every column ends set, over the strip boundaries
    dense.append(np.ones((H - 3, W - 10), bool))
    return MI.pack(bounds, dense)


def bottom_rows(H=65, W=140):
    """One- and two-row masks on the image's last rows, several columns wide, each a set of its own: every column whose bottom pixel
    is set closes its run at row 0 of the next column, outside the rows of the bounds -- more runs than the bounds have pixels."""
    rng = np.random.default_rng(13)
    sets = [MI.pack([[10, H - 1, 20, H - 1]], [np.ones((1, 11), bool)]),
            MI.pack([[10, H - 2, 20, H - 1]], [np.ones((2, 11), bool)]),
            MI.pack([[0, H - 1, W - 1, H - 1]], [np.ones((1, W), bool)]),
            MI.pack([[60, H - 1, 70, H - 1]], [np.arange(11).reshape(1, 11) % 2 == 0])]
    b = [[3, H - 1, 130, H - 1], [40, H - 2, 110, H - 1]]
    sets.append(MI.pack(b, [MI._random_dense(rng, q) for q in b]))
    return sets


def leaving(H=70, W=200, dirty=False):
    """Unclipped bounds leaving the H x W image on each side, on all, wholly outside on each side; instances without rows."""
    rng = np.random.default_rng(11)
    bounds = [[-30, 10, 20, 40], [150, 5, W + 40, 60], [20, -25, 90, 30], [30, 40, 100, H + 20], [-5, -5, W + 4, H + 4],
              [-100, 10, -1, 40], [W, 10, W + 70, 40], [10, -50, 80, -1], [10, H, 80, H + 30], [-200, -200, -100, -100],
              [30, 10, 29, 20], [30, 10, 40, 9], [0, 0, W - 1, H - 1], [W - 1, 0, W + 64, H - 1], [-64, H - 1, 0, H + 3]]
    return MI.pack(bounds, [MI._random_dense(rng, b) for b in bounds], dirty=dirty)


def mixed(dirty=False):
    """40 instances of mixed sizes around a 70 x 200 frame."""
    pm = MI.crowded_set()
    if not dirty:
        return pm
    return MI.pack([[int(v) for v in b] for b in pm.bounds], [pm.dense(i) for i in range(len(pm))], pm.classes, pm.scores, True)
