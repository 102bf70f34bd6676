"""Inputs shared by tests/test_label_pairs_host.py and tests/test_gpu_label_pairs.py: pairs of label maps placed where
csrc/label_pairs.hip can go wrong -- widths around the 64 lanes of a wave and heights of one, two and 65 rows, totals that are no
multiple of the 4 pixels of a lane's 16-byte load and totals below one wave, values at the edges of the presence bitmap's 32-bit
words and at the top of the range in either map, a run that crosses lane, wave and workgroup boundaries, runs of length one, a
million pixels of one pair, tables at and just above the LDS plan's threshold, tables of one row and of one column, non-zero cells
on both sides of a 64-cell ballot and of a 1024-entry scan tile, exactly 2^22 cells and one id more -- and the panoptic scenes
whose scores are known by construction.  Every map is seeded; every reference (the numpy statement of mnc_amd.pairs) is computed
once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_labels_inputs as LI  # noqa: E402  (sets up the import paths)
from mnc_amd import labels as LB  # noqa: E402
from mnc_amd import pairs as PR  # noqa: E402

TOP_ID = 2 ** 24 - 1


def _flat(H, W):
    return np.arange(H * W, dtype=np.int64).reshape(H, W)


def long_runs():
    """1 x 3000: the pair (1, 7) runs over pixels 5 .. 1029, across lanes, waves and the first workgroup's 1024 pixels; (1, 8) over
    1030 .. 2499, across the second's."""
    p = _flat(1, 3000)
    a = np.where(p < 5, 0, np.where(p < 2500, 1, 2))
    b = np.where(p < 1030, 7, 8)
    return a.astype(np.int32), b.astype(np.int32)


def alternating():
    """5 x 130: a alternates with period 2, b with period 3: every run has length 1."""
    p = _flat(5, 130)
    return (p % 2 + 1).astype(np.int32), (p % 3).astype(np.int32)


def one_pair():
    """1024 x 1024 of the single pair (3, 9): 2^20 pixels into one cell."""
    return np.full((1024, 1024), 3, np.int32), np.full((1024, 1024), 9, np.int32)


def lds_edge(extra):
    """128 x 130: a = the row, b = the column modulo 128 -- 128 x 128 cells, exactly pairs.LDS_CELLS, every one of them non-zero;
    extra: one pixel of b renamed to 128, 128 x 129 cells on the same pixels otherwise."""
    assert PR.LDS_CELLS == 128 * 128
    yy, xx = np.mgrid[0:128, 0:130]
    a, b = yy.astype(np.int32), (xx % 128).astype(np.int32)
    if extra:
        b[0, 129] = 128
    return a, b


def straddle():
    """30 x 100: 300 x 300 = 90000 cells, ten of them non-zero per row of the table; row 218 holds cells 65535 and 65536, the two
    sides of a 64-cell ballot and of the scan tile of 1024 ballots."""
    p = _flat(30, 100)
    a = p // 10
    b = (p % 10 + 13 * a + 1) % 300
    return a.astype(np.int32), b.astype(np.int32)


def most_cells(extra):
    """64 x 64: 2048 values in either map, 2^22 cells; extra: one more value in b."""
    p = _flat(64, 64)
    a, b = (p // 2).astype(np.int32), ((p * 7) % 2048).astype(np.int32)
    if extra:
        b[63, 63] = 5000
    return a, b


def shifted(label, dy, dx):
    """(label, label rolled by (dy, dx)): two maps that hold 0 and overlap in most instances."""
    return np.ascontiguousarray(label), np.ascontiguousarray(np.roll(label, (dy, dx), (0, 1)))


def edge_map():
    pm, H, W = LI.sets()["edge"]
    return LB.to_labels_numpy(pm, H, W)


CASES = {
    "tail_3x67": lambda: (LI.patches(3, 67, 6, 201), LI.patches(3, 67, 5, 202)),             # 201 pixels: 50 lanes and one pixel
    "tail_1x1027": lambda: (LI.patches(1, 1027, 6, 203), LI.patches(1, 1027, 5, 204)),       # a second workgroup of three pixels
    "below_a_wave": lambda: (LI.patches(1, 7, 3, 205), LI.patches(1, 7, 2, 206)),
    "words_in_a": lambda: (LI.with_ids([31, 32, 33]), LI.with_ids([5, TOP_ID], 45)),
    "words_in_b": lambda: (LI.with_ids([5, TOP_ID], 45), LI.with_ids([31, 32, 33])),
    "top_in_both": lambda: (LI.with_ids([TOP_ID - 1, TOP_ID]), LI.with_ids([0, TOP_ID], 46)),
    "long_runs": long_runs, "alternating": alternating, "one_pair": one_pair,
    "lds_exact": lambda: lds_edge(False), "lds_above": lambda: lds_edge(True),
    "one_row": lambda: (np.full((9, 70), 4, np.int32), LI.patches(9, 70, 8, 207)),
    "one_column": lambda: (LI.patches(9, 70, 8, 207), np.full((9, 70), 4, np.int32)),
    "straddle": straddle, "most_cells": lambda: most_cells(False),
    "blobs": lambda: shifted(LI.get("blobs"), 3, 5), "edge": lambda: shifted(edge_map(), 1, 2),
    "superpixels": lambda: (LI.get("superpixels_part"), LI.patches(70, 130, 9, 208)),
}
for _w in LI.WIDTHS:
    for _h in LI.HEIGHTS:
        CASES["size_%dx%d" % (_h, _w)] = (lambda h, w: lambda: (LI.patches(h, w, 6, 100 + 7 * h + w), LI.patches(h, w, 5, 300 + 7 * h + w)))(_h, _w)
REFUSED = {"most_cells_plus_one": lambda: most_cells(True)}
SMALL = sorted(k for k in CASES if k.startswith("size_") or k in ("tail_3x67", "below_a_wave", "alternating", "one_row", "one_column"))
_CASES, _REFERENCE = {}, {}


def get(name):
    if name not in _CASES:
        a, b = (CASES[name] if name in CASES else REFUSED[name])()
        a.setflags(write=False)
        b.setflags(write=False)
        _CASES[name] = (a, b)
    return _CASES[name]


def reference(name):
    """label_pairs_numpy of the case, computed once and left unchanged."""
    if name not in _REFERENCE:
        _REFERENCE[name] = PR.label_pairs_numpy(*get(name))
        for f in PR.LabelPairs.FIELDS:
            getattr(_REFERENCE[name], f).setflags(write=False)
    return _REFERENCE[name]


def same_pairs(got, want):
    """Field by field: values, dtype and shape."""
    for f in PR.LabelPairs.FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f
    return True


# ---- semantic maps ----

def class_pair(H=40, W=70, C=21, seed=50):
    """(gt, pred): class maps with values 0 .. C - 1, gt with a border of 255 (ignore)."""
    rng = np.random.default_rng(seed)
    gt = LI.patches(H, W, C - 1, seed) % C
    pred = gt.copy()
    flip = rng.random((H, W)) < 0.2
    pred[flip] = rng.integers(0, C, int(flip.sum()))
    gt = gt.copy()
    gt[0, :] = 255
    gt[:, -1] = 255
    return gt.astype(np.int32), pred.astype(np.int32)


# ---- panoptic scenes ----

CATEGORIES = {1: {"id": 1, "isthing": 1}, 2: {"id": 2, "isthing": 1}, 3: {"id": 3, "isthing": 0}}


def seg(i, c, crowd=0):
    return {"id": int(i), "category_id": int(c), "iscrowd": int(crowd)}


def columns(h, w, spans):
    """int32 [h, w]: spans = [(id, first column, last column)], 0 elsewhere."""
    out = np.zeros((h, w), np.int32)
    for i, x1, x2 in spans:
        out[:, x1:x2 + 1] = i
    return out


def random_scene(seed, H=12, W=17):
    """(gt_map, gt_segments, pred_map, pred_segments): a few rectangles per map over void, categories 1 .. 3, some gt crowd, the
    pred a jittered copy of the gt's rectangles plus strays -- small enough for a brute force over boolean masks."""
    rng = np.random.default_rng(seed)
    gt, pred = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    boxes = []
    for k in range(int(rng.integers(2, 6))):
        h, w = int(rng.integers(2, 7)), int(rng.integers(2, 8))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        gt[y:y + h, x:x + w] = 10 + k
        boxes.append((y, x, h, w, int(rng.integers(1, 4))))
    cats = {}
    for k, (y, x, h, w, c) in enumerate(boxes):
        dy, dx = int(rng.integers(-2, 3)), int(rng.integers(-2, 3))
        y2, x2 = min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)
        pred[y2:y2 + h, x2:x2 + w] = 100 + k
        cats[100 + k] = c
    for k in range(int(rng.integers(0, 3))):
        y, x = int(rng.integers(0, H - 2)), int(rng.integers(0, W - 2))
        pred[y:y + 2, x:x + 3] = 200 + k
        cats[200 + k] = int(rng.integers(1, 4))
    gt_segments = [seg(10 + k, boxes[k][4], int(rng.random() < 0.25)) for k in range(len(boxes)) if (gt == 10 + k).any()]
    if rng.random() < 0.5:
        cats[100] = cats[100] % 3 + 1                                      # a pred of the wrong category
    pred_segments = [seg(i, cats[int(i)]) for i in np.unique(pred) if i != 0]
    return gt, gt_segments, pred, pred_segments
