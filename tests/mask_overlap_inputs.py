"""Inputs shared by tests/test_mask_overlaps_host.py and tests/test_gpu_mask_overlaps.py: packed mask sets made from dense
masks without going through the resize (so that every bound, width and bit is chosen here), the hand-made NMS cases, and an
independent statement of the overlap on a painted canvas."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_inputs as RI  # noqa: E402,F401  (sets up the reference-shaped import paths)
from mnc_amd.masks import PackedMasks  # noqa: E402

H, W = 70, 200                                   # the frame the edge sets are placed around (bounds may leave it)
WIDTHS = [1, 63, 64, 65, 128, 129]
DELTAS = [0, 1, 31, 63, -1, -31, -63, 64, -65]   # ax1 - bx1: every residue of {0, 1, 31, 63} mod 64, both signs


def pack(bounds, dense, classes=None, scores=None, dirty=False):
    """bounds [n][4], dense: bool [h, w] per instance ((h, 0) or (0, w) for one without rows) -> PackedMasks; areas are the true
    counts.  dirty: every padding bit (columns >= w of the last word of a row) is set to 1."""
    offsets, areas, words, at = [], [], [], 0
    for b, m in zip(bounds, dense):
        h, w = max(b[3] - b[1] + 1, 0), max(b[2] - b[0] + 1, 0)
        assert m.shape == (h, w) or h * w == 0
        offsets.append(at)
        areas.append(int(m.sum()) if h * w else 0)
        if h * w == 0:
            continue
        rows = np.zeros((h, (w + 63) // 64 * 8), np.uint8)
        rows[:, :(w + 7) // 8] = np.packbits(m, axis=1, bitorder="little")
        rows = rows.reshape(-1).view(np.uint64).reshape(h, -1).copy()
        if dirty and w % 64:
            rows[:, -1] |= np.uint64(2 ** 64 - 2 ** (w % 64))
        words.append(rows.reshape(-1))
        at += rows.size * 8
    bits = np.concatenate(words) if words else np.zeros(0, np.uint64)
    return PackedMasks(np.array(bounds, np.int32).reshape(-1, 4), offsets, areas, classes, scores, bits)


def _random_dense(rng, b):
    h, w = max(b[3] - b[1] + 1, 0), max(b[2] - b[0] + 1, 0)
    return rng.integers(0, 2, (h, w)).astype(bool)


def edge_boxes():
    """-> (A bounds, B bounds).  All pairs of the two lists are compared, so every width of A meets every horizontal offset of
    B; the named rectangles follow."""
    rng = np.random.default_rng(41)
    A, B = [], []
    for w in WIDTHS:                                                      # A: every width at x1 = 40
        y1 = int(rng.integers(0, 30))
        A.append([40, y1, 40 + w - 1, y1 + int(rng.integers(0, 30))])
    for d in DELTAS:                                                      # B: x1 = 40 - d, three widths each
        for w in (1, 65, 129):
            y1 = int(rng.integers(0, 30))
            B.append([40 - d, y1, 40 - d + w - 1, y1 + int(rng.integers(0, 30))])
    big, small = [10, 5, 150, 60], [50, 20, 60, 30]
    A += [big, small, [10, 5, 50, 20]]                                   # one wholly inside the other, in both orders
    B += [small, big,
          [20, 20, 60, 40],                                               # shares exactly row 20 with (10, 5, 50, 20)
          [50, 0, 90, 30],                                                # ... exactly column 50
          [50, 20, 80, 50],                                               # ... exactly pixel (50, 20)
          [51, 5, 80, 20], [10, 21, 50, 30]]                              # adjacent to it, disjoint
    both = [[-30, -10, 20, 15], [150, 50, 260, 90], [-5, -5, W + 4, H + 4]]      # negative coordinates, past the image, around it
    A += both
    B += both
    A.append([30, 10, 29, 20])                                            # an instance without rows
    B.append([30, 10, 40, 9])
    return A, B


def edge_sets(dirty=False):
    """-> (A, B) PackedMasks over edge_boxes(): random masks, the last three of `both` identical in A and B (IoU exactly 1.0 with
    themselves), one all-zero mask in each set."""
    rng = np.random.default_rng(43)
    ba, bb = edge_boxes()
    da, db = [_random_dense(rng, b) for b in ba], [_random_dense(rng, b) for b in bb]
    for b in ([-30, -10, 20, 15], [150, 50, 260, 90], [-5, -5, W + 4, H + 4]):
        db[bb.index(b)] = da[ba.index(b)].copy()
    da[1][:] = False                                                      # all-zero masks: against each other the union is 0
    db[1][:] = False
    db[2][:] = False
    ca, cb = rng.integers(1, 4, len(ba)), rng.integers(1, 4, len(bb))
    sa, sb = rng.uniform(0, 1, len(ba)).astype(np.float32), rng.uniform(0, 1, len(bb)).astype(np.float32)
    return pack(ba, da, ca, sa, dirty), pack(bb, db, cb, sb, dirty)


def crowded_set(n=40, seed=47):
    """Many overlapping instances with few distinct scores and classes: blobs around a handful of centres."""
    rng = np.random.default_rng(seed)
    bounds, dense = [], []
    for i in range(n):
        cx, cy = [(50, 30), (120, 35), (90, 20)][i % 3]
        x1, y1 = cx - int(rng.integers(10, 40)), cy - int(rng.integers(5, 25))
        x2, y2 = cx + int(rng.integers(10, 70)), cy + int(rng.integers(5, 25))
        yy, xx = np.mgrid[y1:y2 + 1, x1:x2 + 1]
        m = ((xx - cx) / float(rng.integers(8, 60))) ** 2 + ((yy - cy) / float(rng.integers(4, 22))) ** 2 <= 1.0
        bounds.append([x1, y1, x2, y2])
        dense.append(m)
    scores = (rng.integers(0, 12, n) / 12.0).astype(np.float32)          # ties: the stable order matters
    return pack(bounds, dense, rng.integers(1, 4, n), scores)


def nms_cases():
    """{name: PackedMasks}: the hand-made cases of the mask NMS."""
    rng = np.random.default_rng(53)
    m = rng.integers(0, 2, (9, 70)).astype(bool)
    m[0, 0] = True
    box = [3, 4, 72, 12]
    far = [100, 40, 100 + 69, 48]
    one = np.ones((1, 1), bool)
    return {
        "three_identical": pack([box] * 3, [m] * 3, [1, 1, 1], [0.3, 0.9, 0.5]),
        "tie": pack([box, box, far, box], [m, m, m, m], [1, 1, 1, 1], [0.5, 0.5, 0.5, 0.5]),
        # inter = 1, union = 2: IoU exactly 0.5
        "half": pack([[0, 0, 0, 0], [0, 0, 1, 0]], [one, np.ones((1, 2), bool)], [1, 1], [0.9, 0.8]),
        "classes": pack([box] * 3, [m] * 3, [1, 2, 1], [0.9, 0.8, 0.7]),
    }


def canvas_counts(a, b):
    """The overlap stated once more, without slicing one box by the other: both masks painted onto a canvas that holds all
    bounds, & and | counted there.  -> (inter, union) int64 [na, nb]."""
    allb = np.concatenate((a.bounds, b.bounds)).astype(np.int64)
    x0, y0 = int(allb[:, 0].min()), int(allb[:, 1].min())
    cw, ch = int(allb[:, 2].max()) - x0 + 1, int(allb[:, 3].max()) - y0 + 1

    def paint(pm, i):
        c = np.zeros((max(ch, 1), max(cw, 1)), bool)
        h, w = pm.size(i)
        if h and w:
            x1, y1 = int(pm.bounds[i][0]) - x0, int(pm.bounds[i][1]) - y0
            c[y1:y1 + h, x1:x1 + w] = pm.dense(i)
        return c

    pa, pb = [paint(a, i) for i in range(len(a))], [paint(b, j) for j in range(len(b))]
    inter, union = np.zeros((len(a), len(b)), np.int64), np.zeros((len(a), len(b)), np.int64)
    for i in range(len(a)):
        for j in range(len(b)):
            inter[i, j], union[i, j] = (pa[i] & pb[j]).sum(), (pa[i] | pb[j]).sum()
    return inter, union
