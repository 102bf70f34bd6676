"""Inputs shared by tests/test_mask_match_host.py and tests/test_gpu_mask_match.py: detections and ground truths as packed mask
sets in the 70 x 200 frame of mask_overlap_inputs.py, masks of a few pixels to a few hundred -- the hand-made cases of COCO's
matching rule (each a Case: the two sets and the arguments of match_numpy), the sets that make a class's ground truths span more
than one chunk of 64, and the seeded random sets."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_overlap_inputs as MI  # noqa: E402  (sets up the reference-shaped import paths)

H, W = MI.H, MI.W
ALL = [0, 1e10]

Case = collections.namedtuple("Case", "dt gt kw")


def solid(boxes, classes=None, scores=None, dirty=False):
    """Rectangles with every pixel set -> PackedMasks."""
    return MI.pack(boxes, [np.ones((b[3] - b[1] + 1, b[2] - b[0] + 1), bool) for b in boxes], classes, scores, dirty)


def case(dt_boxes, dt_scores, gt_boxes, dt_classes=None, gt_classes=None, **kw):
    dt = solid(dt_boxes, np.ones(len(dt_boxes)) if dt_classes is None else dt_classes, dt_scores)
    gt = solid(gt_boxes, np.ones(len(gt_boxes)) if gt_classes is None else gt_classes)
    kw.setdefault("iscrowd", np.zeros(len(gt_boxes), np.uint8))
    kw.setdefault("iou_thrs", [0.5])
    kw.setdefault("area_rngs", [ALL])
    return Case(dt, gt, kw)


def hand_cases():
    """{name: Case}.  The expected tables are written out in tests/test_mask_match_host.py."""
    B, far = [10, 10, 19, 19], [100, 40, 109, 49]                      # 100 pixels each, disjoint
    five = [[20 * i, 0, 20 * i + 9, 0] for i in range(5)]              # five disjoint rows of 10 pixels
    return collections.OrderedDict([
        # a 2-pixel detection over a 1-pixel ground truth: IoU exactly 0.5 -- matches at t = 0.5, not just above
        ("threshold", case([[0, 0, 1, 0]], [0.9], [[0, 0, 0, 0]], iou_thrs=[0.5, float(np.nextafter(0.5, 1.0))])),
        # two identical ground truths: the higher index first, the next detection gets the other
        ("identical_gts", case([B, B], [0.9, 0.8], [B, B])),
        # ground truth 0 (ignored) equals the detection, ground truth 1 (not ignored) has IoU 6 / 10 with it
        ("not_ignored_wins", case([[0, 0, 9, 0]], [0.9], [[0, 0, 9, 0], [0, 0, 5, 0]], ignore=[1, 0])),
        # a crowd of 100 x 10 pixels; three detections of 100 pixels with 100, 50 and 50 of them inside it
        ("crowd", case([[0, 0, 9, 9], [95, 0, 104, 9], [90, 5, 99, 14]], [0.9, 0.8, 0.7], [[0, 0, 99, 9]], iscrowd=[1])),
        # ignore = 1 without crowd: taken once, the second detection is a false positive
        ("ignore_once", case([B, B], [0.9, 0.8], [B], ignore=[1])),
        # unmatched detections of 100 and 25 pixels against the range [0, 50]
        ("area", case([B, [40, 40, 44, 44]], [0.9, 0.8], [far], area_rngs=[ALL, [0, 50]])),
        # max_det = 3 of five detections, three of them with equal scores; in the second range everything is out of range
        ("max_det", case(five, [0.5, 0.9, 0.5, 0.5, 0.7], five, max_det=3, area_rngs=[ALL, [0, 5]])),
        # class 2 only among the detections, class 3 only among the ground truths, although their masks are equal
        ("classes", case([B, far], [0.9, 0.8], [B, far], dt_classes=[1, 2], gt_classes=[1, 3])),
        ("no_detections", case([], [], [B, far], ignore=[0, 1], area_rngs=[ALL, [0, 50]])),
        ("no_ground_truths", case([B, [40, 40, 44, 44]], [0.8, 0.9], [], area_rngs=[ALL, [0, 50]])),
        ("nothing", case([], [], [])),
    ])


def _blob(rng, x, y, w, h):
    """A random mask in a w x h box at (x, y) with its corners' rows and columns occupied (so that the box is what was asked)."""
    m = rng.random((h, w)) < 0.8
    m[0, 0] = m[-1, -1] = True
    return [x, y, x + w - 1, y + h - 1], m


def chunk_set(n_gt, n_dt, seed):
    """One class (1) with n_gt ground truths -- first in the set, so that their indices are their places in the class's list --
    and n_dt detections, a few of class 2 after them.  Ground truths 63 and 64 are identical (a tie across the chunk boundary,
    with two detections that equal them); the detections are shifted copies of ground truths, some of them exact.  -> Case with
    T = 2, A = 2, max_det = 2048."""
    rng = np.random.default_rng(seed)
    gb, gd = [], []
    for g in range(n_gt):
        b, m = _blob(rng, int(rng.integers(0, W - 24)), int(rng.integers(0, H - 14)), int(rng.integers(2, 24)), int(rng.integers(2, 14)))
        gb.append(b)
        gd.append(m)
    gb[64], gd[64] = list(gb[63]), gd[63].copy()
    db, dd = [], []
    for d in range(n_dt):
        g = int(rng.integers(0, n_gt)) if d > 1 else 63
        dx = int(rng.integers(-1, 2)) if d > 1 else 0
        db.append([gb[g][0] + dx, gb[g][1], gb[g][2] + dx, gb[g][3]])
        dd.append(gd[g].copy())
    extra_b, extra_m = zip(*[_blob(rng, 30 * i, 5, 12, 9) for i in range(4)])
    gt = MI.pack(gb + list(extra_b), gd + list(extra_m), [1] * n_gt + [2] * 4)
    scores = (rng.integers(0, 8, n_dt + 4) / 8.0).astype(np.float32)               # many ties
    dt = MI.pack(db + list(extra_b), dd + list(extra_m), [1] * n_dt + [2] * 4, scores)
    G = n_gt + 4
    crowd = (rng.random(G) < 0.1).astype(np.uint8)
    ignore = (rng.random(G) < 0.1).astype(np.uint8)
    crowd[63:65], ignore[63:65] = 0, 0
    return Case(dt, gt, {"iscrowd": crowd, "ignore": ignore, "iou_thrs": [0.5, 0.75], "area_rngs": [ALL, [0, 120]], "max_det": 2048})


def random_set(seed, n_dt=70, n_gt=30, dirty=False):
    """Three classes, default thresholds and area ranges (T = 10, A = 4), crowd and ignore flags on about a fifth of the ground
    truths, the annotation areas (eval_area) spread over COCO's three ranges.  The crowd regions are large and several detections
    lie in each; most detections are shifted copies of a ground truth of their class.  -> Case."""
    rng = np.random.default_rng(seed)
    gb, gd, gc = [], [], []
    crowd = np.zeros(n_gt, np.uint8)
    for g in range(n_gt):
        crowd[g] = g % 10 == 3
        if crowd[g]:
            b, m = _blob(rng, int(rng.integers(0, 60)), int(rng.integers(0, 20)), int(rng.integers(60, 120)), int(rng.integers(25, 45)))
        else:
            b, m = _blob(rng, int(rng.integers(0, W - 30)), int(rng.integers(0, H - 20)), int(rng.integers(2, 30)), int(rng.integers(2, 20)))
        gb.append(b)
        gd.append(m)
        gc.append(1 + g % 3)
    ignore = (rng.random(n_gt) < 0.12).astype(np.uint8)
    eval_area = rng.choice([200.0, 900.0, 1024.0, 3000.0, 9216.0, 20000.0], n_gt)
    db, dd, dc = [], [], []
    for d in range(n_dt):
        g = int(rng.integers(0, n_gt))
        kind = rng.random()
        if kind < 0.15:                                                            # nowhere near its ground truth
            b, m = _blob(rng, int(rng.integers(0, W - 30)), int(rng.integers(0, H - 20)), int(rng.integers(2, 30)), int(rng.integers(2, 20)))
        elif crowd[g]:                                                             # a piece of the crowd region
            x, y = gb[g][0] + int(rng.integers(0, 40)), gb[g][1] + int(rng.integers(0, 10))
            b, m = _blob(rng, x, y, int(rng.integers(4, 20)), int(rng.integers(4, 14)))
            m &= gd[g][y - gb[g][1]:y - gb[g][1] + m.shape[0], x - gb[g][0]:x - gb[g][0] + m.shape[1]]
            m[0, 0] = m[-1, -1] = True
        else:                                                                      # the ground truth, moved by up to a pixel
            dx, dy = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
            b, m = [gb[g][0] + dx, gb[g][1] + dy, gb[g][2] + dx, gb[g][3] + dy], gd[g].copy()
        db.append(b)
        dd.append(m)
        dc.append(gc[g])
    scores = (rng.integers(0, 40, n_dt) / 40.0).astype(np.float32)
    return Case(MI.pack(db, dd, dc, scores, dirty), MI.pack(gb, gd, gc, None, dirty),
                {"iscrowd": crowd, "ignore": ignore, "eval_area": eval_area})


RANDOM_SEEDS = (101, 102, 103)


def degenerate(m, crowd):
    """What keeps a random set from passing for nothing, counted at (all areas, IoU 0.5) of a match_numpy result -> (matches,
    ignored detections, unmatched detections, the most detections one crowd ground truth was taken by)."""
    dm, di = m.dt_match[0, 0], m.dt_ignore[0, 0]
    taken = max([int((dm == g).sum()) for g in np.flatnonzero(crowd)] + [0])
    return int((dm >= 0).sum()), int((di != 0).sum()), int((dm < 0).sum()), taken
