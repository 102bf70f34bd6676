"""Inputs shared by tests/test_mask_boundary_host.py and tests/test_gpu_mask_boundary.py: packed mask sets placed where
csrc/mask_boundary.hip can go wrong -- widths around the 64-column word crossed with distances below, at and above a word, runs and
holes of 2d - 1 ... 2d + 2 pixels, tall narrow masks that span several blocks of 2d + 1 rows, bounds that leave the image on every
side with unaligned source shifts and dirty padding, one set at real size -- and the hand-made image on which mask IoU and
boundary IoU disagree.  Every reference (mnc_amd.boundary.boundary_numpy) is computed once and shared."""
import collections
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_match_inputs as MM  # noqa: E402  (sets up the reference-shaped import paths)
import render_inputs as RI  # noqa: E402
from mnc_amd import rle  # noqa: E402
from mnc_amd.boundary import boundary_numpy  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MI = MM.MI

WIDTHS = [1, 63, 64, 65, 127, 128, 129, 200]
DISTANCES = [1, 2, 31, 32, 33, 63, 64, 65, 100]
TALL_DISTANCES = [1, 23, 149, 150]
WIDTH_W = 260

Set = collections.namedtuple("Set", "pm H W d")


def blob(rng, h, w, holes=3):
    """A union of rectangles and ellipses in an h x w box with punched holes, its corners' rows and columns occupied."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(3):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(0.2, 0.7) * h + 1, rng.uniform(0.2, 0.7) * w + 1
        if rng.random() < 0.5:
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        else:
            m |= (abs(yy - cy) <= ry * 0.7) & (abs(xx - cx) <= rx * 0.7)
    for _ in range(holes):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = False
    m[0, 0] = m[-1, -1] = True
    return m


def runs(rng, n, d):
    """bool [n]: set runs of 2d + 1, 2d + 2 and 2d pixels parted by holes of 2d - 1, 2d and 2d + 1, from a random phase on."""
    parts = []
    for run, hole in ((2 * d + 1, 2 * d - 1), (2 * d + 2, 2 * d), (2 * d, 2 * d + 1)):
        parts += [np.ones(run, bool), np.zeros(hole, bool)]
    line = np.concatenate(parts * (n // (12 * d + 3) + 2))
    at = int(rng.integers(0, 2 * d + 1))
    return line[at:at + n]


def width_set(d):
    """About 24 instances in a max(90, 2d + 20) x 260 image: per width of WIDTHS a grid of runs and holes around 2d, a blob, and one
    near-full rectangle at least 2d + 3 wide and high, so that something of it survives the erosion (a 90-row image cannot hold a
    window of 2d + 1 rows once d >= 45, and no listed width one of 201 columns: the image grows with d and these rectangles are
    added, the listed widths and distances all stay)."""
    rng = np.random.default_rng(900 + d)
    H, W = max(90, 2 * d + 20), WIDTH_W
    bounds, dense = [], []

    def place(m):
        h, w = m.shape
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        bounds.append([x, y, x + w - 1, y + h - 1])
        dense.append(m)

    for k, w in enumerate(WIDTHS):
        h = min(H, 2 * d + 6 + k)
        grid = runs(rng, h, d)[:, None] & runs(rng, w, d)[None, :]
        grid[0, 0] = grid[-1, -1] = True
        place(grid)
        place(blob(rng, int(rng.integers(20, H + 1)), w))
        full = np.ones((min(H, 2 * d + 3 + k), max(w, 2 * d + 3 + k)), bool)
        full[0, :2] = False                                               # a notch in a corner
        place(full)
    n = len(bounds)
    return Set(MI.pack(bounds, dense, rng.integers(1, 4, n), rng.uniform(0, 1, n).astype(np.float32)), H, W, d)


def tall_set(d):
    """Height 300: two masks 70 wide (a full one and a blob), and one 300 wide, in a 300 x 320 image -- the column pass walks
    several blocks of 2d + 1 rows; at d = 149 a 2 x 2 core of the wide one survives, at d = 150 everything erodes."""
    rng = np.random.default_rng(950 + d)
    wide = np.ones((300, 300), bool)
    wide[150, 0] = False
    bounds = [[5, 0, 74, 299], [131, 0, 200, 299], [13, 0, 312, 299]]
    return Set(MI.pack(bounds, [np.ones((300, 70), bool), blob(rng, 300, 70, 12), wide], [1, 2, 3], [0.5, 0.6, 0.7]), 300, 320, d)


def leaving_set(d=3, dirty=True):
    """A 60 x 150 image: bounds that leave it on each side (the source shifts -x1 mod 64 are 1 and 63, once beyond a word), one
    around it, some wholly outside, instances without rows in the middle of the set; every padding bit of the input set."""
    rng = np.random.default_rng(970)
    H, W = 60, 150
    bounds = [[-1, 5, 80, 40], [-63, 10, 30, 50], [-65, -4, 70, 30], [-127, 20, 20, 70], [100, 10, 170, 40], [20, -9, 90, 20],
              [30, 35, 120, 75], [-5, -5, W + 4, H + 4],
              [40, 10, 39, 20],                                           # no rows
              [-80, 10, -1, 30], [150, 0, 190, 20], [10, -30, 60, -1], [10, 60, 60, 80],      # wholly outside
              [50, 30, 60, 29],                                           # no rows
              [0, 0, W - 1, H - 1], [64, 0, 127, 59], [149, 59, 200, 90]]
    dense = []
    for b in bounds:
        h, w = max(b[3] - b[1] + 1, 0), max(b[2] - b[0] + 1, 0)
        m = rng.random((h, w)) < 0.97 if h * w else np.zeros((h, w), bool)
        if h * w:
            m[h // 4:h // 4 + 2, :] = True
        dense.append(m)
    n = len(bounds)
    return Set(MI.pack(bounds, dense, np.arange(n) % 3 + 1, np.linspace(0.1, 0.9, n), dirty), H, W, d)


def real_set():
    """Ten instances of the 600 x 1000 synthetic image of render_inputs (bounds not clipped) at the image's own distance, 23."""
    from mnc_amd.masks import instance_masks_numpy
    W, H, pred, _ = RI.random_case(RI.BIG_SIZES.index((600, 1000)))
    boxes = np.array([np.asarray(b, np.float64) for b in pred["boxes"][:10]])
    pm = instance_masks_numpy(boxes, np.array(pred["masks"][:10]), H, W, clip=False, binarize_thresh=0.4, classes=pred["cls_name"][:10])
    return Set(pm, H, W, 23)


_REFERENCE = {}


def reference(key, make):
    """(the Set, boundary_numpy of it), computed once per key and left unchanged."""
    if key not in _REFERENCE:
        s = make()
        _REFERENCE[key] = (s, boundary_numpy(s.pm, s.H, s.W, s.d))
    return _REFERENCE[key]


def eroded_areas(s, want):
    """area(E) per instance: the pixels of the cropped mask that are not in its boundary."""
    return np.array([int(s.pm.full(i, s.H, s.W).sum()) - int(want.areas[i]) for i in range(len(s.pm))])


# ---- matching ----

SQ_H, SQ_W, SQ_D = 120, 160, 4                 # boundary_distance(120, 160) = 4


def rounded_square():
    """The image on which the two measures disagree: ground truth a 100 x 100 square at (20, 10); detection 0 the same square with
    its corners rounded off (radius 30) and its right edge 6 columns short; detection 1 the ground truth itself, at a lower score.
    -> Case with T = [0.5, 0.75]."""
    gt = np.ones((100, 100), bool)
    yy, xx = np.mgrid[0:100, 0:100]
    det = np.ones((100, 100), bool)
    r = 30
    for cy, ys in ((r, yy < r), (99 - r, yy > 99 - r)):
        for cx, xs in ((r, xx < r), (99 - r, xx > 99 - r)):
            det &= ~(ys & xs & ((yy - cy) ** 2 + (xx - cx) ** 2 > r * r))
    det[:, 94:] = False
    box = [20, 10, 119, 109]
    dt = MI.pack([box, box], [det, gt], [1, 1], [0.9, 0.8])
    return MM.Case(dt, MI.pack([box], [gt], [1]), {"iscrowd": [0], "iou_thrs": [0.5, 0.75], "area_rngs": [MM.ALL]})


def crowd_case():
    """One crowd ground truth, a 60 x 40 rectangle; one detection, the 20 x 20 square in its top left corner.  At d = 2 the
    detection's band (the frame of width 2, 144 pixels) meets the crowd's band in the two sides they share, 2 * 2 * 20 - 4 = 76
    pixels: boundary IoU 76 / 144 with the crowd's union, mask IoU 400 / 400."""
    dt = MM.solid([[10, 10, 29, 29]], [1], [0.9])
    gt = MM.solid([[10, 10, 69, 49]], [1])
    return MM.Case(dt, gt, {"iscrowd": [1], "iou_thrs": [0.5, 0.55], "area_rngs": [MM.ALL]})


def frame(seed):
    """The random set of mask_match_inputs and an image that covers it."""
    c = MM.random_set(seed)
    return c, MM.H + 10, MM.W + 10


def big_random_set(seed, n_gt=12, n_dt=40):
    """A set on which `segm` and `boundary` disagree: ground truths of 40-90 pixels a side in a 200 x 300 image, three classes,
    crowd and ignore flags; the detections are their ground truth with the contour moved -- eroded or dilated by 1-3 pixels, or
    with a corner cut -- so that the interior keeps the mask IoU high while the band's IoU falls.  -> (Case, H, W, d = 4)."""
    rng = np.random.default_rng(seed)
    H, W, d = 200, 300, 4
    gb, gd, gc = [], [], []
    for g in range(n_gt):
        w, h = int(rng.integers(40, 91)), int(rng.integers(40, 91))
        x, y = int(rng.integers(3, W - w - 3)), int(rng.integers(3, H - h - 3))
        yy, xx = np.mgrid[0:h, 0:w]
        m = ((yy - h / 2.0) / (h / 2.0)) ** 2 + ((xx - w / 2.0) / (w / 2.0)) ** 2 <= 1.0 if g % 2 else np.ones((h, w), bool)
        m[0, 0] = m[-1, -1] = True
        gb.append([x, y, x + w - 1, y + h - 1])
        gd.append(m)
        gc.append(1 + g % 3)
    crowd = (np.arange(n_gt) % 6 == 5).astype(np.uint8)
    ignore = (rng.random(n_gt) < 0.15).astype(np.uint8)
    db, dd, dc = [], [], []
    for k in range(n_dt):
        g = int(rng.integers(0, n_gt))
        m, b = gd[g], gb[g]
        grow = int(rng.integers(-3, 4))
        p = np.pad(m, 3)
        out = p.copy()
        for _ in range(abs(grow)):                                        # one pixel in or out, 4-connected
            q = out if grow > 0 else ~out
            q = q | np.roll(q, 1, 0) | np.roll(q, -1, 0) | np.roll(q, 1, 1) | np.roll(q, -1, 1)
            out = q if grow > 0 else ~q
        if k % 4 == 0:
            out[:int(rng.integers(5, 25)), :int(rng.integers(5, 25))] = False
        out[0, 0] = out[-1, -1] = True
        db.append([b[0] - 3, b[1] - 3, b[2] + 3, b[3] + 3])
        dd.append(out)
        dc.append(gc[g])
    scores = (rng.integers(0, 40, n_dt) / 40.0).astype(np.float32)
    case = MM.Case(MI.pack(db, dd, dc, scores), MI.pack(gb, gd, gc), {"iscrowd": crowd, "ignore": ignore})
    return case, H, W, d


BIG_SEEDS = (301, 302)


def differing(seg, bnd):
    """The detections whose match differs between two Match results, at any area range and threshold."""
    return int((seg.dt_match != bnd.dt_match).any(axis=(0, 1)).sum())


def coco_files(tmp_path):
    """A ground-truth file and a results file over the two big random sets -> (gt path, dt path, the sets)."""
    sets = {"im%d" % s: big_random_set(s) for s in BIG_SEEDS}
    images, anns, results = [], [], []
    for name, (c, H, W, _) in sets.items():
        images.append({"id": name, "height": H, "width": W})
        for i, r in enumerate(rle.mask_rle_numpy(c.gt, H, W)):
            anns.append({"id": len(anns) + 1, "image_id": name, "category_id": int(c.gt.classes[i]), "segmentation": r,
                         "iscrowd": int(c.kw["iscrowd"][i]), "area": float(c.gt.areas[i]), "ignore": int(c.kw["ignore"][i])})
        for i, r in enumerate(rle.mask_rle_numpy(c.dt, H, W)):
            results.append({"image_id": name, "category_id": int(c.dt.classes[i]), "segmentation": r, "score": float(c.dt.scores[i])})
    gt_path, dt_path = str(tmp_path / "gt.json"), str(tmp_path / "dt.json")
    with open(gt_path, "w") as f:
        json.dump({"images": images, "categories": [{"id": k} for k in (1, 2, 3)], "annotations": anns}, f)
    with open(dt_path, "w") as f:
        json.dump(results, f)
    return gt_path, dt_path, sets


def tool(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "tools", "eval_coco.py")] + list(args), capture_output=True, text=True,
                          cwd=REPO)
