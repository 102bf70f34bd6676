"""Shared inputs of the rendering tests (tests/test_render_host.py, tests/test_gpu_render.py): a numpy statement of the per-pixel,
order-free rule csrc/render.hip evaluates (the GPU tests' second oracle), the blend rule, and seeded random pred_dicts that
between them reach every corner the kernel has a branch for."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _init_paths  # noqa: F401,E402

S = 21
OUTLINE = 150
# (H, W): the sizes the GPU tests must include (2 x 2, VOC-like, the bench's, one whose width is no multiple of the 64-pixel tile)
BIG_SIZES = [(2, 2), (375, 500), (600, 1000), (100, 130)]
N_RANDOM = 224


def rounded_box(box, W, H):
    b = np.round(np.asarray(box)[:4]).astype(int)
    return (min(max(b[0], 0), W - 1), min(max(b[1], 0), H - 1), min(max(b[2], 0), W - 1), min(max(b[3], 0), H - 1))


def rule_images(img_width, img_height, pred_dict, binarize_thresh=0.4, stats=None):
    """inst, cls by the backward walk: per pixel, cls = 150 if outline_i else class_i if hit_i for the LAST i where either holds,
    inst = i + 1 for the last i with hit_i; the two stop independently.  No instance is painted over another: every pixel is
    decided once.  stats (a dict) receives the largest number of instances hitting one pixel."""
    from utils.blob import resize_to
    W, H = img_width, img_height
    assert W >= 2 and H >= 2
    inst = np.zeros((H, W), int)
    cls = np.zeros((H, W), int)
    done_i = np.zeros((H, W), bool)
    done_c = np.zeros((H, W), bool)
    hits = np.zeros((H, W), int)
    for i in range(len(pred_dict["boxes"]) - 1, -1, -1):
        x1, y1, x2, y2 = rounded_box(pred_dict["boxes"][i], W, H)
        hit = np.zeros((H, W), bool)
        m = resize_to(np.asarray(pred_dict["masks"][i]).astype(np.float32), x2 - x1 + 1, y2 - y1 + 1)
        hit[y1:y2 + 1, x1:x2 + 1] = m >= np.float32(binarize_thresh)
        outline = np.zeros((H, W), bool)
        ys, xs = np.mgrid[0:H, 0:W]
        in_y, in_x = (ys >= y1) & (ys <= y2), (xs >= x1) & (xs <= x2)
        # a numpy slice that starts at -1 is empty: a side at coordinate 0 draws nothing
        if x1 > 0:
            outline |= in_y & (xs >= x1 - 1) & (xs <= x1)
        if x2 > 0:
            outline |= in_y & (xs >= x2 - 1) & (xs <= x2)
        if y1 > 0:
            outline |= in_x & (ys >= y1 - 1) & (ys <= y1)
        if y2 > 0:
            outline |= in_x & (ys >= y2 - 1) & (ys <= y2)
        take_o = outline & ~done_c
        take_h = hit & ~outline & ~done_c
        cls[take_o] = OUTLINE
        cls[take_h] = pred_dict["cls_name"][i]
        done_c |= take_o | take_h
        take_i = hit & ~done_i
        inst[take_i] = i + 1
        done_i |= take_i
        hits += hit
    if stats is not None:
        stats["max_hits"] = int(hits.max()) if hits.size else 0
    return inst, cls


def blend_rule(a, b, alpha):
    """Pillow's blend of two uint8 arrays as the kernel evaluates it: float32 arithmetic, one rounding per operation, truncation."""
    a32, d32 = a.astype(np.float32), (b.astype(np.int32) - a.astype(np.int32)).astype(np.float32)
    prod = (np.float32(alpha) * d32).astype(np.float32)
    return (a32 + prod).astype(np.float32).astype(np.int32).astype(np.uint8)


def _mask(rng, kind):
    yy, xx = np.mgrid[0:S, 0:S]
    if kind == 0:                                  # smooth field around the threshold
        m = 0.5 + 0.5 * np.sin(rng.uniform(0, 6) + rng.uniform(0.1, 0.6) * xx + rng.uniform(0.1, 0.6) * yy)
    elif kind == 1:                                # a disc
        m = (np.hypot(xx - rng.uniform(6, 14), yy - rng.uniform(6, 14)) <= rng.uniform(4, 10)) * rng.uniform(0.5, 1.0)
    elif kind == 2:                                # values exactly at float32(0.4), beside values one ulp below
        m = np.full((S, S), np.float32(0.4), np.float32)
        m[rng.integers(0, S, 40), rng.integers(0, S, 40)] = np.nextafter(np.float32(0.4), np.float32(0))
        m[:, :3] = 0.0
    else:                                          # everything set
        m = np.ones((S, S))
    return m.astype(np.float32)


def random_case(k):
    """-> (W, H, pred_dict, tags): tags names the corners this case was built to reach."""
    rng = np.random.default_rng(7000 + k)
    if k < len(BIG_SIZES):
        H, W = BIG_SIZES[k]
    else:
        H, W = int(rng.integers(2, 70)), int(rng.integers(2, 140))
    n = 0 if k % 37 == 5 else int(rng.integers(1, 10)) if k >= len(BIG_SIZES) else 24
    boxes, masks, classes, tags = [], [], [], set()
    cx, cy = rng.uniform(0, W - 1), rng.uniform(0, H - 1)      # a centre several instances share (overlaps)
    for i in range(n):
        kind = int(rng.integers(0, 9))
        x1, x2 = np.sort(rng.uniform(-8, W + 8, 2))
        y1, y2 = np.sort(rng.uniform(-8, H + 8, 2))
        if kind == 1:
            x1, y1 = 0.0, rng.uniform(0, 0.49)
        elif kind == 2:
            x1, x2 = rng.uniform(-6, -1), rng.uniform(-0.5, 0.49)
        elif kind == 3:
            x1 = x2 = float(rng.integers(0, W))
        elif kind == 4:
            y1 = y2 = float(rng.integers(0, H))
        elif kind == 5:
            x1, x2 = np.floor(x1) + 0.5, np.floor(x2) + 0.5
            y1, y2 = np.floor(y1) + 0.5, np.floor(y2) + 0.5
        elif kind == 6:
            x1, y1, x2, y2 = -5.2, -3.7, W + 4.1, H + 6.3
        elif kind >= 7:
            hw, hh = rng.uniform(1, 30, 2)
            x1, x2, y1, y2 = cx - hw, cx + hw, cy - hh, cy + hh
        tags.add("kind%d" % kind)
        box = np.array([x1, y1, x2, y2, rng.uniform(0.3, 1.0)], np.float32 if rng.integers(0, 2) else np.float64)
        boxes.append(box)
        masks.append(_mask(rng, 3 if kind == 6 and rng.integers(0, 2) else int(rng.integers(0, 4))))
        classes.append(int(rng.integers(1, 21)))
    return W, H, {"image_name": "case%d" % k, "cls_name": classes, "boxes": boxes, "masks": masks}, tags


def coverage(cases):
    """Which corners a list of (W, H, pred_dict, tags) reaches; the tests assert every entry."""
    c = dict.fromkeys(["x1_0", "y1_0", "x2_0", "over_left", "over_top", "over_right", "over_bottom", "one_wide", "one_high",
                       "half", "small", "large", "empty", "at_thresh", "overlap3"], False)
    for W, H, pred, _ in cases:
        if not pred["boxes"]:
            c["empty"] = True
        for box, m in zip(pred["boxes"], pred["masks"]):
            raw = np.asarray(box, np.float64)[:4]
            x1, y1, x2, y2 = rounded_box(box, W, H)
            c["x1_0"] |= x1 == 0
            c["y1_0"] |= y1 == 0
            c["x2_0"] |= x2 == 0
            c["over_left"] |= raw[0] < -0.5
            c["over_top"] |= raw[1] < -0.5
            c["over_right"] |= raw[2] > W - 0.5
            c["over_bottom"] |= raw[3] > H - 0.5
            c["one_wide"] |= x2 == x1
            c["one_high"] |= y2 == y1
            c["half"] |= bool((raw % 1 == 0.5).any())
            c["small"] |= 1 < x2 - x1 + 1 < S
            c["large"] |= x2 - x1 + 1 > S
            c["at_thresh"] |= bool((m == np.float32(0.4)).any())
        st = {}
        if pred["boxes"] and W * H <= 20000:
            rule_images(W, H, pred, stats=st)
            c["overlap3"] |= st["max_hits"] >= 3
    return c


def all_cases():
    return [random_case(k) for k in range(N_RANDOM)]


def class_lists(rng, W, H, vis_thresh, num_classes=21, per_class=(0, 4)):
    """(list_mask, list_box) as gpu_mask_voting returns them (integral boxes | float32 score -> float64), scores on both sides of
    vis_thresh and, in every other class, one exactly at it."""
    list_mask, list_box = [], []
    for c in range(num_classes - 1):
        k = int(rng.integers(per_class[0], per_class[1] + 1))
        b = np.zeros((k, 5), np.float64)
        for j in range(k):
            x = np.sort(rng.integers(0, W, 2))
            y = np.sort(rng.integers(0, H, 2))
            b[j] = (x[0], y[0], x[1], y[1], np.float32(rng.uniform(0, 1)))
        if k and c % 2 == 0:
            b[0, 4] = np.float32(vis_thresh)
        list_box.append(b)
        list_mask.append(np.stack([_mask(rng, int(rng.integers(0, 4))) for _ in range(k)]).reshape(k, 1, S, S) if k
                         else np.zeros((0, 1, S, S), np.float32))
    return list_mask, list_box
