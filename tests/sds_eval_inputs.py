"""Inputs and the Python-loop restatement for the SDS evaluation tests (test_sds_eval_host.py, test_gpu_sds_eval.py): a seeded
random case written in tools/test_net.py's on-disk layout (per-class _det.pkl / _seg.pkl, the GT caches of check_voc_sds_cache,
the image list), and the per-prediction best overlap computed with resize_to + mask_overlap as voc_eval_sds does."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _init_paths  # noqa: F401,E402

from datasets.pascal_voc_seg import CLASSES  # noqa: E402

S = 21


def _gt_mask(rng, h, w):
    """An ellipse or a rectangle with holes."""
    Y, X = np.mgrid[0:h, 0:w]
    if rng.random() < 0.5:
        m = ((X - (w - 1) / 2.0) / (w / 2.0)) ** 2 + ((Y - (h - 1) / 2.0) / (h / 2.0)) ** 2 <= 1.0
    else:
        m = np.ones((h, w), bool)
    return m & (rng.random((h, w)) > 0.03)


def _pred_mask(rng):
    yy, xx = np.mgrid[0:S, 0:S]
    cx, cy, r = rng.uniform(6, 14), rng.uniform(6, 14), rng.uniform(4, 12)
    soft = 1.0 - np.hypot(xx - cx, yy - cy) / r + rng.normal(0, 0.2, (S, S))
    return soft >= 0.4                    # the _seg.pkl masks are binarised


def random_case(seed=5, n_images=40, per_image=75):
    """~n_images * per_image predictions over 8 classes.  Classes 1-5 have GT instances (1-5 per image and class, in every
    image but image 0), classes 6-8 have none.  Boxes: jittered GT bounds (reaching past them), random boxes 3-60 px (narrower
    than S) and 60-300 px wide, coordinates at .5 and float64 values no float32 holds.  Scores are rounded to 0.05: many tie."""
    rng = np.random.default_rng(seed)
    names = ["rnd_%03d" % i for i in range(n_images)]
    gt = {c: {} for c in range(1, 21)}
    boxes = [[np.zeros((0, 5)) for _ in names] for _ in range(21)]
    masks = [[np.zeros((0, S, S), bool) for _ in names] for _ in range(21)]
    for ii, name in enumerate(names):
        H, W = int(rng.integers(150, 400)), int(rng.integers(150, 500))
        if ii > 0:
            for c in range(1, 6):
                for _ in range(int(rng.integers(0, 4))):
                    w, h = int(rng.integers(4, min(200, W))), int(rng.integers(4, min(200, H)))
                    x1, y1 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
                    gt[c].setdefault(name, []).append({"mask": _gt_mask(rng, h, w), "mask_cls": c, "already_detect": False,
                                                       "mask_bound": np.array([x1, y1, x1 + w - 1, y1 + h - 1], np.float64)})
        for _ in range(per_image):
            c = int(rng.integers(1, 9))
            insts = gt[c].get(name, []) if c <= 5 else []
            kind = rng.random()
            if insts and kind < 0.6:
                g = insts[int(rng.integers(len(insts)))]
                b, gm = g["mask_bound"], g["mask"]
                bw, bh = b[2] - b[0] + 1, b[3] - b[1] + 1
                box = b + rng.normal(0, 0.03, 4) * np.array([bw, bh, bw, bh])
                iy = (np.arange(S) * gm.shape[0]) // S
                ix = (np.arange(S) * gm.shape[1]) // S
                m = gm[iy][:, ix] ^ (rng.random((S, S)) < 0.02)        # the instance's shape, a few pixels flipped
            else:
                w = rng.uniform(3, 60) if kind < 0.8 else rng.uniform(60, 300)
                h = rng.uniform(3, 300)
                x1, y1 = rng.uniform(-10, W - 3), rng.uniform(-10, H - 3)
                box = np.array([x1, y1, x1 + w, y1 + h])
                m = _pred_mask(rng)
            r = rng.random()
            if r < 0.3:
                box = np.floor(box) + 0.5                       # exact halves: rounding half to even
            elif r < 0.4:
                box = box + 1e-9                                # no float32 holds these
            box[2] = max(box[2], box[0] + 0.6)
            box[3] = max(box[3], box[1] + 0.6)
            score = np.round(rng.random() * 20) / 20.0
            boxes[c][ii] = np.vstack([boxes[c][ii], np.append(box, score)[None]])
            masks[c][ii] = np.concatenate([masks[c][ii], m[None]])
    return {"names": names, "gt": gt, "boxes": boxes, "masks": masks}


def write_case(root, case):
    """root/out/<cls>_det.pkl, <cls>_seg.pkl; root/cache/<cls>_mask_gt.pkl; root/list.txt.  -> (out, cache, list)."""
    out, cache = os.path.join(root, "out"), os.path.join(root, "cache")
    os.makedirs(out, exist_ok=True)
    os.makedirs(cache, exist_ok=True)
    for c, cls in enumerate(CLASSES):
        if c == 0:
            continue
        with open(os.path.join(out, cls + "_det.pkl"), "wb") as f:
            pickle.dump(case["boxes"][c], f, pickle.HIGHEST_PROTOCOL)
        with open(os.path.join(out, cls + "_seg.pkl"), "wb") as f:
            pickle.dump(case["masks"][c], f, pickle.HIGHEST_PROTOCOL)
        with open(os.path.join(cache, cls + "_mask_gt.pkl"), "wb") as f:
            pickle.dump(case["gt"].get(c, {}), f, pickle.HIGHEST_PROTOCOL)
    lst = os.path.join(root, "list.txt")
    with open(lst, "w") as f:
        f.write("".join(n + "\n" for n in case["names"]))
    return out, cache, lst


def cpu_aps(out, cache, lst, thr):
    """voc_eval_sds of every class at one threshold (the CPU evaluator itself; the devkit path is only read when the GT caches
    are missing)."""
    from utils.voc_eval import voc_eval_sds
    with np.errstate(all="ignore"):
        return [voc_eval_sds(os.path.join(out, cls + "_det.pkl"), os.path.join(out, cls + "_seg.pkl"), os.path.dirname(out), lst,
                             cls, cache, CLASSES, ov_thresh=thr) for cls in CLASSES[1:]]


def overlap_terms(gt_bound, pred_box, gt_mask, pred_mask):
    """(inter, union, ov) of mask_overlap(gt_bound, pred_box, gt_mask, pred_mask); ov is mask_overlap's own value."""
    from transform.mask_transform import mask_overlap
    ov = mask_overlap(gt_bound, pred_box, gt_mask, pred_mask)
    area = int(gt_mask.sum()) + int(pred_mask.sum())
    x1, y1 = max(gt_bound[0], pred_box[0]), max(gt_bound[1], pred_box[1])
    x2, y2 = min(gt_bound[2], pred_box[2]), min(gt_bound[3], pred_box[3])
    if x1 > x2 or y1 > y2:
        return 0, area, ov
    a = gt_mask[y1 - gt_bound[1]: y2 - gt_bound[1] + 1, x1 - gt_bound[0]: x2 - gt_bound[0] + 1]
    b = pred_mask[y1 - pred_box[1]: y2 - pred_box[1] + 1, x1 - pred_box[0]: x2 - pred_box[0] + 1]
    inter = int(np.logical_and(a, b).sum())
    return inter, area - inter, ov


def loop_best_overlap(boxes, masks, gt_begin, gt_end, gt_dicts, thresh=0.4):
    """voc_eval_sds's per-prediction loop (resize_to, >= thresh, mask_overlap over the GT range, first strictly greater ov from
    -1000) -> best_gt, best_inter, best_union, best ov (the ov mask_overlap returned)."""
    from utils.blob import resize_to
    P = len(boxes)
    bg = np.full(P, -1, np.int64)
    bi = np.zeros(P, np.int64)
    bu = np.zeros(P, np.int64)
    bo = np.zeros(P)
    for p in range(P):
        pred_box = np.round(boxes[p, :4]).astype(int)
        pm = resize_to(masks[p].reshape(S, S).astype(np.float32), pred_box[2] - pred_box[0] + 1, pred_box[3] - pred_box[1] + 1)
        pm = pm >= thresh
        cur = -1000
        for g in range(gt_begin[p], gt_end[p]):
            gd = gt_dicts[g]
            inter, union, ov = overlap_terms(np.round(gd["mask_bound"]).astype(int), pred_box, gd["mask"], pm)
            if ov > cur:
                cur, bg[p], bi[p], bu[p], bo[p] = ov, g, inter, union, ov
    return bg, bi, bu, bo


def unpack_gt(bounds, offsets, bits):
    """The packed GT rows back to boolean masks."""
    out = []
    for b, o in zip(bounds, offsets):
        w, h = int(b[2] - b[0] + 1), int(b[3] - b[1] + 1)
        rb = (w + 7) // 8
        rows = bits[o: o + h * rb].reshape(h, rb)
        out.append(np.unpackbits(rows, axis=1, bitorder="little")[:, :w].astype(bool))
    return out


def numpy_entry(boxes, masks, gt_begin, gt_end, gt_bounds, gt_offsets, gt_bits, gt_areas, binarize_thresh, device_id=0):
    """A stand-in for voc_eval.sds_best_overlap built from the CPU loop: the GT masks are unpacked from the bit rows, the
    overlaps come from resize_to + mask_overlap."""
    gts = [{"mask": m, "mask_bound": np.asarray(b, np.float64)} for b, m in
           zip(gt_bounds, unpack_gt(gt_bounds, gt_offsets, gt_bits))]
    assert all(int(g["mask"].sum()) == a for g, a in zip(gts, gt_areas))
    bg, bi, bu, _ = loop_best_overlap(np.asarray(boxes), np.asarray(masks), gt_begin, gt_end, gts, binarize_thresh)
    return bg.astype(np.int32), bi, bu
