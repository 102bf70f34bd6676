"""Inputs shared by tests/test_coco_accum_host.py and tests/test_gpu_coco_accum.py: synthetic image records for COCO's accumulate
(mnc_amd.coco_eval.accumulate / accumulate_device, csrc/coco_accum.hip), made directly -- no masks: per image classes, float32
scores quantised to a handful of levels (ties within and across images), ranks_numpy ranks, random dt_match in {-1, 0, 1}, random
ignore flags, random ground-truth classes and gt_ignore.  The cases are sized from the kernel's own constants
(coco_eval.ACCUM_SORT_TILE, ACCUM_SCAN_CHUNK) and keep the image count low: the host oracle's time grows with images x K x A x M."""
import collections
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_match_inputs  # noqa: E402,F401  (sets up the import paths mnc_amd needs)
from mnc_amd import coco_eval  # noqa: E402

TILE, CHUNK = coco_eval.ACCUM_SORT_TILE, coco_eval.ACCUM_SCAN_CHUNK
LEVELS = (0.875, 0.75, 0.5, 0.25, 0.125)
EDGE_LEVELS = (float("inf"), 1.5, 0.5, 0.0, -0.0, -0.5, -2.0, float("-inf"))      # 8 levels, both zeros, both infinities

# kw: the arguments of accumulate / accumulate_device after the images
Case = collections.namedtuple("Case", "images kw")


def record(rng, dt_classes, gt_classes, T, A, levels=LEVELS, p_ignore=0.2, p_gt_ignore=0.3):
    """One image record (the dict of coco_eval.image_record) with random tables."""
    dt_classes, gt_classes = np.asarray(dt_classes, np.int32), np.asarray(gt_classes, np.int32)
    D, G = len(dt_classes), len(gt_classes)
    scores = rng.choice(np.asarray(levels, np.float32), D).astype(np.float32)
    return {"dt_classes": dt_classes, "dt_scores": scores, "gt_classes": gt_classes, "rank": coco_eval.ranks_numpy(dt_classes, scores),
            "dt_match": rng.integers(-1, 2, (A, T, D)).astype(np.int32), "dt_ignore": (rng.random((A, T, D)) < p_ignore).astype(np.uint8),
            "gt_ignore": (rng.random((A, G)) < p_gt_ignore).astype(np.uint8)}


def records(seed, n_images, dt_classes, gt_classes, T=10, A=4, **kw):
    """All detections' classes (dt_classes) and all ground truths' (gt_classes) shuffled and dealt to n_images images."""
    rng = np.random.default_rng(seed)
    dt = np.array_split(rng.permutation(np.asarray(dt_classes, np.int32)), n_images)
    gt = np.array_split(rng.permutation(np.asarray(gt_classes, np.int32)), n_images)
    return [record(rng, d, g, T, A, **kw) for d, g in zip(dt, gt)]


def tiny():
    """(a) 3 images, 2 classes, a dozen detections: small enough to read by eye."""
    images = records(1, 3, [1] * 7 + [2] * 5, [1] * 4 + [2] * 3, T=2, A=1, p_gt_ignore=0.2)
    return Case(images, {"iou_thrs": [0.5, 0.75], "area_rngs": [[0, 1e10]], "max_dets": (1, 3), "classes": [1, 2],
                         "rec_thrs": [0.0, 0.25, 0.5, 0.75, 1.0]})


def chunks():
    """(b) class 1's list spans three scan chunks plus one element, class 2 holds one detection, class 3 exactly one chunk, class
    4 none; 4 images, so that a class's ranks stay below the largest max_det."""
    dt = [1] * (3 * CHUNK + 1) + [2] + [3] * CHUNK
    return Case(records(2, 4, dt, [1] * 40 + [2] * 3 + [3] * 20 + [4] * 5), {"max_dets": (1, 10, 2048), "classes": [1, 2, 3, 4]})


def tiles():
    """(c) N spans three sort tiles plus one key, with the 8 edge score levels only: every tie group crosses tile and image
    boundaries."""
    n = 3 * TILE + 1
    dt = [1] * (n // 2) + [2] * (n // 3) + [3] * (n - n // 2 - n // 3)
    images = records(3, 7, dt, [1] * 30 + [2] * 30 + [3] * 30, T=3, A=2, levels=EDGE_LEVELS)
    return Case(images, {"iou_thrs": [0.5, 0.7, 0.9], "area_rngs": [[0, 1e10], [0, 1024]], "max_dets": (1, 100, 2048),
                         "classes": [1, 2, 3]})


def empty_cells():
    """(d) class 5: ground truths, no detections; class 6: detections, every ground truth ignored; class 7: detections, no ground
    truth; class 9: detections and ground truths of a class that is not evaluated; max_dets 1, 3, 5 with up to a dozen detections
    of a class in an image: ranks at and above each."""
    images = records(4, 5, [1] * 60 + [6] * 20 + [7] * 15 + [9] * 30, [1] * 25 + [5] * 6 + [6] * 8 + [9] * 10, T=2, A=2)
    for im in images:
        im["gt_ignore"][:, im["gt_classes"] == 6] = 1
    return Case(images, {"iou_thrs": [0.5, 0.75], "area_rngs": [[0, 1e10], [0, 1024]], "max_dets": (1, 3, 5), "classes": [1, 5, 6, 7]})


def small_parameters():
    """(e) T = A = M = 1, R = 3 with unsorted recall thresholds."""
    images = records(5, 3, [1] * 90 + [2] * 40, [1] * 20 + [2] * 10, T=1, A=1)
    return Case(images, {"iou_thrs": [0.5], "area_rngs": [[0, 1e10]], "max_dets": (100,), "classes": [1, 2], "rec_thrs": [0.7, 0.1, 0.4]})


def limit_parameters():
    """(e) the limits T = 16, A = 8, M = 8."""
    images = records(6, 3, [1] * 300 + [2] * 150, [1] * 30 + [2] * 20, T=16, A=8)
    return Case(images, {"iou_thrs": np.linspace(0.2, 0.95, 16), "area_rngs": [[0, 10.0 ** (a + 2)] for a in range(8)],
                         "max_dets": (1, 2, 3, 5, 10, 20, 50, 100), "classes": [1, 2]})


CASES = collections.OrderedDict([("tiny", tiny), ("chunks", chunks), ("tiles", tiles), ("empty_cells", empty_cells),
                                 ("small_parameters", small_parameters), ("limit_parameters", limit_parameters)])

_oracle = {}


def oracle(name):
    """-> (Case, accumulate's result), computed once and shared; callers leave it unchanged."""
    if name not in _oracle:
        c = CASES[name]()
        _oracle[name] = (c, coco_eval.accumulate(c.images, **c.kw))
    return _oracle[name]


def flatten_loop(images, classes, max_dets):
    """flatten_records as a plain loop over images and detections."""
    classes = [int(k) for k in classes]
    cls, score, rank, flags, gcls, gig = [], [], [], [], [], []
    for im in images:
        for d in range(len(im["dt_classes"])):
            if im["rank"][d] >= max(max_dets):
                continue
            k = int(im["dt_classes"][d])
            cls.append(classes.index(k) if k in classes else -1)
            score.append(im["dt_scores"][d])
            rank.append(im["rank"][d])
            flags.append((im["dt_match"][:, :, d] >= 0) * 1 + (im["dt_ignore"][:, :, d] != 0) * 2)
        for g in range(len(im["gt_classes"])):
            k = int(im["gt_classes"][g])
            gcls.append(classes.index(k) if k in classes else -1)
            gig.append(im["gt_ignore"][:, g])
    A, T = images[0]["dt_match"].shape[:2]
    return {"dt_class_idx": np.array(cls, np.int32), "dt_score": np.array(score, np.float32), "dt_rank": np.array(rank, np.int32),
            "dt_flags": np.array(flags, np.uint8).reshape(-1, A, T).transpose(1, 2, 0), "gt_class_idx": np.array(gcls, np.int32),
            "gt_ignore": np.array(gig, np.uint8).reshape(-1, A).T}
