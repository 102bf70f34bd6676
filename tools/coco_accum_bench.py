#!/usr/bin/env python3
"""Time COCO's accumulate -- the match tables of a whole set turned into precision [T, R, K, A, M] and recall [T, K, A, M] -- in
host form (mnc_amd.coco_eval.accumulate: the published loop over class, area range, max_det and image) against device form
(mnc_amd.coco_eval.accumulate_device: the records flattened on the host, then one mnc_coco_accumulate call, csrc/coco_accum.hip),
on synthetic image records of val2017's size made without masks: --images (5000) images of --dets (100) detections and 7 ground
truths, 80 classes, the default 10 thresholds, 4 area ranges, max_dets (1, 10, 100) and 101 recall thresholds.

"host_ms" is accumulate on the first --host-images of the images (all classes), "host_ms_scaled" that time multiplied by images /
host-images: the loop's time grows with images x K x A x M, and the scaling is stated in the output ("host_scaled": true) whenever
it was done.  "device_ms_*" is accumulate_device end to end -- the flattening, the copies both ways, the kernels; "flatten_ms" the
flattening alone; "kernels_ms_median" the device time of one call's launches between a HIP event pair (mnc_coco_accum_timing).
"device_equals_host" compares the tables of the --host-images subset bit for bit.  Medians over --iters rounds after one warm-up;
one JSON line.

    python tools/coco_accum_bench.py [--images 5000] [--dets 100] [--host-images 200] [--iters 5]
"""
import argparse
import time

import numpy as np

from _task_harness import emit, kernels_us, median_ms

CLASSES = 80
GTS = 7


def records(n_images, dets, seed=0):
    """Image records with random tables: scores on 1000 levels (ties across images), about half of the detections matched."""
    from mnc_amd import coco_eval
    rng = np.random.default_rng(seed)
    T, A = len(coco_eval.IOU_THRS), len(coco_eval.AREA_RNGS)
    images = []
    for _ in range(n_images):
        dt_classes = rng.integers(1, CLASSES + 1, dets).astype(np.int32)
        scores = (rng.integers(0, 1000, dets) / 1000.0).astype(np.float32)
        images.append({"dt_classes": dt_classes, "dt_scores": scores, "gt_classes": rng.integers(1, CLASSES + 1, GTS).astype(np.int32),
                       "rank": coco_eval.ranks_numpy(dt_classes, scores),
                       "dt_match": rng.integers(-1, 2, (A, T, dets)).astype(np.int32),
                       "dt_ignore": (rng.random((A, T, dets)) < 0.1).astype(np.uint8),
                       "gt_ignore": (rng.random((A, GTS)) < 0.3).astype(np.uint8)})
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--host-images", type=int, default=200, help="the images accumulate is timed on (its time is scaled to --images)")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    from mnc_amd import coco_eval
    classes = list(range(1, CLASSES + 1))
    images = records(args.images, args.dets)
    part = images[:max(1, min(args.host_images, args.images))]
    t0 = time.perf_counter()
    want = coco_eval.accumulate(part, classes=classes)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = coco_eval.accumulate_device(part, classes=classes)                  # (the warm-up: the workspace is made here)
    same = bool(np.array_equal(got["precision"], want["precision"]) and np.array_equal(got["recall"], want["recall"]))
    coco_eval.accumulate_device(images, classes=classes)                      # (the workspace grows to the full size)
    uniq = np.asarray(classes, np.int64)
    flatten = median_ms(lambda: coco_eval.flatten_records(images, uniq, coco_eval.MAX_DETS), args.iters)
    device = median_ms(lambda: coco_eval.accumulate_device(images, classes=classes), args.iters)
    kernels = kernels_us("mnc_coco_accum_timing", lambda: coco_eval.accumulate_device(images, classes=classes), args.iters)
    scale = len(images) / float(len(part))
    emit({"workload": "COCO accumulate: per-image match tables -> precision [T, R, K, A, M] and recall [T, K, A, M]",
          "images": len(images), "detections": len(images) * args.dets, "ground_truths": len(images) * GTS,
          "classes": CLASSES, "T": 10, "A": 4, "M": 3, "R": 101,
          "host": "accumulate", "host_images": len(part), "host_ms": round(host_ms, 1), "host_scaled": len(part) != len(images),
          "host_ms_scaled": round(host_ms * scale, 1),
          "device": "accumulate_device: flatten_records on the host, one mnc_coco_accumulate call, host arrays in and out",
          "device_rounds": max(args.iters, 1), "device_equals_host": same, "flatten_ms_median": flatten[0],
          "device_ms_median": device[0], "device_ms_min": device[1], "kernels_ms_median": None if kernels is None else round(kernels / 1e3, 3)})


if __name__ == "__main__":
    main()
