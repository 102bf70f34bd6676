#!/usr/bin/env python3
"""Time the boundary bands of one image's instance masks and the matching on min(mask IoU, boundary IoU) (mnc_amd/boundary.py,
mnc_amd/coco_eval.py; csrc/mask_boundary.hip, csrc/mask_match.hip): the numpy statements (boundary_numpy: unpack, pad, AND the
window, repack; match_boundary_numpy: both sets' bands, two IoU tables, evaluateImg's loop) against the device calls
(PackedMasks.boundary: the sizes-only call and the call with room, host arrays in and out; PackedMasks.match_boundary: one
mnc_mask_match_boundary call, host arrays in, the five tables out) on host PackedMasks, and the device time of the launches alone
between HIP event pairs (mnc_mask_boundary_timing) -- on a 600x1000 and a 375x500 synthetic image at the image's own distance
(23 and 12).  The sets are those of tools/mask_match_bench.py: the 5-stage VGG-16 graph with seeded synthetic weights,
gpu_mask_voting, the --keep best-scoring instances as detections, --gts of them, evenly spaced, as ground truths, every tenth a
crowd; default thresholds and area ranges (T = 10, A = 4), max_det = 100.  Both sides are timed in this process, in this run:
medians over --iters device rounds and --host-iters host rounds after one warm-up each.  Prints one JSON line and writes it, under
a heading, to --profile (default profiles/mask_boundary_bench.txt; "" writes nothing).

    python tools/mask_boundary_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--gts 20] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances


HEADING = """tools/mask_boundary_bench.py --iters %d --host-iters %d on one MI355X: per image, mnc_amd.boundary.boundary_numpy of the %d
best instances against PackedMasks.boundary (mnc_mask_boundary, csrc/mask_boundary.hip: host arrays in and out, the sizes-only call
and the call with room), and mnc_amd.coco_eval.match_boundary_numpy of them against %d synthetic ground truths (evenly spaced
instances themselves, every tenth a crowd; T = 10, A = 4, max_det = 100) against PackedMasks.match_boundary (one
mnc_mask_match_boundary call), on a 600x1000 and a 375x500 synthetic image at d = 23 and 12; kernels_us: the device time of one
call's launches between a HIP event pair (mnc_mask_boundary_timing).  Host and device sides measured in the same process and run.

"""


def main():
    ap = parser()
    ap.add_argument("--gts", type=int, default=20)
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_boundary_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import boundary
    from mnc_amd.coco_eval import match_boundary_numpy
    from mnc_amd.masks import PackedMasks
    timed = lambda fn: kernels_us("mnc_mask_boundary_timing", fn, args.iters)        # noqa: E731 (fn: a single call of one of the two entries)
    sizes = []
    for H, W, _, dt, _ in voted_instances("mask_boundary_bench", args.keep, args.math):
        n, d = len(dt), boundary.boundary_distance(H, W)
        gt = dt.take(np.linspace(0, n - 1, min(args.gts, n)).astype(int))
        crowd = (np.arange(len(gt)) % 10 == 9).astype(np.uint8)
        want_b, got_b = boundary.boundary_numpy(dt, H, W, d), dt.boundary(H, W)                     # (the warm-ups)
        same_b = all(np.array_equal(getattr(want_b, f), getattr(got_b, f)) for f in PackedMasks.FIELDS)
        want_m, got_m = match_boundary_numpy(dt, gt, H, W, crowd, return_iou=True), dt.match_boundary(gt, H, W, crowd, return_iou=True)
        same_m = all(np.array_equal(a, b) for a, b in zip(want_m[0], got_m[0])) and np.array_equal(want_m[1], got_m[1])
        b_host = median_ms(lambda: boundary.boundary_numpy(dt, H, W, d), args.host_iters)
        b_dev = median_ms(lambda: dt.boundary(H, W), args.iters)
        m_host = median_ms(lambda: match_boundary_numpy(dt, gt, H, W, crowd), args.host_iters)
        m_dev = median_ms(lambda: dt.match_boundary(gt, H, W, crowd), args.iters)
        room = np.zeros(max(want_b.bits.size, 1), np.uint64)
        sizes.append({"image": "%dx%d" % (H, W), "d": d, "detections": n, "ground_truths": len(gt), "bits_bytes": int(dt.bits.nbytes),
                      "boundary_bits_bytes": int(want_b.bits.nbytes), "pixels_set": int(dt.areas.sum()),
                      "boundary_pixels": int(want_b.areas.sum()), "matches_at_iou50": int((want_m[0].dt_match[0, 0] >= 0).sum()),
                      "boundary_equals_host": bool(same_b), "match_equals_host": bool(same_m),
                      "boundary_host_ms_median": b_host[0], "boundary_host_ms_min": b_host[1],
                      "boundary_device_ms_median": b_dev[0], "boundary_device_ms_min": b_dev[1],
                      "boundary_kernels_us_median": timed(lambda: boundary.boundary_call(dt, H, W, d, room)),
                      "match_host_ms_median": m_host[0], "match_host_ms_min": m_host[1],
                      "match_device_ms_median": m_dev[0], "match_device_ms_min": m_dev[1],
                      "match_kernels_us_median": timed(lambda: dt.match_boundary(gt, H, W, crowd))})
    emit({"workload": "boundary bands (2 % of the diagonal) of mnc 5-stage vgg16's voted instances at image resolution, "
                      "and COCO matching on min(mask IoU, boundary IoU) against synthetic ground truths",
          "host": "boundary_numpy / match_boundary_numpy on a host PackedMasks",
          "device": "PackedMasks.boundary (two mnc_mask_boundary calls) / PackedMasks.match_boundary (one "
                    "mnc_mask_match_boundary call), host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep, args.gts), args.profile)


if __name__ == "__main__":
    main()
