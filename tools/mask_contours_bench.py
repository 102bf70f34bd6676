#!/usr/bin/env python3
"""Time the outlines of one image's instance masks as polygons (mnc_amd/contours.py; csrc/mask_contours.hip): the numpy statement
(contours_numpy: a sequential walk in Python per instance -- the loop over dense(i) the entry removes) against the device call
(PackedMasks.contours: host arrays in and out, its copies included) on host PackedMasks, and the device time of the launches alone
between a HIP event pair (mnc_mask_contours_timing; the read-backs of the edge, loop and vertex totals lie inside the pair) -- on a
600x1000 and a 375x500 synthetic image.  The sets are those of tools/mask_components_bench.py: the 5-stage VGG-16 graph with seeded
synthetic weights, gpu_mask_voting, the --keep best-scoring instances.  8-connectivity.  All sides are timed in this process, in
this run: medians over --iters device rounds and --host-iters host rounds after one warm-up each.  Prints one JSON line and writes
it, under a heading, to --profile (default profiles/mask_contours_bench.txt; "" writes nothing).

    python tools/mask_contours_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances


HEADING = """tools/mask_contours_bench.py --iters %d --host-iters %d on one MI355X: per image, the %d best instances as a host PackedMasks;
mnc_amd.contours.contours_numpy (a sequential walk per instance over dense(i)) against PackedMasks.contours (mnc_mask_contours,
csrc/mask_contours.hip: host arrays in and out, one call) at connectivity 8, on a 600x1000 and a 375x500 synthetic image;
kernels_us: the device time of the call's launches between a HIP event pair (mnc_mask_contours_timing), the read-backs of the
edge, loop and vertex totals inside it; launches: 12 + 2 ceil(log2(edges)) kernels, each waiting for the one before.  Host and
device sides measured in the same process and run.

"""


def _edges(c):
    """The unit edges of all loops: the sides' lengths added up."""
    return int(sum(np.abs(np.roll(c.loop(l), -1, axis=0).astype(np.int64) - c.loop(l)).sum() for l in range(len(c.area))))


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_contours_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import contours as CT
    sizes = []
    for H, W, _, pm, _ in voted_instances("mask_contours_bench", args.keep, args.math):
        host, dev = (lambda: CT.contours_numpy(pm, 8)), (lambda: pm.contours(8))
        want, got = host(), dev()                                                                  # (the warm-ups)
        edges = _edges(want)
        h, d = median_ms(host, args.host_iters), median_ms(dev, args.iters)
        sizes.append({"image": "%dx%d" % (H, W), "instances": len(pm), "bits_bytes": int(pm.bits.nbytes), "pixels_set": int(pm.areas.sum()),
                      "edges": edges, "loops": int(len(want.area)), "holes": int((want.area < 0).sum()), "vertices": int(len(want.xy)),
                      "launches": 12 + 2 * int(np.ceil(np.log2(max(edges, 1)))),
                      "equals_host": bool(all(np.array_equal(getattr(want, f), getattr(got, f)) for f in CT.Contours.FIELDS)),
                      "numpy_ms_median": h[0], "numpy_ms_min": h[1], "device_ms_median": d[0], "device_ms_min": d[1],
                      "kernels_us_median": kernels_us("mnc_mask_contours_timing", dev, args.iters)})
    emit({"workload": "outlines (8-connected) of mnc 5-stage vgg16's voted instances at image resolution as closed polygons",
          "host": "mnc_amd.contours.contours_numpy", "device": "PackedMasks.contours, one call, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
