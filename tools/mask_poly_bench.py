#!/usr/bin/env python3
"""Time the way in from an annotation file: COCO polygon segmentations rasterised into packed masks, in host form
(mnc_amd.polygons.masks_from_polygons_numpy: the walk, the crossings, sort and merge, decode, OR, pack) against device form
(PackedMasks.from_polygons: mnc_mask_from_polygons, csrc/mask_poly.hip, host lists in, host arrays out -- the sizes-only call and
the call with room, as the method makes them), on 20 annotations of 1-3 polygons with 10-60 vertices in a 600x1000 and in a 375x500
image.  "device_sizes_only_ms" is one call without the bits (edge table, copies, the toggle and fill kernels, one read-back);
"kernels_us_median" is the device time of one call with room -- the plane fill and the three kernels between HIP event pairs
(mnc_mask_poly_timing).
Medians over --iters device rounds and --host-iters host rounds after one warm-up each; one JSON line.

    python tools/mask_poly_bench.py [--iters 20] [--host-iters 3]
"""
import argparse
import math

import numpy as np

from _task_harness import emit, kernels_us, median_ms


def annotations(H, W, n=20, seed=0):
    """n annotations of 1-3 polygons, each 10-60 vertices on a wobbling circle around a centre inside the image."""
    rng = np.random.default_rng(seed + H)
    segs = []
    for _ in range(n):
        polys = []
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(10, 61))
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.03, 0.25) * min(H, W)
            a = np.sort(rng.uniform(0, 2 * math.pi, k))
            rad = r * rng.uniform(0.6, 1.0, k)
            polys.append(np.stack((cx + rad * np.cos(a), cy + rad * np.sin(a)), axis=1).reshape(-1).tolist())
        segs.append(polys)
    return segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    args = ap.parse_args()
    from mnc_amd import polygons
    from mnc_amd.masks import PackedMasks
    sizes = []
    for H, W in ((600, 1000), (375, 500)):
        segs = annotations(H, W)
        want = polygons.masks_from_polygons_numpy(segs, H, W)
        got = PackedMasks.from_polygons(segs, H, W)                          # (the warm-up: the workspace is made here)
        same = all(np.array_equal(getattr(want, f), getattr(got, f)) for f in ("bounds", "offsets", "areas", "bits"))
        checked, _, _ = polygons._check_segs("mask_poly_bench", segs, H, W)
        xy, vert_ptr, poly_ptr = polygons._flatten(checked)
        host = median_ms(lambda: polygons.masks_from_polygons_numpy(segs, H, W), args.host_iters)
        dev = median_ms(lambda: PackedMasks.from_polygons(segs, H, W), args.iters)
        first = median_ms(lambda: polygons.masks_from_polygons_call(xy, vert_ptr, poly_ptr, H, W), args.iters)
        room = np.zeros(max(want.bits.size, 1), np.uint64)
        kernels = kernels_us("mnc_mask_poly_timing", lambda: polygons.masks_from_polygons_call(xy, vert_ptr, poly_ptr, H, W, room), args.iters)
        walk = sum(len(polygons.polygon_walk_numpy(p)[0]) for polys in segs for p in polys)
        sizes.append({"image": "%dx%d" % (H, W), "annotations": len(segs), "polygons": int(poly_ptr[-1]), "vertices": int(vert_ptr[-1]),
                      "walk_points": int(walk), "pixels_set": int(want.areas.sum()), "bits_bytes": int(want.bits.nbytes),
                      "device_equals_host": bool(same), "host_ms_median": host[0], "host_ms_min": host[1],
                      "device_ms_median": dev[0], "device_ms_min": dev[1], "device_sizes_only_ms_median": first[0],
                      "device_sizes_only_ms_min": first[1], "kernels_us_median": kernels})
    emit({"workload": "COCO polygon segmentations of one image rasterised into packed masks (maskApi.c's rleFrPoly + merge)",
          "host": "masks_from_polygons_numpy", "device": "PackedMasks.from_polygons: two mnc_mask_from_polygons calls, "
          "host lists in, host arrays out", "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1),
          "sizes": sizes})


if __name__ == "__main__":
    main()
