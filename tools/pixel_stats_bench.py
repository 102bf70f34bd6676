#!/usr/bin/env python3
"""Time the pixel statistics and the histograms of an image under packed masks (mnc_amd/pixels.py; csrc/mask_pixels.hip) in four
forms: the numpy statements (pixel_stats_numpy, histogram_numpy); the loop a user writes today -- v = image[pm.full(i, H, W)] per
instance, then its count, sums, minima and maxima, resp. np.bincount per channel -- the yardstick; the device calls with their copies
(PackedMasks.pixel_stats and .histogram, host arrays in and out: the set and the image go up, the figures come back); and the
kernels alone between a HIP event pair (mnc_mask_pixels_timing) -- on the --keep best instances of a 600x1000 and a 375x500
synthetic image (the sets of tools/mask_boundary_bench.py) and that uint8 RGB image itself.  All sides are timed in this process, in
this run: medians over --iters device rounds and --host-iters host rounds after one warm-up each.  The device results are compared
with the statements'; whether each device call beats the loop of the same run is reported, not asserted, and so are what the
upload of the image alone costs (a synchronised host-to-device copy of its bytes, mnc_h2d) as a share of the call, and what the
kernels achieve against the bytes they must read: the image bytes of the instances' frames inside the image plus their words.
Prints one JSON line and writes it, under a heading, to --profile (default profiles/pixel_stats_bench.txt; "" writes nothing).

    python tools/pixel_stats_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances
from mask_labels_bench import upload_ms

HEADING = """tools/pixel_stats_bench.py --iters %d --host-iters %d on one MI355X: per image, pixel_stats (count, sums, extremes and their
positions per instance and channel) and histogram (256 bins per channel) of the uint8 RGB image under the %d best instances of a
600x1000 and a 375x500 synthetic image.  host: the numpy statements of mnc_amd/pixels.py.  loop: what a user writes today -- v =
image[pm.full(i, H, W)] per instance, then v.sum(0), (v * v).sum(0), v.min(0), v.max(0), resp. np.bincount(v[:, c], minlength=256) per
channel -- the yardstick.  device: PackedMasks.pixel_stats / .histogram (mnc_mask_pixel_stats / mnc_mask_histogram), host arrays in and
out, copies included.  kernels_us: the device time of the launches alone between a HIP event pair (mnc_mask_pixels_timing): one launch
each.  image_upload_ms: one synchronised host-to-device copy of the image's bytes, and its share of each call.  must_read_bytes: the
image bytes of the instances' frames inside the image plus the words of those rows; kernels_gb_s: those bytes over the kernels' time.
All sides measured in the same process and run.

"""


def stats_loop(pm, image):
    """The loop over full(i, H, W) -> [(count, sum, sumsq, min, max)]."""
    H, W = image.shape[:2]
    out = []
    for i in range(len(pm)):
        v = image[pm.full(i, H, W)].astype(np.int64)
        out.append((len(v), v.sum(0), (v * v).sum(0), v.min(0), v.max(0)) if len(v) else (0, None, None, None, None))
    return out


def hist_loop(pm, image):
    H, W = image.shape[:2]
    out = np.zeros((len(pm), image.shape[2], 256), np.int64)
    for i in range(len(pm)):
        v = image[pm.full(i, H, W)]
        for c in range(image.shape[2]):
            out[i, c] = np.bincount(v[:, c], minlength=256)
    return out


def must_read(pm, image):
    """The image bytes of the instances' frames inside the image plus the words of those rows."""
    H, W = image.shape[:2]
    total = 0
    for x1, y1, x2, y2 in pm.bounds.tolist():
        ax, ay, bx, by = max(x1, 0), max(y1, 0), min(x2, W - 1), min(y2, H - 1)
        if ax <= bx and ay <= by and x2 >= x1:
            total += (by - ay + 1) * ((bx - ax + 1) * image.shape[2] * image.itemsize + ((x2 - x1) // 64 + 1) * 8)
    return total


def measure(H, W, pm, args):
    from mnc_amd import pixels
    image = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)           # (the image the instances come from)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b) if isinstance(x, np.ndarray))    # noqa: E731
    want_s, got_s, loop_s = pixels.pixel_stats_numpy(pm, image), pm.pixel_stats(image), stats_loop(pm, image)       # (the warm-ups)
    want_h, got_h, loop_h = pixels.histogram_numpy(pm, image), pm.histogram(image), hist_loop(pm, image)
    need = must_read(pm, image)
    entry = {"image": "%dx%d" % (H, W), "instances": len(pm), "set_pixels_in_image": int(got_s.count.sum()),
             "bits_bytes": int(pm.bits.nbytes), "image_bytes": int(image.nbytes), "must_read_bytes": int(need),
             "stats_equals_host": bool(same(got_s, want_s)), "histogram_equals_host": bool(same(got_h, want_h)),
             "stats_loop_equals_device": bool(all(
                 r[0] == got_s.count[i] and (r[0] == 0 or (np.array_equal(r[1], got_s.sum[i]) and np.array_equal(r[2], got_s.sumsq[i])
                                                           and np.array_equal(r[3], got_s.min[i]) and np.array_equal(r[4], got_s.max[i])))
                 for i, r in enumerate(loop_s))),
             "histogram_loop_equals_device": bool(np.array_equal(loop_h, got_h.hist))}
    forms = {"stats": (lambda: pixels.pixel_stats_numpy(pm, image), lambda: stats_loop(pm, image), lambda: pm.pixel_stats(image)),
             "histogram": (lambda: pixels.histogram_numpy(pm, image), lambda: hist_loop(pm, image), lambda: pm.histogram(image))}
    up = upload_ms(image, args.iters)
    entry.update({"image_upload_ms_median": up[0], "image_upload_ms_min": up[1]})
    for k, (host, loop_fn, device) in forms.items():
        h, s, d = median_ms(host, args.host_iters), median_ms(loop_fn, args.host_iters), median_ms(device, args.iters)
        us = kernels_us("mnc_mask_pixels_timing", device, args.iters)
        entry.update({k + "_host_ms_median": h[0], k + "_host_ms_min": h[1], k + "_loop_ms_median": s[0], k + "_loop_ms_min": s[1],
                      k + "_device_ms_median": d[0], k + "_device_ms_min": d[1], k + "_device_faster_than_loop": bool(d[0] < s[0]),
                      k + "_loop_over_device": round(s[0] / d[0], 1) if d[0] else None,
                      k + "_kernels_us_median": us, k + "_kernels_gb_s": round(need / us / 1e3, 1) if us else None,
                      k + "_upload_share_of_call": round(up[0] / d[0], 3) if d[0] else None})
    return entry


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "pixel_stats_bench.txt"))
    args = ap.parse_args()
    sizes = [measure(H, W, pm.fetch(), args) for H, W, _, pm, _ in voted_instances("pixel_stats_bench", args.keep, args.math)]
    emit({"workload": "pixel statistics and 256-bin histograms of a uint8 RGB image under mnc 5-stage vgg16's voted instances",
          "host": "pixel_stats_numpy / histogram_numpy",
          "loop": "v = image[pm.full(i, H, W)] per instance, then sums, minima, maxima resp. np.bincount per channel",
          "device": "PackedMasks.pixel_stats / .histogram, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
