#!/usr/bin/env python3
"""Time the squared Euclidean distance transform, the inscribed disc and the morphology by a disc of one image's instance masks
(mnc_amd/distance.py; csrc/mask_distance.hip) in four forms: the numpy statements (distance_numpy, inscribed_numpy, morph_numpy);
a scipy loop over dense(i) (scipy.ndimage.distance_transform_edt of the padded mask, its argmax, binary_opening / binary_closing
and binary_dilation with the disc on the array padded by rho) -- what a user writes today, and the yardstick; the device calls
with their copies (PackedMasks.distance / .inscribed / .open + .close / .dilate, host arrays in and out); and the kernels alone
between HIP event pairs (mnc_mask_distance_timing).  The operations: distance, inscribed, open + close at R = 2, dilate at R = 23
(the boundary distance of the 600x1000 image) clipped to the image -- on the --keep best instances of a 600x1000 and a 375x500
synthetic image (the sets of tools/mask_boundary_bench.py).  All sides are timed in this process, in this run: medians over --iters
device rounds and --host-iters host rounds after one warm-up each.  Prints one JSON line and writes it, under a heading, to
--profile (default profiles/mask_distance_bench.txt; "" writes nothing).

    python tools/mask_distance_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import math
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances

SMOOTH_R, DILATE_R = 2, 23

HEADING = """tools/mask_distance_bench.py --iters %d --host-iters %d on one MI355X: per image, on the %d best instances: the squared distance
maps, the inscribed discs, open + close by the disc of radius 2 and the dilation by the disc of radius 23 clipped to the image.
host: the numpy statements of mnc_amd/distance.py.  scipy: the loop over dense(i) a user writes today (distance_transform_edt of
the zero-padded mask; its argmax; binary_opening then binary_closing, and binary_dilation, with the disc on the array padded by
rho) -- the yardstick.  device: PackedMasks.distance / .inscribed / .open + .close / .dilate, host arrays in and out, copies
included (mnc_mask_distance / _inscribed / _morph, csrc/mask_distance.hip).  kernels_us: the device time of the launches alone
between a HIP event pair (mnc_mask_distance_timing; for open + close the sum of the two calls).  All sides measured in the same
process and run.

"""


def _disc(r2):
    rho = math.isqrt(r2)
    yy, xx = np.mgrid[-rho:rho + 1, -rho:rho + 1]
    return yy * yy + xx * xx <= r2, rho


def _scipy_forms(pm, H, W, r2_smooth, r2_dilate):
    """The scipy loops -> {name: callable}, or None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    idx = [i for i in range(len(pm)) if 0 not in pm.size(i)]
    s2, p2 = _disc(r2_smooth)
    s23, p23 = _disc(r2_dilate)

    def edt():
        return [ndimage.distance_transform_edt(np.pad(pm.dense(i), 1))[1:-1, 1:-1] for i in idx]

    def inscribed():
        out = []
        for i in idx:
            d = ndimage.distance_transform_edt(np.pad(pm.dense(i), 1))[1:-1, 1:-1]
            at = int(np.argmax(d))
            out.append((at % d.shape[1], at // d.shape[1], d.reshape(-1)[at]))
        return out

    def smooth():
        out = []
        for i in idx:
            m = np.pad(pm.dense(i), p2)
            out.append(ndimage.binary_closing(ndimage.binary_opening(m, s2), s2)[p2:-p2 or None, p2:-p2 or None])
        return out

    def dilate():
        return [ndimage.binary_dilation(np.pad(pm.dense(i), p23), s23) for i in idx]

    return {"distance": edt, "inscribed": inscribed, "open_close": smooth, "dilate": dilate}


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_distance_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import distance as DT
    from mnc_amd.masks import PackedMasks
    r2s, r2d = DT.radius_sq(SMOOTH_R), DT.radius_sq(DILATE_R)
    timed = lambda fn: kernels_us("mnc_mask_distance_timing", fn, args.iters)        # noqa: E731 (fn: a single call of one entry)
    same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f)) for f in PackedMasks.FIELDS)  # noqa: E731
    sizes = []
    for H, W, _, pm, _ in voted_instances("mask_distance_bench", args.keep, args.math):
        host = {"distance": lambda: DT.distance_numpy(pm), "inscribed": lambda: DT.inscribed_numpy(pm),
                "open_close": lambda: DT.morph_numpy(DT.morph_numpy(pm, "open", r2s), "close", r2s),
                "dilate": lambda: DT.morph_numpy(pm, "dilate", r2d, H, W)}
        device = {"distance": pm.distance, "inscribed": pm.inscribed, "open_close": lambda: pm.open(r2=r2s).close(r2=r2s),
                  "dilate": lambda: pm.dilate(r2=r2d, H=H, W=W)}
        scipy_forms = _scipy_forms(pm, H, W, r2s, r2d)
        want = {k: fn() for k, fn in host.items()}                                   # (the warm-ups)
        got = {k: fn() for k, fn in device.items()}
        equal = {"distance": all(np.array_equal(a, b) for a, b in zip(want["distance"], got["distance"])),
                 "inscribed": all(np.array_equal(a, b) for a, b in zip(want["inscribed"], got["inscribed"])),
                 "open_close": same(want["open_close"], got["open_close"]), "dilate": same(want["dilate"], got["dilate"])}
        # the kernels alone: one entry call each, into buffers with room
        opened = pm.open(r2=r2s)
        room_sq = np.zeros(max(int(want["distance"].dist_ptr[-1]), 1), np.uint32)
        room_s = np.zeros(max(pm.bits.size, 1), np.uint64)
        room_d = np.zeros(max(want["dilate"].bits.size, 1), np.uint64)
        k_open = timed(lambda: DT.morph_call(pm, 2, r2s, 0, 0, room_s))
        k_close = timed(lambda: DT.morph_call(opened, 3, r2s, 0, 0, room_s))
        kernels = {"distance": timed(lambda: DT.distance_call(pm, room_sq)), "inscribed": timed(pm.inscribed),
                   "open_close": None if k_open is None or k_close is None else round(k_open + k_close, 2),
                   "dilate": timed(lambda: DT.morph_call(pm, 1, r2d, H, W, room_d))}
        entry = {"image": "%dx%d" % (H, W), "instances": len(pm), "bits_bytes": int(pm.bits.nbytes),
                 "pixels_of_rows": int(want["distance"].dist_ptr[-1]), "pixels_set": int(pm.areas.sum()),
                 "smooth_r2": r2s, "dilate_r2": r2d, "pixels_changed_by_open_close": int(np.abs(want["open_close"].areas - pm.areas).sum()),
                 "largest_r2": int(want["inscribed"][1].max()) if len(pm) else 0}
        for k in ("distance", "inscribed", "open_close", "dilate"):
            h, d = median_ms(host[k], args.host_iters), median_ms(device[k], args.iters)
            s = median_ms(scipy_forms[k], args.host_iters) if scipy_forms else (None, None)
            entry.update({k + "_equals_host": bool(equal[k]), k + "_host_ms_median": h[0], k + "_host_ms_min": h[1],
                          k + "_scipy_ms_median": s[0], k + "_scipy_ms_min": s[1], k + "_device_ms_median": d[0],
                          k + "_device_ms_min": d[1], k + "_kernels_us_median": kernels[k],
                          k + "_device_faster_than_scipy": None if s[0] is None else bool(d[0] < s[0])})
        sizes.append(entry)
    emit({"workload": "squared Euclidean distance maps, inscribed discs, open + close at R = 2 and dilate at R = 23 of mnc 5-stage "
                      "vgg16's voted instances at image resolution",
          "host": "distance_numpy / inscribed_numpy / morph_numpy on a host PackedMasks",
          "scipy": "a loop of scipy.ndimage over dense(i): distance_transform_edt, binary_opening + binary_closing, binary_dilation",
          "device": "PackedMasks.distance / .inscribed / .open + .close / .dilate, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
