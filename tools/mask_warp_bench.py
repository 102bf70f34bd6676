#!/usr/bin/env python3
"""Time the geometric transforms of one image's instance masks (mnc_amd/warp.py; csrc/mask_warp.hip) in four forms: the numpy
statements (isometry_numpy, warp_numpy); the loop over full(i, H, W) a user writes today -- numpy's fliplr / rot90, Pillow's resize /
transform with NEAREST on H x W arrays, boxes from np.nonzero -- the yardstick; the device calls with their copies
(PackedMasks.fliplr / .rot90 / .resize / .warp_affine, host arrays in and out); and the kernels alone between HIP event pairs
(mnc_mask_warp_timing) -- on the --keep best instances of a 600x1000 and a 375x500 synthetic image (the sets of
tools/mask_boundary_bench.py).  The five cases: fliplr, rot90 by one quarter turn, resize to half and to 1.5 times the size, and
warp_affine by 30 degrees about the centre.  All sides are timed in this process, in this run: medians over --iters device rounds
and --host-iters host rounds after one warm-up each.  For the isometries the loop's boxes and pixel counts are compared with the
device's; Pillow computes its resize and transform in floating point and is a yardstick for time only.  Prints one JSON line and
writes it, under a heading, to --profile (default profiles/mask_warp_bench.txt; "" writes nothing).

    python tools/mask_warp_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances

OPS = ("fliplr", "rot90", "half", "up15", "rot30")

HEADING = """tools/mask_warp_bench.py --iters %d --host-iters %d on one MI355X: per image, on the %d best instances: fliplr(W), rot90(1, H, W),
resize to half (half) and to 1.5 times (up15) the image, and warp_affine by 30 degrees about the centre (rot30).  host: the numpy
statements of mnc_amd/warp.py.  loop: what a user writes today over full(i, H, W) -- np.fliplr / np.rot90, Pillow's resize /
transform(AFFINE) with NEAREST, the tight boxes from np.nonzero -- the yardstick.  device: PackedMasks.fliplr / .rot90 / .resize /
.warp_affine, host arrays in and out, copies included (mnc_mask_isometry / mnc_mask_warp, csrc/mask_warp.hip; a size call that
launches nothing, then one launching call).  kernels_us: the device time of the five launches alone between a HIP event pair
(mnc_mask_warp_timing).  All sides measured in the same process and run.

"""


def _box(m):
    if not m.any():
        return (0, 0, -1, -1)
    ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    return (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))


def _loop_forms(pm, H, W, M_inv):
    """The loops over full(i, H, W) -> {name: callable}; each returns per result its tight box and its pixel count."""
    from PIL import Image
    nearest = getattr(Image, "Resampling", Image).NEAREST
    affine = getattr(Image, "Transform", Image).AFFINE
    n = len(pm)

    def each(fn):
        def run():
            out = []
            for i in range(n):
                m = fn(pm.full(i, H, W))
                out.append((_box(m), int(m.sum())))
            return out
        return run

    def pil(fn):
        return lambda m: np.asarray(fn(Image.fromarray(m.view(np.uint8) * 255))) > 0

    return {"fliplr": each(np.fliplr), "rot90": each(np.rot90),
            "half": each(pil(lambda im: im.resize((W // 2, H // 2), nearest))),
            "up15": each(pil(lambda im: im.resize((W * 3 // 2, H * 3 // 2), nearest))),
            "rot30": each(pil(lambda im: im.transform((W, H), affine, tuple(M_inv.reshape(-1)), nearest)))}


def _clipped_equal(loop, got):
    """The loop's boxes and counts against the device result's: equal where the instances lie inside the image."""
    return all(tuple(int(v) for v in got.bounds[i]) == box and int(got.areas[i]) == count for i, (box, count) in enumerate(loop))


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_warp_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import warp as WP
    from mnc_amd.masks import PackedMasks
    timed = lambda fn: kernels_us("mnc_mask_warp_timing", fn, args.iters)             # noqa: E731 (fn: a single launching call)
    same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f)) for f in PackedMasks.FIELDS)    # noqa: E731
    sizes = []
    for H, W, _, pm, _ in voted_instances("mask_warp_bench", args.keep, args.math):
        pm = pm.fetch()
        a, b = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        M = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]])
        A = np.linalg.inv(M[:, :2])
        M_inv = np.concatenate((A, -A.dot(M[:, 2:])), axis=1)                        # Pillow's AFFINE data: output -> input
        half, up = WP.resize_map(H, W, H // 2, W // 2), WP.resize_map(H, W, H * 3 // 2, W * 3 // 2)
        rot = WP.affine_map(M)
        host = {"fliplr": lambda: WP.isometry_numpy(pm, 2, W - 1, 0), "rot90": lambda: WP.isometry_numpy(pm, *WP.rot90_code(1, H, W)),
                "half": lambda: WP.warp_numpy(pm, *half, window=(0, 0, W // 2 - 1, H // 2 - 1)),
                "up15": lambda: WP.warp_numpy(pm, *up, window=(0, 0, W * 3 // 2 - 1, H * 3 // 2 - 1)),
                "rot30": lambda: WP.warp_numpy(pm, *rot, window=(0, 0, W - 1, H - 1))}
        device = {"fliplr": lambda: pm.fliplr(W), "rot90": lambda: pm.rot90(1, H, W), "half": lambda: pm.resize(H, W, H // 2, W // 2),
                  "up15": lambda: pm.resize(H, W, H * 3 // 2, W * 3 // 2), "rot30": lambda: pm.warp_affine(M, H, W)}
        loops = _loop_forms(pm, H, W, M_inv)
        want = {k: fn() for k, fn in host.items()}                                   # (the warm-ups)
        got = {k: fn() for k, fn in device.items()}
        inside = bool((pm.bounds[:, :2] >= 0).all() and (pm.bounds[:, 2] < W).all() and (pm.bounds[:, 3] < H).all())
        entry = {"image": "%dx%d" % (H, W), "instances": len(pm), "bits_bytes": int(pm.bits.nbytes), "pixels_set": int(pm.areas.sum()),
                 "bounds_inside_image": inside}
        for k in OPS:
            h, d, s = median_ms(host[k], args.host_iters), median_ms(device[k], args.iters), median_ms(loops[k], args.host_iters)
            loop = loops[k]()
            entry.update({k + "_equals_host": bool(same(want[k], got[k])),
                          k + "_loop_equals_device": bool(_clipped_equal(loop, got[k])) if inside and k in ("fliplr", "rot90") else None,
                          k + "_loop_pixels": int(sum(c for _, c in loop)), k + "_device_pixels": int(got[k].areas.sum()),
                          k + "_result_bytes": int(got[k].bits.nbytes), k + "_host_ms_median": h[0], k + "_host_ms_min": h[1],
                          k + "_loop_ms_median": s[0], k + "_loop_ms_min": s[1], k + "_device_ms_median": d[0],
                          k + "_device_ms_min": d[1], k + "_kernels_us_median": timed(device[k]),
                          k + "_device_faster_than_loop": bool(d[0] < s[0])})
        sizes.append(entry)
    emit({"workload": "fliplr, rot90, resize to half and to 1.5 times, warp_affine by 30 degrees of mnc 5-stage vgg16's voted instances "
                      "at image resolution",
          "host": "isometry_numpy / warp_numpy on a host PackedMasks",
          "loop": "a loop over full(i, H, W): np.fliplr / np.rot90, Pillow's resize / transform with NEAREST, tight boxes from np.nonzero",
          "device": "PackedMasks.fliplr / .rot90 / .resize / .warp_affine, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
