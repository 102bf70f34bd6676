#!/usr/bin/env python3
"""Time the simplification of one image's mask outlines to a pixel tolerance (mnc_amd/contours.py; csrc/contour_simplify.hip): the
numpy statement (simplify_numpy: a sequential Douglas-Peucker per loop in Python integers -- the loop over Contours.loop(l) the entry
removes) against the device call (Contours.simplify: host arrays in and out, its copies included), and the device time of the
launches alone between a HIP event pair (mnc_contours_simplify_timing; the copies and the read-back of V' lie outside the pair) --
on the outlines of the --keep best instances of a 600x1000 and a 375x500 synthetic image (the sets of tools/mask_contours_bench.py,
connectivity 8) and on the 600-tooth comb, one loop whose recursion is hundreds deep.  PackedMasks.contours(), the call that feeds
the simplification, is timed on the same sets in the same run.  Medians over --iters device rounds and --host-iters host rounds after
one warm-up each.  Prints one JSON line and writes it, under a heading, to --profile (default profiles/contours_simplify_bench.txt;
"" writes nothing).

    python tools/contours_simplify_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--epsilon 1.0] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances

LAUNCHES = 5                    # cs_wave, cs_block, scan_tiles, scan_top (csrc/scan.hip), cs_write (csrc/contour_simplify.hip: cs_launch)

HEADING = """tools/contours_simplify_bench.py --iters %d --host-iters %d --epsilon %g on one MI355X: per image, the outlines (connectivity 8) of the
%d best instances as a host Contours; mnc_amd.contours.simplify_numpy (a sequential Douglas-Peucker per loop in Python integers)
against Contours.simplify (mnc_contours_simplify, csrc/contour_simplify.hip: host arrays in and out, one call), on a 600x1000 and a
375x500 synthetic image and on the 600-tooth comb (one loop, a split per tooth); kernels_us: the device time of the call's one
memset and five launches between a HIP event pair (mnc_contours_simplify_timing), the copies and the read-back of V' outside it;
launches: the kernel launches of a call, the same whatever the data; contours_*: PackedMasks.contours() of the same set in the same
run.  Host and device sides measured in the same process and run.

"""


def comb(teeth=600):
    """One instance of 2 * teeth x teeth pixels: a bottom row and a tooth on every other column, each a pixel shorter than the one
    before (tests/contour_simplify_inputs.py's)."""
    from mnc_amd.masks import PackedMasks
    m = np.zeros((teeth, 2 * teeth), bool)
    m[-1, :] = True
    for t in range(teeth):
        m[t:, 2 * t] = True
    return PackedMasks.from_dense([[0, 0, 2 * teeth - 1, teeth - 1]], [m])


def measure(name, pm, epsilon, args):
    from mnc_amd import contours as CT
    c = pm.contours(8)
    host, dev = (lambda: CT.simplify_numpy(c, epsilon)), (lambda: c.simplify(epsilon))
    want, got = host(), dev()                                                                      # (the warm-ups)
    h, d, ct = median_ms(host, args.host_iters), median_ms(dev, args.iters), median_ms(lambda: pm.contours(8), args.iters)
    lengths = np.diff(c.vert_ptr)
    return {"set": name, "instances": len(pm), "loops": int(len(c.area)), "loops_up_to_64": int((lengths <= 64).sum()),
            "longest_loop": int(lengths.max()) if len(lengths) else 0, "vertices_in": int(len(c.xy)), "vertices_out": int(len(want.xy)),
            "launches": LAUNCHES, "equals_host": bool(all(np.array_equal(getattr(want, f), getattr(got, f)) for f in CT.SimplifiedContours.FIELDS)),
            "numpy_ms_median": h[0], "numpy_ms_min": h[1], "device_ms_median": d[0], "device_ms_min": d[1],
            "kernels_us_median": kernels_us("mnc_contours_simplify_timing", dev, args.iters),
            "contours_device_ms_median": ct[0], "contours_kernels_us_median": kernels_us("mnc_mask_contours_timing", lambda: pm.contours(8), args.iters)}


def main():
    ap = parser()
    ap.add_argument("--epsilon", type=float, default=1.0)
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "contours_simplify_bench.txt"))
    args = ap.parse_args()
    sizes = [measure("%dx%d" % (H, W), pm, args.epsilon, args) for H, W, _, pm, _ in voted_instances("contours_simplify_bench", args.keep, args.math)]
    sizes.append(measure("comb600", comb(), args.epsilon, args))
    emit({"workload": "outlines (8-connected) of mnc 5-stage vgg16's voted instances simplified to %g px (Douglas-Peucker on closed loops)" % args.epsilon,
          "host": "mnc_amd.contours.simplify_numpy", "device": "Contours.simplify, one call, host arrays in and out", "epsilon": args.epsilon,
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.epsilon, args.keep), args.profile)


if __name__ == "__main__":
    main()
