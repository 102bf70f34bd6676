#!/usr/bin/env python3
"""Time the moments, the convex hulls and the rectangles of least area of one image's instance masks (mnc_amd/shape.py;
csrc/mask_shape.hip) in four forms: the numpy statements (moments_numpy, hull_numpy, oriented_numpy); the loop over dense(i) a user
writes today -- numpy sums over np.nonzero(dense(i)) for the moments, scipy.spatial.ConvexHull over the corners of the set pixels
for the hull, and the same hull followed by a numpy loop over its edges for the rectangle -- the yardstick; the device calls with
their copies (PackedMasks.moments / .hull / .oriented_boxes, host arrays in and out); and the kernels alone between HIP event pairs
(mnc_mask_shape_timing) -- on the --keep best instances of a 600x1000 and a 375x500 synthetic image (the sets of
tools/mask_boundary_bench.py).  All sides are timed in this process, in this run: medians over --iters device rounds and
--host-iters host rounds after one warm-up each.  Prints one JSON line and writes it, under a heading, to --profile (default
profiles/mask_shape_bench.txt; "" writes nothing).

    python tools/mask_shape_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances

OPS = ("moments", "hull", "oriented")

HEADING = """tools/mask_shape_bench.py --iters %d --host-iters %d on one MI355X: per image, on the %d best instances: the moments of order up
to two, the convex hulls with their areas, and the rectangles of least area with the diameters.  host: the numpy statements of
mnc_amd/shape.py.  loop: what a user writes today over dense(i) -- numpy sums over np.nonzero for the moments,
scipy.spatial.ConvexHull over the corners of the set pixels for the hull, that hull and a numpy loop over its edges for the
rectangle -- the yardstick.  device: PackedMasks.moments / .hull / .oriented_boxes, host arrays in and out, copies included
(mnc_mask_moments / _hull / _oriented, csrc/mask_shape.hip; the hull is two calls, sizes then vertices).  kernels_us: the device
time of the launches alone between a HIP event pair (mnc_mask_shape_timing; for the hull the call with room).  All sides measured
in the same process and run.

"""


def _loop_forms(pm):
    """The loops over dense(i) -> {name: callable}, or None without scipy."""
    try:
        from scipy.spatial import ConvexHull
    except ImportError:
        return None
    idx = [i for i in range(len(pm)) if int(pm.areas[i]) > 0]

    def moments():
        out = []
        for i in idx:
            y, x = np.nonzero(pm.dense(i))
            out.append((x.size, x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()))
        return out

    def corners(i):
        y, x = np.nonzero(pm.dense(i))
        return np.unique(np.concatenate([np.stack([x + a, y + b], 1) for a in (0, 1) for b in (0, 1)]), axis=0)

    def hull():
        out = []
        for i in idx:
            pts = corners(i)
            ch = ConvexHull(pts)
            out.append((pts[ch.vertices], ch.volume))
        return out

    def oriented():
        out = []
        for i in idx:
            pts = corners(i)
            v = pts[ConvexHull(pts).vertices].astype(np.float64)
            e = np.roll(v, -1, axis=0) - v
            e /= np.linalg.norm(e, axis=1)[:, None]
            t, s = v @ e.T, v @ np.stack([-e[:, 1], e[:, 0]], 1).T
            area = (t.max(axis=0) - t.min(axis=0)) * (s.max(axis=0) - s.min(axis=0))
            out.append((int(area.argmin()), area.min()))
        return out

    return {"moments": moments, "hull": hull, "oriented": oriented}


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_shape_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import shape as SH
    timed = lambda fn: kernels_us("mnc_mask_shape_timing", fn, args.iters)          # noqa: E731 (fn: a single call of one entry)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))             # noqa: E731
    sizes = []
    for H, W, _, pm, _ in voted_instances("mask_shape_bench", args.keep, args.math):
        pm = pm.fetch()
        host = {"moments": lambda: SH.moments_numpy(pm), "hull": lambda: SH.hull_numpy(pm), "oriented": lambda: SH.oriented_numpy(pm)}
        device = {"moments": pm.moments, "hull": pm.hull, "oriented": pm.oriented_boxes}
        loops = _loop_forms(pm)
        want = {k: fn() for k, fn in host.items()}                                   # (the warm-ups)
        got = {k: fn() for k, fn in device.items()}
        room_xy, room_a = np.zeros((max(len(want["hull"].xy), 1), 2), np.int32), np.zeros(max(len(pm), 1), np.int64)
        kernels = {"moments": timed(pm.moments), "hull": timed(lambda: SH.hull_call(pm, room_xy, room_a)), "oriented": timed(pm.oriented_boxes)}
        counts = np.diff(want["hull"].vert_ptr)
        entry = {"image": "%dx%d" % (H, W), "instances": len(pm), "bits_bytes": int(pm.bits.nbytes), "pixels_set": int(pm.areas.sum()),
                 "hull_vertices": int(counts.sum()), "most_hull_vertices": int(counts.max()) if len(counts) else 0,
                 "mean_solidity": round(float(want["hull"].solidity(pm.areas).mean()), 4) if len(pm) else 0.0}
        for k in OPS:
            h, d = median_ms(host[k], args.host_iters), median_ms(device[k], args.iters)
            s = median_ms(loops[k], args.host_iters) if loops else (None, None)
            entry.update({k + "_equals_host": bool(same(want[k], got[k])), k + "_host_ms_median": h[0], k + "_host_ms_min": h[1],
                          k + "_loop_ms_median": s[0], k + "_loop_ms_min": s[1], k + "_device_ms_median": d[0],
                          k + "_device_ms_min": d[1], k + "_kernels_us_median": kernels[k],
                          k + "_device_faster_than_loop": None if s[0] is None else bool(d[0] < s[0])})
        sizes.append(entry)
    emit({"workload": "moments of order up to two, convex hulls and rectangles of least area of mnc 5-stage vgg16's voted instances at "
                      "image resolution",
          "host": "moments_numpy / hull_numpy / oriented_numpy on a host PackedMasks",
          "loop": "a loop over dense(i): numpy sums over np.nonzero, scipy.spatial.ConvexHull over the pixel corners, a numpy loop over "
                  "its edges",
          "device": "PackedMasks.moments / .hull / .oriented_boxes, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
