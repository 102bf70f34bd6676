#!/usr/bin/env python3
"""Time the set algebra of one image's instance masks (mnc_amd/algebra.py; csrc/mask_algebra.hip) in four forms: the numpy statements
(combine_numpy, merge_numpy, layer_numpy); the loop over full(i, H, W) a user writes today -- H x W bool arrays combined with numpy's
operators and boxed by np.nonzero -- the yardstick; the device calls with their copies (PackedMasks | / .merge(by="class") /
.layered, host arrays in and out); and the kernels alone between HIP event pairs (mnc_mask_algebra_timing) -- on the --keep best
instances of a 600x1000 and a 375x500 synthetic image (the sets of tools/mask_boundary_bench.py).  The three cases: a | b with b the
same instances rotated by one (instance i united with instance i + 1), merge(by="class") (the per-class semantic masks), and
layered() (every pixel to the best instance that covers it).  All sides are timed in this process, in this run: medians over --iters
device rounds and --host-iters host rounds after one warm-up each.  Prints one JSON line and writes it, under a heading, to --profile
(default profiles/mask_algebra_bench.txt; "" writes nothing).

    python tools/mask_algebra_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances

OPS = ("or", "merge", "layer")

HEADING = """tools/mask_algebra_bench.py --iters %d --host-iters %d on one MI355X: per image, on the %d best instances: a | b (instance i united
with instance i + 1), merge(by="class") (one semantic mask per class) and layered() (pairwise disjoint instances, the best score
first).  host: the numpy statements of mnc_amd/algebra.py.  loop: what a user writes today over full(i, H, W) -- H x W bool arrays
combined with numpy's operators, their tight boxes from np.nonzero -- the yardstick.  device: PackedMasks.__or__ / .merge / .layered,
host arrays in and out, copies included (mnc_mask_combine / _merge / _layer, csrc/mask_algebra.hip; a size call that launches
nothing, then one launching call).  kernels_us: the device time of the five launches alone between a HIP event pair
(mnc_mask_algebra_timing).  All sides measured in the same process and run.

"""


def _box(m):
    if not m.any():
        return (0, 0, -1, -1)
    ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    return (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))


def _loop_forms(pm, other, groups, H, W):
    """The loops over full(i, H, W) -> {name: callable}; each returns per result its tight box and its pixel count."""
    n = len(pm)

    def union():
        out = []
        for i in range(n):
            m = pm.full(i, H, W) | other.full(i, H, W)
            out.append((_box(m), int(m.sum())))
        return out

    def merge():
        out = []
        for g in groups:
            m = np.zeros((H, W), bool)
            for i in g:
                m |= pm.full(int(i), H, W)
            out.append((_box(m), int(m.sum())))
        return out

    def layer():
        out, covered = [None] * n, np.zeros((H, W), bool)
        for i in np.argsort(-pm.scores, kind="stable"):
            m = pm.full(int(i), H, W)
            m &= ~covered
            covered |= m
            out[int(i)] = (_box(m), int(m.sum()))
        return out

    return {"or": union, "merge": merge, "layer": layer}


def _clipped_equal(loop, got):
    """The loop's boxes and counts against the device result's: equal where the instances lie inside the image."""
    return all(tuple(int(v) for v in got.bounds[i]) == box and int(got.areas[i]) == count for i, (box, count) in enumerate(loop))


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_algebra_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import algebra as AL
    from mnc_amd.masks import PackedMasks
    timed = lambda fn: kernels_us("mnc_mask_algebra_timing", fn, args.iters)        # noqa: E731 (fn: a single launching call)
    same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f)) for f in PackedMasks.FIELDS)    # noqa: E731
    sizes = []
    for H, W, _, pm, _ in voted_instances("mask_algebra_bench", args.keep, args.math):
        pm = pm.fetch()
        n = len(pm)
        other = pm.take(np.roll(np.arange(n), -1))
        groups = AL.class_groups(pm.classes)[1]
        csr = AL.groups_csr(groups)
        host = {"or": lambda: AL.combine_numpy(pm, other, "or"), "merge": lambda: AL.merge_numpy(pm, *csr),
                "layer": lambda: AL.layer_numpy(pm)}
        device = {"or": lambda: pm | other, "merge": lambda: pm.merge(by="class"), "layer": pm.layered}
        loops = _loop_forms(pm, other, groups, H, W)
        want = {k: fn() for k, fn in host.items()}                                   # (the warm-ups)
        got = {k: fn() for k, fn in device.items()}
        inside = bool((pm.bounds[:, :2] >= 0).all() and (pm.bounds[:, 2] < W).all() and (pm.bounds[:, 3] < H).all())
        entry = {"image": "%dx%d" % (H, W), "instances": n, "classes": len(groups), "bits_bytes": int(pm.bits.nbytes),
                 "pixels_set": int(pm.areas.sum()), "pixels_covered": int(want["layer"].areas.sum()),
                 "instances_left_empty_by_layered": int((want["layer"].areas == 0).sum()), "bounds_inside_image": inside}
        for k in OPS:
            h, d, s = median_ms(host[k], args.host_iters), median_ms(device[k], args.iters), median_ms(loops[k], args.host_iters)
            entry.update({k + "_equals_host": bool(same(want[k], got[k])),
                          k + "_loop_equals_device": bool(_clipped_equal(loops[k](), got[k])) if inside else None,
                          k + "_result_bytes": int(got[k].bits.nbytes), k + "_host_ms_median": h[0], k + "_host_ms_min": h[1],
                          k + "_loop_ms_median": s[0], k + "_loop_ms_min": s[1], k + "_device_ms_median": d[0],
                          k + "_device_ms_min": d[1], k + "_kernels_us_median": timed(device[k]),
                          k + "_device_faster_than_loop": bool(d[0] < s[0])})
        sizes.append(entry)
    emit({"workload": "a | b, merge(by=\"class\") and layered() of mnc 5-stage vgg16's voted instances at image resolution",
          "host": "combine_numpy / merge_numpy / layer_numpy on a host PackedMasks",
          "loop": "a loop over full(i, H, W): numpy's operators on H x W bool arrays, tight boxes from np.nonzero",
          "device": "PackedMasks.__or__ / .merge(by=\"class\") / .layered, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
