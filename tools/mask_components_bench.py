#!/usr/bin/env python3
"""Time the connected components of one image's instance masks and what is built on them (mnc_amd/components.py;
csrc/mask_components.hip): the numpy statements (components_numpy, select_numpy, fill_holes_numpy, split_numpy: runs and a
union-find in Python per instance) and scipy.ndimage.label / binary_fill_holes in a loop over dense(i) -- the detour the layer
removes -- against the device calls (PackedMasks.components / .select / .fill_holes / .split: host arrays in and out, their copies
included) on host PackedMasks, and the device time of the launches alone between HIP event pairs (mnc_mask_components_timing; the
two read-backs of the totals lie inside the pair) -- on a 600x1000 and a 375x500 synthetic image.  The sets are those of
tools/mask_boundary_bench.py: the 5-stage VGG-16 graph with seeded synthetic weights, gpu_mask_voting, the --keep best-scoring
instances.  8-connectivity for the components, 4-connectivity of the background for the holes; the selection is min_area = 20,
keep = 1 ("the largest piece, no specks").  All sides are timed in this process, in this run: medians over --iters device rounds and
--host-iters host rounds after one warm-up each.  Prints one JSON line and writes it, under a heading, to --profile (default
profiles/mask_components_bench.txt; "" writes nothing).

    python tools/mask_components_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances


HEADING = """tools/mask_components_bench.py --iters %d --host-iters %d on one MI355X: per image, the %d best instances as a host PackedMasks;
mnc_amd.components' numpy statements and a scipy.ndimage loop over dense(i) (label + find_objects + the areas for the table, label
and a per-instance repack for the selection, binary_fill_holes and a repack for the holes) against PackedMasks.components / .select
(min_area 20, keep 1) / .fill_holes / .split (mnc_mask_components, _select, _fill_holes, _split, csrc/mask_components.hip: host
arrays in and out, one call each), on a 600x1000 and a 375x500 synthetic image; kernels_us: the device time of one call's launches
between a HIP event pair (mnc_mask_components_timing), the read-backs of the run and component totals inside it.  Host and device
sides measured in the same process and run.

"""


def _scipy_loops(pm):
    """-> {name: fn} of the same four results through scipy.ndimage in a loop over dense(i); None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    from mnc_amd.masks import pack_rows
    eight = np.ones((3, 3), bool)

    def table():
        out = []
        for i in range(len(pm)):
            lab, count = ndimage.label(pm.dense(i), structure=eight)
            out.append((np.bincount(lab.reshape(-1), minlength=count + 1)[1:], ndimage.find_objects(lab)))
        return out

    def select():
        out = []
        for i in range(len(pm)):
            lab, count = ndimage.label(pm.dense(i), structure=eight)
            area = np.bincount(lab.reshape(-1), minlength=count + 1)[1:]
            stay = np.zeros(count + 1, bool)
            if count and area.max() >= 20:
                stay[1 + int(np.argmax(area))] = True
            out.append(pack_rows(stay[lab]))
        return out

    def fill():
        return [pack_rows(ndimage.binary_fill_holes(pm.dense(i))) for i in range(len(pm)) if pm.size(i)[0]]

    def split():
        out = []
        for i in range(len(pm)):
            lab, _ = ndimage.label(pm.dense(i), structure=eight)
            out += [pack_rows(lab[sl] == c + 1) for c, sl in enumerate(ndimage.find_objects(lab))]
        return out

    return {"components": table, "select": select, "fill_holes": fill, "split": split}


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_components_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import components as CC
    from mnc_amd.masks import PackedMasks
    sizes = []
    for H, W, _, pm, _ in voted_instances("mask_components_bench", args.keep, args.math):
        same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f)) for f in PackedMasks.FIELDS)   # noqa: E731
        host = {"components": lambda: CC.components_numpy(pm, 8), "select": lambda: CC.select_numpy(pm, 8, 20, 1),
                "fill_holes": lambda: CC.fill_holes_numpy(pm, 4), "split": lambda: CC.split_numpy(pm, 8)}
        dev = {"components": lambda: pm.components(8), "select": lambda: pm.select(8, 20, 1),
               "fill_holes": lambda: pm.fill_holes(4), "split": lambda: pm.split(8)}
        want, got = {k: f() for k, f in host.items()}, {k: f() for k, f in dev.items()}             # (the warm-ups)
        equal = {"components": all(np.array_equal(a, b) for a, b in zip(want["components"], got["components"])),
                 "select": same(want["select"], got["select"]), "fill_holes": same(want["fill_holes"], got["fill_holes"]),
                 "split": same(want["split"][0], got["split"][0]) and np.array_equal(want["split"][1], got["split"][1])}
        loops = _scipy_loops(pm)
        table = want["components"]
        entry = {"image": "%dx%d" % (H, W), "instances": len(pm), "bits_bytes": int(pm.bits.nbytes), "pixels_set": int(pm.areas.sum()),
                 "components_8": int(len(table.area)), "instances_with_more_than_one": int((np.diff(table.comp_ptr) > 1).sum()),
                 "pixels_selected": int(want["select"].areas.sum()), "pixels_filled": int(want["fill_holes"].areas.sum() - pm.areas.sum())}
        for k in ("components", "select", "fill_holes", "split"):
            h, d = median_ms(host[k], args.host_iters), median_ms(dev[k], args.iters)
            entry.update({k + "_equals_host": bool(equal[k]), k + "_numpy_ms_median": h[0], k + "_numpy_ms_min": h[1],
                          k + "_device_ms_median": d[0], k + "_device_ms_min": d[1],
                          k + "_kernels_us_median": kernels_us("mnc_mask_components_timing", dev[k], args.iters)})
            if loops is not None:
                loops[k]()
                s = median_ms(loops[k], args.host_iters)
                entry.update({k + "_scipy_loop_ms_median": s[0], k + "_scipy_loop_ms_min": s[1]})
        sizes.append(entry)
    emit({"workload": "connected components (8), selection (min_area 20, keep 1), hole filling (background 4) and split of "
                      "mnc 5-stage vgg16's voted instances at image resolution",
          "host": "mnc_amd.components' numpy statements; scipy.ndimage in a loop over dense(i)",
          "device": "PackedMasks.components / .select / .fill_holes / .split, one call each, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
