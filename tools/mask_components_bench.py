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
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

import _init_paths  # noqa: F401
from mnc_amd import models, synth

HEADING = """tools/mask_components_bench.py --iters %d --host-iters %d on one MI355X: per image, the %d best instances as a host PackedMasks;
mnc_amd.components' numpy statements and a scipy.ndimage loop over dense(i) (label + find_objects + the areas for the table, label
and a per-instance repack for the selection, binary_fill_holes and a repack for the holes) against PackedMasks.components / .select
(min_area 20, keep 1) / .fill_holes / .split (mnc_mask_components, _select, _fill_holes, _split, csrc/mask_components.hip: host
arrays in and out, one call each), on a 600x1000 and a 375x500 synthetic image; kernels_us: the device time of one call's launches
between a HIP event pair (mnc_mask_components_timing), the read-backs of the run and component totals inside it.  Host and device
sides measured in the same process and run.

"""


def _median_ms(fn, rounds):
    times = []
    for _ in range(max(rounds, 1)):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(times)[len(times) // 2], 3), round(min(times), 3)


def _kernels_us(fn, rounds):
    """Median device time of the launches of one fn() -- a single call of one entry -- in microseconds."""
    from mnc_amd import components
    times = []
    for _ in range(max(rounds, 1)):
        components.timing(True)
        fn()
        last = components.timing(False)
        if last >= 0:
            times.append(last * 1e3)
    return round(sorted(times)[len(times) // 2], 2) if times else None


def _scipy_loops(pm):
    """-> {name: fn} of the same four results through scipy.ndimage in a loop over dense(i); None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    from mnc_amd.components import _pack
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
            out.append(_pack(stay[lab]))
        return out

    def fill():
        return [_pack(ndimage.binary_fill_holes(pm.dense(i))) for i in range(len(pm)) if pm.size(i)[0]]

    def split():
        out = []
        for i in range(len(pm)):
            lab, _ = ndimage.label(pm.dense(i), structure=eight)
            out += [_pack(lab[sl] == c + 1) for c, sl in enumerate(ndimage.find_objects(lab))]
        return out

    return {"components": table, "select": select, "fill_holes": fill, "split": split}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--keep", type=int, default=100)
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_components_bench.txt"))
    ap.add_argument("--math", default=os.environ.get("MNC_MATH", "fp32"))
    args = ap.parse_args()
    os.environ["MNC_MATH"] = args.math
    from caffeWrapper.TesterWrapper import TesterWrapper
    from mnc_config import cfg
    from mnc_amd import components as CC
    from mnc_amd.masks import PackedMasks
    from transform.mask_transform import gpu_mask_voting
    from utils.image_io import imread
    cfg.TEST.DEVICE_PREP = True
    with tempfile.TemporaryDirectory() as root:
        cfg.ROOT_DIR = root
        image_path = os.path.join(root, "im0.npy")

        class Imdb(object):
            name, image_index, _image_index, num_classes = "mask_components_bench", ["im0"], ["im0"], 21

            def image_path_at(self, i):
                return image_path

        path = models.write_mnc_5stage_test_prototxt()
        t0 = time.time()
        t = TesterWrapper(path, Imdb(), synth.synthetic_weights(path, seed=0), "seg")
        print("net ready in %.1f s" % (time.time() - t0), file=sys.stderr)
        sizes = []
        for H, W in ((600, 1000), (375, 500)):
            np.save(image_path, np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8))
            im = imread(image_path)
            masks, bxs, scores = t._segmentation_forward(im)
            _, result_box = gpu_mask_voting(masks, bxs, scores, 21, 100, im.shape[1], im.shape[0])
            ranked = np.sort(np.concatenate([b[:, 4] for b in result_box]))[::-1]
            thr = float(ranked[min(args.keep, len(ranked)) - 1])
            pm = PackedMasks(**t.net._inst.view().masks(H, W, score_thresh=thr).fetch().arrays())       # host arrays alone
            t.net.sync()
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
                h, d = _median_ms(host[k], args.host_iters), _median_ms(dev[k], args.iters)
                entry.update({k + "_equals_host": bool(equal[k]), k + "_numpy_ms_median": h[0], k + "_numpy_ms_min": h[1],
                              k + "_device_ms_median": d[0], k + "_device_ms_min": d[1],
                              k + "_kernels_us_median": _kernels_us(dev[k], args.iters)})
                if loops is not None:
                    loops[k]()
                    s = _median_ms(loops[k], args.host_iters)
                    entry.update({k + "_scipy_loop_ms_median": s[0], k + "_scipy_loop_ms_min": s[1]})
            sizes.append(entry)
        line = json.dumps({"workload": "connected components (8), selection (min_area 20, keep 1), hole filling (background 4) and split of "
                                       "mnc 5-stage vgg16's voted instances at image resolution",
                           "host": "mnc_amd.components' numpy statements; scipy.ndimage in a loop over dense(i)",
                           "device": "PackedMasks.components / .select / .fill_holes / .split, one call each, host arrays in and out",
                           "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes})
        print(line)
        if args.profile:
            with open(args.profile, "w") as f:
                f.write(HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep) + line + "\n")
        t.net.close()


if __name__ == "__main__":
    main()
