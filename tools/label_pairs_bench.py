#!/usr/bin/env python3
"""Time the contingency table of two label maps (mnc_amd/pairs.py; csrc/label_pairs.hip) in four forms: the numpy statement
(label_pairs_numpy); the loops a user writes today -- np.unique on the combined key with return_counts, as panopticapi does, and
np.bincount(C * gt + pred), as every semantic evaluator does -- the yardstick; the device call with its copies (pairs.label_pairs,
host arrays in and out); and the kernels alone between HIP event pairs (mnc_label_pairs_timing) -- on four kinds of input: the class
maps of the --keep best instances of a 600x1000 and a 375x500 synthetic image against a shifted copy (21 x 21 cells at most: the LDS
plan), their instance maps against a shifted copy, and a 375x500 superpixel map of about 1600 labels (the jittered grid of
tools/mask_labels_bench.py) against the instance map of that image (the global plan).  All sides are timed in this process, in this
run: medians over --iters device rounds and --host-iters host rounds after one warm-up each.  The device results are compared with
the statement's; whether the device call beats the fastest loop of the same run is reported, not asserted.  On the tables that fit
the LDS plan the counting launch alone is timed under both plans (mnc_label_pairs_plan(1) forces the other one).  Prints one
JSON line and writes it, under a heading, to --profile (default profiles/label_pairs_bench.txt; "" writes nothing).

    python tools/label_pairs_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, median_ms, parser, voted_instances
from mask_labels_bench import superpixels

HEADING = """tools/label_pairs_bench.py --iters %d --host-iters %d on one MI355X: per input, the pair table of two label maps.  Inputs: the
class map and the instance map of the %d best instances of a 600x1000 and a 375x500 synthetic image, each against a copy shifted by
(3, 5) pixels, and a 375x500 superpixel map (a jittered grid) against the instance map of that image.  host: label_pairs_numpy.
unique / bincount: what a user writes today -- np.unique((a << 24) | b, return_counts=True); np.bincount(a * (max(b) + 1) + b) -- the
yardsticks.  device: pairs.label_pairs (mnc_label_pairs), host arrays in and out, copies included.  kernels_us: the device time of
the call's launches between HIP event pairs (mnc_label_pairs_timing 1), without the copies and the read-back between the two groups.
count_lds_us / count_global_us: the counting launch alone (timing 2) under the LDS plan and under the global plan forced by
mnc_label_pairs_plan(1), where the table fits the LDS plan.  All sides measured in the same process and run.

"""


def unique_loop(a, b):
    return np.unique((a.astype(np.int64) << 24) | b, return_counts=True)


def bincount_loop(a, b):
    nb = int(b.max()) + 1
    return np.bincount(a.reshape(-1).astype(np.int64) * nb + b.reshape(-1), minlength=(int(a.max()) + 1) * nb)


def timed_us(mode, fn, rounds):
    """Median microseconds kept by mnc_label_pairs_timing(mode) over single calls of fn()."""
    from mnc_amd import pairs
    times = []
    for _ in range(max(rounds, 1)):
        pairs.timing(mode)
        fn()
        last = pairs.timing(0)
        if last >= 0:
            times.append(last * 1e3)
    return round(sorted(times)[len(times) // 2], 2) if times else None


def measure(name, a, b, args):
    from mnc_amd import pairs
    H, W = a.shape
    want, got = pairs.label_pairs_numpy(a, b), pairs.label_pairs(a, b)                # (the warm-ups)
    key, count = unique_loop(a, b)
    flat = bincount_loop(a, b)
    cells = int(want.a_ids.size) * int(want.b_ids.size)
    entry = {"input": name, "image": "%dx%d" % (H, W), "na": int(want.a_ids.size), "nb": int(want.b_ids.size), "pairs": len(want),
             "plan": "lds" if cells <= pairs.LDS_CELLS else "global",
             "device_equals_host": bool(all(np.array_equal(getattr(want, f), getattr(got, f)) and getattr(want, f).dtype == getattr(got, f).dtype
                                            for f in pairs.LabelPairs.FIELDS)),
             "unique_equals_device": bool(np.array_equal(key, (got.a_ids[got.ia].astype(np.int64) << 24) | got.b_ids[got.ib])
                                          and np.array_equal(count, got.count)),
             "bincount_equals_device": bool(np.array_equal(flat[flat > 0], got.count) and int(flat.sum()) == H * W)}
    call = lambda: pairs.label_pairs(a, b)                                            # noqa: E731
    h = median_ms(lambda: pairs.label_pairs_numpy(a, b), args.host_iters)
    u, c = median_ms(lambda: unique_loop(a, b), args.host_iters), median_ms(lambda: bincount_loop(a, b), args.host_iters)
    d = median_ms(call, args.iters)
    entry.update({"host_ms_median": h[0], "unique_ms_median": u[0], "unique_ms_min": u[1], "bincount_ms_median": c[0],
                  "bincount_ms_min": c[1], "device_ms_median": d[0], "device_ms_min": d[1],
                  "device_faster_than_fastest_loop": bool(d[0] < min(u[0], c[0])),
                  "kernels_us_median": timed_us(1, call, args.iters)})
    if cells <= pairs.LDS_CELLS:
        entry["count_lds_us_median"] = timed_us(2, call, args.iters)
        pairs.plan(True)
        try:
            entry["count_global_us_median"] = timed_us(2, call, args.iters)
            entry["global_plan_equals_host"] = bool(np.array_equal(pairs.label_pairs(a, b).count, want.count))
            entry["device_global_plan_ms_median"] = median_ms(call, args.iters)[0]
        finally:
            pairs.plan(False)
        entry["lds_plan_faster"] = bool(entry["count_lds_us_median"] < entry["count_global_us_median"])
    else:
        entry["count_global_us_median"] = timed_us(2, call, args.iters)
    return entry


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "label_pairs_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import labels
    shift = lambda m: np.ascontiguousarray(np.roll(m, (3, 5), (0, 1)))                # noqa: E731
    inputs, inst = [], None
    for H, W, _, pm, _ in voted_instances("label_pairs_bench", args.keep, args.math):
        pm = pm.fetch()
        cls, inst = labels.to_labels_numpy(pm, H, W, values=pm.classes), labels.to_labels_numpy(pm, H, W)
        inputs.append(("classes", cls, shift(cls)))
        inputs.append(("instances", inst, shift(inst)))
    inputs.append(("superpixels", superpixels(375, 500, 11, 0), inst))
    emit({"workload": "the pair table of two label maps: class maps, instance maps and a superpixel map of mnc 5-stage vgg16's voted instances",
          "host": "label_pairs_numpy", "loops": "np.unique((a << 24) | b, return_counts=True); np.bincount(a * (max(b) + 1) + b)",
          "device": "pairs.label_pairs, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1),
          "sizes": [measure(name, a, b, args) for name, a, b in inputs]},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
