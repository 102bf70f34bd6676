#!/usr/bin/env python3
"""Time label maps in and out of packed masks (mnc_amd/labels.py; csrc/mask_labels.hip) in four forms: the numpy statements
(from_labels_numpy, to_labels_numpy); the loop a user writes today -- np.where(label == id) once per id with the box from its
minima and maxima, and out[pm.full(i, H, W)] = i + 1 over the instances -- the yardstick; the device calls with their copies
(PackedMasks.from_labels, which uploads the map twice, and .to_labels, host arrays in and out); and the kernels alone between HIP
event pairs (mnc_mask_labels_timing) -- on two kinds of input: the label map of the --keep best instances of a 600x1000 and a
375x500 synthetic image (the sets of tools/mask_boundary_bench.py, painted by to_labels_numpy), and a 375x500 superpixel map of
about 1600 labels (a jittered grid of 11 x 11 cells).  All sides are timed in this process, in this run: medians over --iters
device rounds and --host-iters host rounds after one warm-up each.  The device results are compared with the statements'; whether
each device call beats the loop of the same run is reported, not asserted, and so is what one upload of the map costs (a
synchronised host-to-device copy of its bytes, mnc_h2d), which from_labels pays a second time.  Prints one JSON line and
writes it, under a heading, to --profile (default profiles/mask_labels_bench.txt; "" writes nothing).

    python tools/mask_labels_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances

HEADING = """tools/mask_labels_bench.py --iters %d --host-iters %d on one MI355X: per input, from_labels (a label map -> PackedMasks and ids)
and to_labels (PackedMasks -> label map).  Inputs: the label map of the %d best instances of a 600x1000 and a 375x500 synthetic
image, and a 375x500 superpixel map (a jittered grid).  host: the numpy statements of mnc_amd/labels.py.  loop: what a user writes
today -- np.where(label == id) per id with the box from its minima and maxima; out[pm.full(i, H, W)] = i + 1 per instance -- the
yardstick.  device: PackedMasks.from_labels (mnc_label_table, then mnc_label_masks; each uploads the map) and .to_labels
(mnc_mask_to_labels), host arrays in and out, copies included.  kernels_us: the device time of the launches alone between a HIP
event pair (mnc_mask_labels_timing): the table's six, the masks' one, to_labels' one.  map_upload_ms: one synchronised host-to-device
copy of the map's bytes, what the second call of from_labels pays again.  All sides measured in the same process and run.

"""


def superpixels(H, W, cell, seed):
    """int32 [H, W], ids 1 .. k all present: a grid of about cell x cell superpixels whose edges wander by a few pixels."""
    rng = np.random.default_rng(seed)
    dy = np.clip(np.cumsum(rng.integers(-1, 2, W)), -3, 3) + 3
    dx = np.clip(np.cumsum(rng.integers(-1, 2, H)), -3, 3) + 3
    yy, xx = np.mgrid[0:H, 0:W]
    gy, gx = (yy + dy[None, :]) // cell, (xx + dx[:, None]) // cell
    _, inv = np.unique(gy * (gx.max() + 1) + gx, return_inverse=True)
    return (inv.reshape(H, W) + 1).astype(np.int32)


def where_loop(label):
    """The loop of utils.voc_eval.parse_inst over one map -> [(id, box, mask inside the box)]."""
    out = []
    for i in np.unique(label):
        if i == 0:
            continue
        r, c = np.where(label == i)
        x1, y1, x2, y2 = int(c.min()), int(r.min()), int(c.max()), int(r.max())
        out.append((int(i), (x1, y1, x2, y2), label[y1:y2 + 1, x1:x2 + 1] == i))
    return out


def paint_loop(pm, H, W, order):
    out = np.zeros((H, W), np.int32)
    for i in order[::-1]:
        out[pm.full(int(i), H, W)] = i + 1
    return out


def upload_ms(label, rounds):
    """-> (median, min) milliseconds of one synchronised host-to-device copy of the map (mnc_h2d into a buffer of a context of the
    library's own)."""
    import ctypes
    from mnc_amd import _lib
    ctx, dst = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.call("mnc_ctx_create", ctypes.addressof(ctx), 0)
    try:
        _lib.call("mnc_dev_alloc", ctx, label.nbytes, ctypes.addressof(dst))
        copy = lambda: _lib.call("mnc_h2d", ctx, dst, _lib.ptr(label), label.nbytes)    # noqa: E731
        copy()
        out = median_ms(copy, rounds)
        _lib.call("mnc_dev_free", ctx, dst)
    finally:
        _lib.call("mnc_ctx_destroy", ctx)
    return out


def measure(name, label, args):
    from mnc_amd import algebra, labels
    from mnc_amd.masks import PackedMasks
    H, W = label.shape
    same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f)) for f in PackedMasks.FIELDS)    # noqa: E731
    want, want_ids = labels.from_labels_numpy(label)                                 # (the warm-ups)
    got, got_ids = PackedMasks.from_labels(label)
    loop = where_loop(label)
    order = algebra.score_order(got.scores)
    want_map, got_map, loop_map = labels.to_labels_numpy(got, H, W), got.to_labels(H, W), paint_loop(got, H, W, order)
    n, ids, bounds, _, _, _, need = labels.label_table(label, None, (0,))
    entry = {"input": name, "image": "%dx%d" % (H, W), "instances": int(n), "bits_bytes": int(got.bits.nbytes),
             "map_bytes": int(label.nbytes),
             "from_labels_equals_host": bool(same(want, got) and np.array_equal(want_ids, got_ids)),
             "from_labels_loop_equals_device": bool(len(loop) == len(got) and all(
                 i == int(got_ids[k]) and box == tuple(int(v) for v in got.bounds[k]) and np.array_equal(m, got.dense(k))
                 for k, (i, box, m) in enumerate(loop))),
             "to_labels_equals_host": bool(np.array_equal(want_map, got_map) and got_map.dtype == want_map.dtype),
             "to_labels_loop_equals_device": bool(np.array_equal(loop_map, got_map))}
    forms = {"from_labels": (lambda: labels.from_labels_numpy(label), lambda: where_loop(label), lambda: PackedMasks.from_labels(label)),
             "to_labels": (lambda: labels.to_labels_numpy(got, H, W), lambda: paint_loop(got, H, W, order), lambda: got.to_labels(H, W))}
    for k, (host, loop_fn, device) in forms.items():
        h, s, d = median_ms(host, args.host_iters), median_ms(loop_fn, args.host_iters), median_ms(device, args.iters)
        entry.update({k + "_host_ms_median": h[0], k + "_host_ms_min": h[1], k + "_loop_ms_median": s[0], k + "_loop_ms_min": s[1],
                      k + "_device_ms_median": d[0], k + "_device_ms_min": d[1], k + "_device_faster_than_loop": bool(d[0] < s[0])})
    timed = lambda fn: kernels_us("mnc_mask_labels_timing", fn, args.iters)           # noqa: E731 (fn: a single launching call)
    up = upload_ms(label, args.iters)
    entry.update({"table_kernels_us_median": timed(lambda: labels.label_table(label, None, (0,))),
                  "masks_kernels_us_median": timed(lambda: labels.label_masks(label, ids, bounds, need)),
                  "to_labels_kernels_us_median": timed(lambda: got.to_labels(H, W)),
                  "table_call_ms_median": median_ms(lambda: labels.label_table(label, None, (0,)), args.iters)[0],
                  "masks_call_ms_median": median_ms(lambda: labels.label_masks(label, ids, bounds, need), args.iters)[0],
                  "map_upload_ms_median": up[0], "map_upload_ms_min": up[1],
                  "second_upload_share_of_from_labels": round(up[0] / entry["from_labels_device_ms_median"], 3)
                  if entry["from_labels_device_ms_median"] else None})
    return entry


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mask_labels_bench.txt"))
    args = ap.parse_args()
    from mnc_amd import labels
    inputs = []
    for H, W, _, pm, _ in voted_instances("mask_labels_bench", args.keep, args.math):
        inputs.append(("instances", labels.to_labels_numpy(pm.fetch(), H, W)))
    inputs.append(("superpixels", superpixels(375, 500, 11, 0)))
    emit({"workload": "label maps in and out of packed masks: from_labels and to_labels on the label maps of mnc 5-stage vgg16's voted "
                      "instances and on a superpixel map",
          "host": "from_labels_numpy / to_labels_numpy",
          "loop": "np.where(label == id) per id with the box from its minima and maxima; out[pm.full(i, H, W)] = i + 1 per instance",
          "device": "PackedMasks.from_labels / .to_labels, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1),
          "sizes": [measure(name, label, args) for name, label in inputs]},
         HEADING % (max(args.iters, 1), max(args.host_iters, 1), args.keep), args.profile)


if __name__ == "__main__":
    main()
