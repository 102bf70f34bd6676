#!/usr/bin/env python3
"""Time the backward passes of the per-RoI layers (mnc_amd/backward.py; csrc/roi_backward.hip) in this process and run: the numpy
statements on this machine's CPU, the host-array device calls with their copies and layout changes, and the kernels alone between
the HIP event pairs of the context's launch profile.  Shapes: the head's -- ROIWarping backward at C = 512 on the 38 x 63 map of a
600 x 1000 image for 300 RoIs, 14 x 14 and 28 x 28, with the FORWARD kernel's time of the same run beside it as the yardstick --
the 21 -> 14 MaskResize backward and the 14 x 14 x 512 MaskPooling backward for 300 RoIs.  Medians over --iters device rounds and
--host-iters host rounds after one warm-up each.  The results are compared; nothing about speed is asserted.
Prints one JSON line and writes it, under a heading, to --profile (default profiles/roi_backward_bench.txt; "" writes nothing).

    python tools/roi_backward_bench.py [--iters 5] [--host-iters 1] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, median_ms, parser

HEADING = """tools/roi_backward_bench.py --iters %d --host-iters %d on one MI355X.  warp_P: mnc_roi_warp_backward, C = 512, 38 x 63 map, 300
RoIs of a 600 x 1000 image, P x P grid; resize: mnc_mask_resize_backward 21 -> 14, 300 RoIs; maskpool: mnc_mask_pool_backward
14 x 14 x 512, 300 RoIs.  host: the numpy statements of mnc_amd/backward.py on this machine's CPU.  device: host arrays in and out,
copies and layout changes included.  *_us: the launches alone between the HIP event pairs of the context's profile, medians --
dfeat = ranges + gather + hwc_to_c8, drois = c8_to_hwc + the per-RoI reduction; forward_us = mnc_roi_warp (c8_to_hwc + its kernel)
on the same inputs in the same run, the yardstick.  All sides measured in the same process and run.

"""
C, H, W, R, SCALE = 512, 38, 63, 300, 0.0625


def median(values):
    return round(sorted(values)[len(values) // 2], 2) if values else None


def launches_us(fn, rounds, groups):
    """Median microseconds of the launches of fn() per group of launch names -> {group: us}."""
    from mnc_amd import backward as B
    per = {g: [] for g in groups}
    for _ in range(max(rounds, 1)):
        recs = B.kernel_times(fn)
        for g, names in groups.items():
            per[g].append(sum(ms for n, ms in recs if n in names) * 1e3)
    return {g: median(v) for g, v in per.items()}


def forward_us(feat, rois, P, rounds):
    """mnc_roi_warp on the same inputs through the same context: the launches' microseconds, median."""
    from mnc_amd import backward as B
    with B.Session() as s:
        d_feat = s.put(feat.reshape(C // 8, 8, H, W).transpose(0, 2, 3, 1))
        d_rois, d_out = s.put(rois), s.empty(R * P * P * C * 4)
        run = lambda: s.call("mnc_roi_warp", d_feat, C, H, W, d_rois, R, P, P, SCALE, 0, d_out)      # noqa: E731
        run()
        return launches_us(run, rounds, {"forward": ("c8_to_hwc", "roi_warp")})["forward"]


def main():
    ap = parser()
    ap.set_defaults(iters=5, host_iters=1)
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "roi_backward_bench.txt"))
    args = ap.parse_args()
    import mnc_amd
    mnc_amd.install_paths()
    from mnc_amd import backward as B
    rng = np.random.default_rng(11)
    feat = rng.standard_normal((C, H, W)).astype(np.float32)
    x1, y1 = rng.uniform(0, 800, R), rng.uniform(0, 450, R)
    rois = np.stack([np.zeros(R), x1, y1, np.minimum(x1 + rng.uniform(30, 500, R), 999), np.minimum(y1 + rng.uniform(30, 400, R), 599)],
                    1).astype(np.float32)
    line = {"workload": "backward of ROIWarping (C=512, 38x63, 300 RoIs, 14x14 and 28x28), MaskResize 21->14 and MaskPooling 14x14x512",
            "host": "the numpy statements of mnc_amd/backward.py", "device": "mnc_*_backward, host arrays in and out",
            "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1)}
    groups = {"dfeat": ("roi_warp_bw_ranges", "roi_warp_bw_dfeat", "hwc_to_c8"), "drois": ("c8_to_hwc", "roi_warp_bw_drois"),
              "gather": ("roi_warp_bw_dfeat",)}
    for P in (14, 28):
        dtop = rng.standard_normal((R, C, P, P)).astype(np.float32)
        name = "warp_%d" % P
        device = lambda: B.roi_warp_backward(feat, rois, P, P, SCALE, dtop)      # noqa: E731
        got = device()
        h = median_ms(lambda: B.roi_warp_backward_numpy(feat, rois, P, P, SCALE, dtop), args.host_iters)
        want = B.roi_warp_backward_numpy(feat, rois, P, P, SCALE, dtop)
        d = median_ms(device, args.iters)
        line.update({name + "_dfeat_equals_host": bool(np.array_equal(got[0], want[0])),
                     name + "_drois_max_abs_diff": float(np.abs(got[1] - want[1]).max()), name + "_drois_max_abs": float(np.abs(want[1]).max()),
                     name + "_host_ms_median": h[0], name + "_device_ms_median": d[0], name + "_device_ms_min": d[1]})
        us = launches_us(device, args.iters, groups)
        line.update({name + "_dfeat_us": us["dfeat"], name + "_gather_us": us["gather"], name + "_drois_us": us["drois"],
                     name + "_forward_us": forward_us(feat, rois, P, args.iters)})
    dout = rng.standard_normal((R, 1, 14, 14)).astype(np.float32)
    device = lambda: B.mask_resize_backward(dout, 21, 21)      # noqa: E731
    line["resize_equals_host"] = bool(np.array_equal(device(), B.mask_resize_backward_numpy(dout, 21, 21)))
    h, d = median_ms(lambda: B.mask_resize_backward_numpy(dout, 21, 21), args.host_iters), median_ms(device, args.iters)
    line.update({"resize_host_ms_median": h[0], "resize_device_ms_median": d[0],
                 "resize_us": launches_us(device, args.iters, {"k": ("mask_resize_bw",)})["k"]})
    f, m, g = (rng.standard_normal((R, C, 14, 14)).astype(np.float32), rng.uniform(0, 1, (R, 1, 14, 14)).astype(np.float32),
               rng.standard_normal((R, C, 14, 14)).astype(np.float32))
    device = lambda: B.mask_pool_backward(f, m, g)      # noqa: E731
    got, want = device(), B.mask_pool_backward_numpy(f, m, g)
    line.update({"maskpool_dfeat_equals_host": bool(np.array_equal(got[0], want[0])),
                 "maskpool_dmask_max_abs_diff": float(np.abs(got[1] - want[1]).max())})
    h, d = median_ms(lambda: B.mask_pool_backward_numpy(f, m, g), args.host_iters), median_ms(device, args.iters)
    line.update({"maskpool_host_ms_median": h[0], "maskpool_device_ms_median": d[0],
                 "maskpool_us": launches_us(device, args.iters, {"k": ("mask_pool_bw",)})["k"]})
    emit(line, HEADING % (max(args.iters, 1), max(args.host_iters, 1)), args.profile)


if __name__ == "__main__":
    main()
