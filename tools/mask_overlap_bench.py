#!/usr/bin/env python3
"""Time the comparison of one image's instances with one another: the all-pairs mask IoU and the mask NMS of the voted
instances' packed masks, in host form (mnc_amd.masks.mask_overlaps_numpy / mask_nms_numpy: unpack, slice, sum per pair) against
device form (PackedMasks.overlaps() / .nms() of a device-resident InstanceView.masks() result, csrc/mask_overlaps.hip, with the
copy of the matrices resp. the kept list to the host), on a 600x1000 and a 375x500 synthetic image.  The instances are made as
tools/task_bench.py --task seg --masks makes them: the 5-stage VGG-16 graph with seeded synthetic weights, gpu_mask_voting, the
--keep best-scoring instances (synthetic weights give meaningless scores).  Medians over --iters device rounds and --host-iters
host rounds after one warm-up each; one JSON line.

    python tools/mask_overlap_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--thresh 0.5]
"""
import numpy as np

from _task_harness import emit, median_ms, parser, voted_instances


def main():
    ap = parser()
    ap.add_argument("--thresh", type=float, default=0.5)
    args = ap.parse_args()
    from mnc_amd.masks import mask_nms_numpy, mask_overlaps_numpy
    sizes = []
    for H, W, t, host, thr in voted_instances("mask_overlap_bench", args.keep, args.math):
        dev = t.net._inst.view().masks(H, W, score_thresh=thr)       # the device form's input: nothing copied yet
        n = len(dev)                                                 # (the instance table comes down here, the bits never)
        want, got = mask_overlaps_numpy(host), dev.overlaps()
        same = bool(np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))
        keep_want, keep_got = mask_nms_numpy(host, args.thresh), dev.nms(args.thresh)
        same_nms = bool(np.array_equal(keep_want, keep_got))
        assert "bits" not in dev._host
        ov_host = median_ms(lambda: mask_overlaps_numpy(host), args.host_iters, t.net.sync)
        ov_dev = median_ms(dev.overlaps, args.iters, t.net.sync)
        nms_host = median_ms(lambda: mask_nms_numpy(host, args.thresh), args.host_iters, t.net.sync)
        nms_dev = median_ms(lambda: dev.nms(args.thresh), args.iters, t.net.sync)
        sizes.append({"image": "%dx%d" % (H, W), "instances": n, "score_thresh": thr,
                      "pairs_that_meet": int((want[0] > 0).sum()), "bits_bytes": int(host.bits.nbytes),
                      "overlaps_device_equals_host": same, "overlaps_host_ms_median": ov_host[0], "overlaps_host_ms_min": ov_host[1],
                      "overlaps_device_ms_median": ov_dev[0], "overlaps_device_ms_min": ov_dev[1],
                      "nms_thresh": args.thresh, "nms_kept": int(len(keep_want)), "nms_device_equals_host": same_nms,
                      "nms_host_ms_median": nms_host[0], "nms_host_ms_min": nms_host[1],
                      "nms_device_ms_median": nms_dev[0], "nms_device_ms_min": nms_dev[1]})
    emit({"workload": "all-pairs mask IoU and mask NMS of mnc 5-stage vgg16's voted instances at image resolution",
          "host": "mask_overlaps_numpy / mask_nms_numpy on a host PackedMasks",
          "device": "PackedMasks.overlaps() / .nms() of a device-resident result + copy of inter and iou / of the kept list",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes})


if __name__ == "__main__":
    main()
