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
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

import _init_paths  # noqa: F401
from mnc_amd import models, synth


def _median_ms(fn, rounds, sync):
    times = []
    for _ in range(max(rounds, 1)):
        sync()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(times)[len(times) // 2], 3), round(min(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--keep", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=0.5)
    ap.add_argument("--math", default=os.environ.get("MNC_MATH", "fp32"))
    args = ap.parse_args()
    os.environ["MNC_MATH"] = args.math
    from caffeWrapper.TesterWrapper import TesterWrapper
    from mnc_config import cfg
    from mnc_amd.masks import mask_nms_numpy, mask_overlaps_numpy
    from transform.mask_transform import gpu_mask_voting
    from utils.image_io import imread
    cfg.TEST.DEVICE_PREP = True
    with tempfile.TemporaryDirectory() as root:
        cfg.ROOT_DIR = root
        image_path = os.path.join(root, "im0.npy")

        class Imdb(object):
            name, image_index, _image_index, num_classes = "mask_overlap_bench", ["im0"], ["im0"], 21

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
            view = t.net._inst.view()
            host = view.masks(H, W, score_thresh=thr).fetch()            # the host form's input: a copy of everything
            host = type(host)(**host.arrays())
            dev = view.masks(H, W, score_thresh=thr)                     # the device form's: nothing copied yet
            n = len(dev)                                                 # (the instance table comes down here, the bits never)
            want, got = mask_overlaps_numpy(host), dev.overlaps()
            same = bool(np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))
            keep_want, keep_got = mask_nms_numpy(host, args.thresh), dev.nms(args.thresh)
            same_nms = bool(np.array_equal(keep_want, keep_got))
            assert "bits" not in dev._host
            ov_host = _median_ms(lambda: mask_overlaps_numpy(host), args.host_iters, t.net.sync)
            ov_dev = _median_ms(dev.overlaps, args.iters, t.net.sync)
            nms_host = _median_ms(lambda: mask_nms_numpy(host, args.thresh), args.host_iters, t.net.sync)
            nms_dev = _median_ms(lambda: dev.nms(args.thresh), args.iters, t.net.sync)
            sizes.append({"image": "%dx%d" % (H, W), "instances": n, "score_thresh": thr,
                          "pairs_that_meet": int((want[0] > 0).sum()), "bits_bytes": int(host.bits.nbytes),
                          "overlaps_device_equals_host": same, "overlaps_host_ms_median": ov_host[0], "overlaps_host_ms_min": ov_host[1],
                          "overlaps_device_ms_median": ov_dev[0], "overlaps_device_ms_min": ov_dev[1],
                          "nms_thresh": args.thresh, "nms_kept": int(len(keep_want)), "nms_device_equals_host": same_nms,
                          "nms_host_ms_median": nms_host[0], "nms_host_ms_min": nms_host[1],
                          "nms_device_ms_median": nms_dev[0], "nms_device_ms_min": nms_dev[1]})
        print(json.dumps({"workload": "all-pairs mask IoU and mask NMS of mnc 5-stage vgg16's voted instances at image resolution",
                          "host": "mask_overlaps_numpy / mask_nms_numpy on a host PackedMasks",
                          "device": "PackedMasks.overlaps() / .nms() of a device-resident result + copy of inter and iou / of the kept list",
                          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes}))
        t.net.close()


if __name__ == "__main__":
    main()
