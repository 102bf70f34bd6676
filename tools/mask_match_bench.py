#!/usr/bin/env python3
"""Time COCO's matching of one image's detections to its ground truths (mnc_amd/coco_eval.py, csrc/mask_match.hip): the numpy
statement (match_numpy: unpack, slice and sum per pair, then evaluateImg's triple loop) on a host PackedMasks against
PackedMasks.match() of a device-resident InstanceView.masks() result, with its copies of the five tables to the host, and the
device time of the launches alone -- on a 600x1000 and a 375x500 synthetic image.  The detections are made as
tools/mask_overlap_bench.py makes them: the 5-stage VGG-16 graph with seeded synthetic weights, gpu_mask_voting, the --keep
best-scoring instances (synthetic weights give meaningless scores).  The ground truths are synthetic too: --gts of those
instances, evenly spaced, every tenth of them a crowd; default thresholds and area ranges (T = 10, A = 4), max_det = 100.
Medians over --iters device rounds and --host-iters host rounds after one warm-up each; one JSON line.

    python tools/mask_match_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--gts 20]
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


def _kernel_us(net, fn, rounds):
    """Median device time of the launches `fn` makes under the name mask_match -- the context's event pair around the uploads,
    the fills and the four kernels -- in microseconds."""
    times = []
    for _ in range(max(rounds, 1)):
        net.profile(1)
        fn()
        net.sync()
        recs = [r for r in net.profile_records() if r[0] == "mask_match"]
        if recs:
            times.append(sum(r[1] for r in recs) * 1e3)
    net.profile(0)
    return round(sorted(times)[len(times) // 2], 2) if times else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--keep", type=int, default=100)
    ap.add_argument("--gts", type=int, default=20)
    ap.add_argument("--math", default=os.environ.get("MNC_MATH", "fp32"))
    args = ap.parse_args()
    os.environ["MNC_MATH"] = args.math
    from caffeWrapper.TesterWrapper import TesterWrapper
    from mnc_config import cfg
    from mnc_amd.coco_eval import Match, match_numpy
    from transform.mask_transform import gpu_mask_voting
    from utils.image_io import imread
    cfg.TEST.DEVICE_PREP = True
    with tempfile.TemporaryDirectory() as root:
        cfg.ROOT_DIR = root
        image_path = os.path.join(root, "im0.npy")

        class Imdb(object):
            name, image_index, _image_index, num_classes = "mask_match_bench", ["im0"], ["im0"], 21

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
            gt = host.take(np.linspace(0, n - 1, min(args.gts, n)).astype(int))
            crowd = (np.arange(len(gt)) % 10 == 9).astype(np.uint8)
            want, got = match_numpy(host, gt, crowd), dev.match(gt, crowd)
            same = all(np.array_equal(a, b) for a, b in zip(want[:5], got[:5]))
            assert "bits" not in dev._host
            m_host = _median_ms(lambda: match_numpy(host, gt, crowd), args.host_iters, t.net.sync)
            m_dev = _median_ms(lambda: dev.match(gt, crowd), args.iters, t.net.sync)
            sizes.append({"image": "%dx%d" % (H, W), "detections": n, "ground_truths": len(gt), "classes": int(len(np.unique(host.classes))),
                          "score_thresh": thr, "matches_at_iou50": int((want.dt_match[0, 0] >= 0).sum()),
                          "bits_bytes": int(host.bits.nbytes), "device_equals_host": bool(same),
                          "host_ms_median": m_host[0], "host_ms_min": m_host[1],
                          "device_ms_median": m_dev[0], "device_ms_min": m_dev[1],
                          "kernels_us_median": _kernel_us(t.net, lambda: dev.match(gt, crowd), args.iters)})
        print(json.dumps({"workload": "COCO matching (T = 10, A = 4, max_det = 100) of mnc 5-stage vgg16's voted instances against "
                                      "synthetic ground truths at image resolution",
                          "host": "match_numpy on a host PackedMasks", "tables": list(Match._fields[:5]),
                          "device": "PackedMasks.match() of a device-resident result + copies of the five tables",
                          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes}))
        t.net.close()


if __name__ == "__main__":
    main()
