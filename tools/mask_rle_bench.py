#!/usr/bin/env python3
"""Time the way out of one image's instances and the way back: COCO run-length encoding of the voted instances' packed masks, in
host form (mnc_amd.rle.rle_counts_numpy: unpack every mask to a full canvas, flatten it column-major, diff it) against device form
(PackedMasks.rle_counts() of a device-resident InstanceView.masks() result, csrc/mask_rle.hip, with the copies of run_ptr and of
the runs to the host), and the decoding of those counts (masks_from_counts_numpy against mnc_mask_from_rle, host arrays in, host
arrays out), on a 600x1000 and a 375x500 synthetic image.  The instances are made as tools/mask_overlap_bench.py makes them.  The
encode kernels' own time comes from the context's event profile of the same call.  Medians over --iters device rounds and
--host-iters host rounds after one warm-up each; one JSON line.

    python tools/mask_rle_bench.py [--iters 20] [--host-iters 3] [--keep 100]
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
    """Median device time of the launches `fn` makes under the name mask_rle -- the context's event pair around the encoder's five
    launches -- in microseconds."""
    times = []
    for _ in range(max(rounds, 1)):
        net.profile(1)
        fn()
        net.sync()
        recs = [r for r in net.profile_records() if r[0] == "mask_rle"]
        if recs:
            times.append(sum(r[1] for r in recs) * 1e3)
    net.profile(0)
    return round(sorted(times)[len(times) // 2], 2) if times else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--keep", type=int, default=100)
    ap.add_argument("--math", default=os.environ.get("MNC_MATH", "fp32"))
    args = ap.parse_args()
    os.environ["MNC_MATH"] = args.math
    from caffeWrapper.TesterWrapper import TesterWrapper
    from mnc_config import cfg
    from mnc_amd import rle
    from transform.mask_transform import gpu_mask_voting
    from utils.image_io import imread
    cfg.TEST.DEVICE_PREP = True
    with tempfile.TemporaryDirectory() as root:
        cfg.ROOT_DIR = root
        image_path = os.path.join(root, "im0.npy")

        class Imdb(object):
            name, image_index, _image_index, num_classes = "mask_rle_bench", ["im0"], ["im0"], 21

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
            want, got = rle.rle_counts_numpy(host, H, W), dev.rle_counts(H, W)
            same = bool(np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))
            assert "bits" not in dev._host
            back_want = rle.masks_from_counts_numpy(want[0], want[1], H, W)
            back_got = rle.masks_from_counts(want[0], want[1], H, W)
            same_back = all(np.array_equal(getattr(back_want, f), getattr(back_got, f)) for f in ("bounds", "offsets", "areas", "bits"))
            enc_host = _median_ms(lambda: rle.rle_counts_numpy(host, H, W), args.host_iters, t.net.sync)
            enc_dev = _median_ms(lambda: dev.rle_counts(H, W), args.iters, t.net.sync)
            dec_host = _median_ms(lambda: rle.masks_from_counts_numpy(want[0], want[1], H, W), args.host_iters, t.net.sync)
            dec_dev = _median_ms(lambda: rle.masks_from_counts(want[0], want[1], H, W), args.iters, t.net.sync)
            str_host = _median_ms(lambda: rle._to_rles(want[0], want[1], H, W), args.host_iters, t.net.sync)
            sizes.append({"image": "%dx%d" % (H, W), "instances": n, "score_thresh": thr, "runs": int(len(want[1])),
                          "bits_bytes": int(host.bits.nbytes), "encode_device_equals_host": same,
                          "decode_device_equals_host": bool(same_back),
                          "encode_host_ms_median": enc_host[0], "encode_host_ms_min": enc_host[1],
                          "encode_device_ms_median": enc_dev[0], "encode_device_ms_min": enc_dev[1],
                          "encode_kernels_us_median": _kernel_us(t.net, lambda: dev.rle_counts(H, W), args.iters),
                          "decode_host_ms_median": dec_host[0], "decode_host_ms_min": dec_host[1],
                          "decode_device_ms_median": dec_dev[0], "decode_device_ms_min": dec_dev[1],
                          "counts_to_strings_ms_median": str_host[0]})
        print(json.dumps({"workload": "COCO run-length encoding of mnc 5-stage vgg16's voted instances at image resolution, and back",
                          "host": "rle_counts_numpy / masks_from_counts_numpy on a host PackedMasks",
                          "device": "PackedMasks.rle_counts() of a device-resident result + copies of run_ptr and the runs; "
                                    "mnc_mask_from_rle from host counts to host arrays",
                          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes}))
        t.net.close()


if __name__ == "__main__":
    main()
