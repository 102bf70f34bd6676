#!/usr/bin/env python3
"""The "f8" math mode beside "f16" as a stream of images: ImageStream(in_flight=12) at full width over DIFFERENT 600x1000 uint8
images, both modes in one process on one GPU, one JSON line.

    python tools/f8_stream_bench.py [--images 600] [--warmup 36] [--in-flight 12] [--distinct 8] [--repeats 3]

The modes alternate (f16, f8, f16, f8, ...): each turn is a fresh stream, and the line gives every turn's rate and the median per
mode -- the spread between turns of one mode is what a difference between the modes has to be read against.
The comparison is between the two modes of this build on this box; bench.py's headline line is not involved.  Whether the fp8
weights of fc6 + fc6_mask (205 MB instead of 411) stay in the last-level cache across the images in flight shows here, if anywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_mode(weights, math, images, n, warmup, in_flight):
    from mnc_amd.native_net import ImageStream
    stream = ImageStream(weights, in_flight=in_flight, math=math)
    try:
        for i in range(warmup):                      # every net of the stream captures its graph (second image of a size) and replays it
            stream.submit(images[i % len(images)])
        stream.drain()
        t0 = time.perf_counter()
        done = sum(1 for _ in stream.map(images[i % len(images)] for i in range(n)))
        dt = time.perf_counter() - t0
    finally:
        stream.close()
    assert done == n
    return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=36)
    ap.add_argument("--in-flight", type=int, default=12)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--modes", default="f16,f8")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import mnc_amd
    from mnc_amd import models, synth
    mnc_amd.install_paths()
    weights = synth.synthetic_weights(models.write_mnc_5stage_test_prototxt(), seed=0)
    images = [np.random.default_rng(s).integers(0, 256, (600, 1000, 3), dtype=np.uint8) for s in range(args.distinct)]
    out = {"tool": "f8_stream_bench", "size": [600, 1000], "in_flight": args.in_flight, "images": args.images, "warmup": args.warmup,
           "distinct_images": args.distinct, "repeats": args.repeats}
    modes = args.modes.split(",")
    turns = {m: [] for m in modes}
    for _ in range(args.repeats):
        for math in modes:
            turns[math].append(round(run_mode(weights, math, images, args.images, args.warmup, args.in_flight), 2))
    for math in modes:
        out["turns_" + math] = turns[math]
        out["images_per_s_" + math] = round(float(np.median(turns[math])), 2)
    if "images_per_s_f16" in out and "images_per_s_f8" in out:
        out["f8_over_f16"] = round(out["images_per_s_f8"] / out["images_per_s_f16"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
