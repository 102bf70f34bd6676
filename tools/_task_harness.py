"""What the bench tools of the packed-mask tasks share (mask_overlap / mask_rle / mask_match / mask_boundary / mask_components / mask_contours /
contours_simplify / mask_algebra / mask_warp / mask_labels / pixel_stats / surface_dist _bench.py; mask_poly_bench.py, coco_accum_bench.py and train_targets_bench.py take the timers and emit alone): the timers, the instances of the two
synthetic images, the output line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

import _init_paths  # noqa: F401

SIZES = ((600, 1000), (375, 500))


def parser():
    """The flags the instance tools share."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--keep", type=int, default=100)
    ap.add_argument("--math", default=os.environ.get("MNC_MATH", "fp32"))
    return ap


def _median(times, digits):
    return round(sorted(times)[len(times) // 2], digits) if times else None


def median_ms(fn, rounds, sync=None):
    """-> (median, min) wall milliseconds of fn() over `rounds` rounds; sync() (the net's, where device work may be in flight) runs
    before each round, outside the clock."""
    times = []
    for _ in range(max(rounds, 1)):
        if sync is not None:
            sync()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return _median(times, 3), round(min(times), 3)


def kernels_us(timing_entry, fn, rounds):
    """Median device time, in microseconds, of the launches of one fn() -- a single call of an entry that keeps its time for
    `timing_entry` (one of the mnc_*_timing functions) -- between that entry's HIP event pair; None when nothing was kept."""
    from mnc_amd import _lib
    times = []
    for _ in range(max(rounds, 1)):
        _lib.timing(timing_entry, True)
        fn()
        last = _lib.timing(timing_entry, False)
        if last >= 0:
            times.append(last * 1e3)
    return _median(times, 2)


def profiled_us(net, name, fn, rounds):
    """The same figure for an entry that runs on the net's context: the records `name` of the context's event profile of fn()."""
    times = []
    for _ in range(max(rounds, 1)):
        net.profile(1)
        fn()
        net.sync()
        recs = [r for r in net.profile_records() if r[0] == name]
        if recs:
            times.append(sum(r[1] for r in recs) * 1e3)
    net.profile(0)
    return _median(times, 2)


def voted_instances(tool, keep, math):
    """The instances every tool measures on: the 5-stage VGG-16 graph with seeded synthetic weights (which give meaningless scores),
    one forward and gpu_mask_voting per synthetic image of SIZES (the Imdb stub is named `tool`), the `keep` best-scoring
    instances.  Yields per image (H, W, tester, masks, thresh): the TesterWrapper, the instances' masks as a PackedMasks of host
    arrays alone, and the score threshold that selects them (t.net._inst.view().masks(H, W, score_thresh=thresh) is the same
    set, device-resident).  The net is closed when the generator ends."""
    os.environ["MNC_MATH"] = math
    from caffeWrapper.TesterWrapper import TesterWrapper
    from mnc_config import cfg
    from mnc_amd import models, synth
    from mnc_amd.masks import PackedMasks
    from transform.mask_transform import gpu_mask_voting
    from utils.image_io import imread
    cfg.TEST.DEVICE_PREP = True
    with tempfile.TemporaryDirectory() as root:
        cfg.ROOT_DIR = root
        image_path = os.path.join(root, "im0.npy")

        class Imdb(object):
            name, image_index, _image_index, num_classes = tool, ["im0"], ["im0"], 21

            def image_path_at(self, i):
                return image_path

        path = models.write_mnc_5stage_test_prototxt()
        t0 = time.time()
        t = TesterWrapper(path, Imdb(), synth.synthetic_weights(path, seed=0), "seg")
        print("net ready in %.1f s" % (time.time() - t0), file=sys.stderr)
        try:
            for H, W in SIZES:
                np.save(image_path, np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8))
                im = imread(image_path)
                masks, bxs, scores = t._segmentation_forward(im)
                _, result_box = gpu_mask_voting(masks, bxs, scores, 21, 100, im.shape[1], im.shape[0])
                ranked = np.sort(np.concatenate([b[:, 4] for b in result_box]))[::-1]
                thr = float(ranked[min(keep, len(ranked)) - 1])
                host = PackedMasks(**t.net._inst.view().masks(H, W, score_thresh=thr).fetch().arrays())
                t.net.sync()
                yield H, W, t, host, thr
        finally:
            t.net.close()


def emit(line_dict, heading="", profile_path=None):
    """Print the result as one JSON line; with a profile_path, write it there under `heading`."""
    line = json.dumps(line_dict)
    print(line)
    if profile_path:
        with open(profile_path, "w") as f:
            f.write(heading + line + "\n")
