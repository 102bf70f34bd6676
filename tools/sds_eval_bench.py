#!/usr/bin/env python3
"""The SDS mAP^r evaluation at the size of SBD val, CPU loop against the device evaluator, one JSON line.

    python tools/sds_eval_bench.py [--images 5732] [--cpu-images 60] [--no-trace]

A synthetic set in tools/test_net.py's on-disk layout under a temporary directory: `--images` images of 500 x 375 with 1-5 GT
instances each (ellipses and rectangles of 20-350 px with holes, in check_voc_sds_cache's cached form) and 50-100 predictions per
image over the 20 classes (jittered GT boxes with the instance's shape as mask, and random boxes and blobs).  Timed:
  cpu     voc_eval_sds of every class at 0.5 and 0.7 on the first `--cpu-images` images, extrapolated per prediction to the set
  device  imdb.evaluate_segmentation(on_device=True) on the whole set, end to end (result pickles written and read, packing,
          upload, kernel, matching); the first call and a second one
  kernel  sds_best_overlap_kernel from a `rocprofv3 --kernel-trace --stats` run of the device evaluation in a child process
The device APs of the CPU subset are checked against the CPU's."""
import argparse
import contextlib
import glob
import io
import json
import os
import pickle
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

import _init_paths  # noqa: F401
from datasets.pascal_voc_seg import CLASSES, PascalVOCSeg
from mnc_config import cfg
from utils.voc_eval import voc_eval_sds, voc_eval_sds_device

S = 21
H, W = 375, 500


def make_set(root, n_images, seed):
    """devkit/val.txt + devkit/annotations_cache/<cls>_mask_gt.pkl; -> (all_boxes, all_masks) as the tester returns them."""
    rng = np.random.default_rng(seed)
    names = ["sbd_%05d" % i for i in range(n_images)]
    gt = [{} for _ in CLASSES]
    all_boxes = [[np.zeros((0, 5)) for _ in names] for _ in CLASSES]
    all_masks = [[np.zeros((0, 1, S, S), np.float32) for _ in names] for _ in CLASSES]
    yy, xx = np.mgrid[0:S, 0:S]
    for ii, name in enumerate(names):
        insts = []
        for _ in range(int(rng.integers(1, 6))):
            w, h = int(rng.integers(20, 351)), int(rng.integers(20, 351))
            w, h = min(w, W), min(h, H)
            x1, y1 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
            Y, X = np.mgrid[0:h, 0:w]
            m = ((X - (w - 1) / 2.0) / (w / 2.0)) ** 2 + ((Y - (h - 1) / 2.0) / (h / 2.0)) ** 2 <= 1.0 if rng.random() < 0.5 \
                else np.ones((h, w), bool)
            m &= rng.random((h, w)) > 0.05                                          # holes
            c = int(rng.integers(1, 21))
            d = {"mask": m, "mask_cls": c, "mask_bound": np.array([x1, y1, x1 + w - 1, y1 + h - 1], np.float64),
                 "already_detect": False}
            gt[c].setdefault(name, []).append(d)
            insts.append(d)
        n = int(rng.integers(50, 101))
        cls = rng.integers(1, 21, n)
        boxes = np.zeros((n, 5))
        masks = np.zeros((n, 1, S, S), np.float32)
        for k in range(n):
            if rng.random() < 0.4:
                d = insts[int(rng.integers(len(insts)))]
                cls[k] = d["mask_cls"]
                b = d["mask_bound"]
                bw, bh = b[2] - b[0] + 1, b[3] - b[1] + 1
                boxes[k, :4] = b + rng.normal(0, 0.05, 4) * np.array([bw, bh, bw, bh])
                iy, ix = (np.arange(S) * d["mask"].shape[0]) // S, (np.arange(S) * d["mask"].shape[1]) // S
                masks[k, 0] = d["mask"][iy][:, ix] ^ (rng.random((S, S)) < 0.03)
            else:
                w, h = rng.uniform(20, 350, 2)
                x1, y1 = rng.uniform(0, W - 20), rng.uniform(0, H - 20)
                boxes[k, :4] = [x1, y1, min(x1 + w, W - 1), min(y1 + h, H - 1)]
                cx, cy, r = rng.uniform(6, 14), rng.uniform(6, 14), rng.uniform(4, 12)
                masks[k, 0] = (1.0 - np.hypot(xx - cx, yy - cy) / r) >= 0.4
            boxes[k, 2] = max(boxes[k, 2], boxes[k, 0] + 1)
            boxes[k, 3] = max(boxes[k, 3], boxes[k, 1] + 1)
        boxes[:, 4] = rng.random(n)
        for c in np.unique(cls):
            sel = cls == c
            all_boxes[c][ii] = boxes[sel]
            all_masks[c][ii] = masks[sel]
    devkit = os.path.join(root, "devkit")
    cache = os.path.join(devkit, "annotations_cache")
    os.makedirs(cache)
    with open(os.path.join(devkit, "val.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    for c, name in enumerate(CLASSES):
        if c:
            with open(os.path.join(cache, name + "_mask_gt.pkl"), "wb") as f:
                pickle.dump(gt[c], f, pickle.HIGHEST_PROTOCOL)
    return names, all_boxes, all_masks


def cpu_subset(root, names, all_boxes, all_masks, n):
    """voc_eval_sds of every class at 0.5 and 0.7 on the first n images (their own result pickles).  -> (seconds, predictions,
    {thr: APs})."""
    out = os.path.join(root, "out_cpu")
    os.makedirs(out)
    lst = os.path.join(root, "devkit", "cpu.txt")
    with open(lst, "w") as f:
        f.write("".join(x + "\n" for x in names[:n]))
    preds = 0
    for c, name in enumerate(CLASSES):
        if c:
            with open(os.path.join(out, name + "_det.pkl"), "wb") as f:
                pickle.dump(all_boxes[c][:n], f, pickle.HIGHEST_PROTOCOL)
            with open(os.path.join(out, name + "_seg.pkl"), "wb") as f:
                pickle.dump([m.reshape(len(m), S, S) >= cfg.BINARIZE_THRESH for m in all_masks[c][:n]], f, pickle.HIGHEST_PROTOCOL)
            preds += sum(len(b) for b in all_boxes[c][:n])
    devkit = os.path.join(root, "devkit")
    cache = os.path.join(devkit, "annotations_cache")
    aps = {}
    t = time.perf_counter()
    with np.errstate(all="ignore"):
        for thr in (0.5, 0.7):
            aps[thr] = [voc_eval_sds(os.path.join(out, x + "_det.pkl"), os.path.join(out, x + "_seg.pkl"), devkit, lst, x, cache,
                                     CLASSES, ov_thresh=thr) for x in CLASSES[1:]]
    secs = time.perf_counter() - t
    with np.errstate(all="ignore"):
        dev = voc_eval_sds_device(os.path.join(out, "{}_det.pkl"), os.path.join(out, "{}_seg.pkl"), devkit, lst, CLASSES, cache)
    same = all(np.array_equal(np.array(dev[t_]), np.array(aps[t_]), equal_nan=True) for t_ in aps)
    return secs, preds, same


def device_only(root):
    """The device evaluation of the whole set from the result pickles a previous run left (the traced child)."""
    devkit = os.path.join(root, "devkit")
    out = os.path.join(root, "out")
    with np.errstate(all="ignore"):
        voc_eval_sds_device(os.path.join(out, "{}_det.pkl"), os.path.join(out, "{}_seg.pkl"), devkit, os.path.join(devkit, "val.txt"),
                            CLASSES, os.path.join(devkit, "annotations_cache"))


def kernel_trace(root):
    """rocprofv3 --kernel-trace --stats of device_only in a child process -> (calls, total ms) of sds_best_overlap_kernel."""
    tdir = os.path.join(root, "trace")
    cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "sds", "--",
           sys.executable, os.path.abspath(__file__), "--device-only", root]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("traced run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    for db in glob.glob(os.path.join(tdir, "**", "*.db"), recursive=True):
        con = sqlite3.connect(db)
        row = con.execute("select count(*), sum(duration) from kernels where name like '%sds_best_overlap_kernel%'").fetchone()
        if row and row[0]:
            return int(row[0]), row[1] / 1e6
    for csv in glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True):
        import csv as _csv
        for rec in _csv.DictReader(open(csv)):
            if "sds_best_overlap_kernel" in rec.get("Name", ""):
                return int(rec["Calls"]), float(rec["TotalDurationNs"]) / 1e6
    raise RuntimeError("no sds_best_overlap_kernel in the trace under " + tdir)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=5732)
    ap.add_argument("--cpu-images", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--device-only", metavar="DIR", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.device_only:
        device_only(args.device_only)
        return
    root = tempfile.mkdtemp(prefix="sds_eval_bench_")
    try:
        t = time.perf_counter()
        names, all_boxes, all_masks = make_set(root, args.images, args.seed)
        gen_s = time.perf_counter() - t
        P = sum(len(b) for cl in all_boxes for b in cl)
        G = sum(len(v) for c, x in enumerate(CLASSES[1:], 1)
                for v in pickle.load(open(os.path.join(root, "devkit", "annotations_cache", x + "_mask_gt.pkl"), "rb")).values())
        cpu_s, cpu_p, same = cpu_subset(root, names, all_boxes, all_masks, args.cpu_images)
        per_pred_thr = cpu_s / (cpu_p * 2)
        imdb = PascalVOCSeg("val", "2012", os.path.join(root, "devkit"))
        out = os.path.join(root, "out")
        os.makedirs(out)
        dev_s = []
        for _ in range(2):
            t = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                res = imdb.evaluate_segmentation(all_boxes, all_masks, out, on_device=True)
            dev_s.append(time.perf_counter() - t)
        line = {"task": "sds_eval", "images": args.images, "predictions": P, "gt_instances": G, "generate_s": round(gen_s, 1),
                "cpu_subset_images": args.cpu_images, "cpu_subset_predictions": cpu_p, "cpu_subset_s": round(cpu_s, 3),
                "cpu_us_per_pred_per_thresh": round(per_pred_thr * 1e6, 1),
                "cpu_s_est_full": round(per_pred_thr * P * 2, 1),
                "device_s_first": round(dev_s[0], 3), "device_s_second": round(dev_s[1], 3),
                "speedup_est": round(per_pred_thr * P * 2 / min(dev_s), 1), "device_aps_equal_cpu_on_subset": same,
                "mAP_05": round(float(np.mean(res[0.5])), 4), "mAP_07": round(float(np.mean(res[0.7])), 4)}
        if not args.no_trace:
            calls, ms = kernel_trace(root)
            line.update({"kernel_calls": calls, "kernel_ms": round(ms, 3)})
        print(json.dumps(line))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
