#!/usr/bin/env python3
"""The MCG proposal maskdb of one VOC-sized image, numpy form against the device call, one JSON line.

    python tools/mcg_maskdb_bench.py [--proposals 2000] [--labels 40] [--numpy-proposals 100] [--calls 20] [--no-trace]

One synthetic 375 x 500 label map of ~1500 superpixels (a jittered grid) with `--proposals` unions of `--labels` superpixels each,
half of them adjacent and half scattered.  Timed:
  numpy    db/mcg_maskdb.py:mcg_maskdb_numpy (the reference's loop) on the first `--numpy-proposals` proposals, scaled to all
  device   mcg_maskdb_device end to end, host arrays to host arrays, after a warm-up call: the median of `--calls` calls
  files    scipy.io.loadmat + CSR flattening of the MCG file (read_mcg_raw) and scipy.io.savemat of the result, per image
  kernels  mcg_extent_kernel / mcg_mask_kernel from a `rocprofv3 --kernel-trace --stats` run of the device calls in a child
           process (no counters in that run)
The device result of the numpy subset is checked against the numpy form."""
import argparse
import glob
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

import _init_paths  # noqa: F401
from db.mcg_maskdb import mcg_maskdb_device, mcg_maskdb_numpy, read_mcg_raw, write_maskdb

H, W, CELL = 375, 500, 11
KERNELS = ("mcg_extent_kernel", "mcg_mask_kernel")


def make_image(n_proposals, n_labels, seed):
    """-> (superpixels uint16 [H, W], list of id lists)."""
    rng = np.random.default_rng(seed)
    dy = np.clip(np.cumsum(rng.integers(-1, 2, W)), -3, 3) + 3
    dx = np.clip(np.cumsum(rng.integers(-1, 2, H)), -3, 3) + 3
    yy, xx = np.mgrid[0:H, 0:W]
    gy, gx = (yy + dy[None, :]) // CELL, (xx + dx[:, None]) // CELL
    _, inv = np.unique(gy * (gx.max() + 1) + gx, return_inverse=True)
    sp = (inv.reshape(H, W) + 1).astype(np.uint16)
    k = int(sp.max())
    labels = []
    for i in range(n_proposals):
        if i % 2 == 0:
            side = int(np.ceil(np.sqrt(n_labels))) * CELL
            h, w = min(H, int(rng.integers(CELL, 2 * side))), min(W, int(rng.integers(CELL, 2 * side)))
            y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            ids = rng.permutation(np.unique(sp[y:y + h:2, x:x + w:2]))[:n_labels]
        else:
            ids = rng.integers(1, k + 1, n_labels)
        labels.append(np.asarray(ids, np.uint16))
    return sp, labels


def write_raw(path, sp, labels):
    import scipy.io
    cell = np.empty((len(labels), 1), object)
    for i, x in enumerate(labels):
        cell[i, 0] = x.reshape(1, -1)
    scipy.io.savemat(path, {"superpixels": sp, "labels": cell})


def device_only(path, calls):
    """The traced child: the device calls alone."""
    sp, ptr, ids = read_mcg_raw(path)
    for _ in range(calls + 1):
        mcg_maskdb_device(sp, ptr, ids)


def kernel_trace(root, path, calls):
    """rocprofv3 --kernel-trace --stats of device_only in a child process -> {kernel: (calls, mean us)}."""
    tdir = os.path.join(root, "trace")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "mcg", "--",
           sys.executable, os.path.abspath(__file__), "--device-only", path, "--calls", str(calls)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("traced run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    out = {}
    for db in glob.glob(os.path.join(tdir, "**", "*.db"), recursive=True):
        con = sqlite3.connect(db)
        for k in KERNELS:
            row = con.execute("select count(*), sum(duration) from kernels where name like '%" + k + "%'").fetchone()
            if row and row[0]:
                out[k] = (int(row[0]), row[1] / 1e3 / row[0])
        if out:
            return out
    for csv in glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True):
        import csv as _csv
        for rec in _csv.DictReader(open(csv)):
            for k in KERNELS:
                if k in rec.get("Name", ""):
                    out[k] = (int(rec["Calls"]), float(rec["TotalDurationNs"]) / 1e3 / int(rec["Calls"]))
    if not out:
        raise RuntimeError("no mcg kernels in the trace under " + tdir)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--proposals", type=int, default=2000)
    ap.add_argument("--labels", type=int, default=40)
    ap.add_argument("--numpy-proposals", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--device-only", metavar="FILE", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.device_only:
        device_only(args.device_only, args.calls)
        return
    root = tempfile.mkdtemp(prefix="mcg_maskdb_bench_")
    try:
        sp, labels = make_image(args.proposals, args.labels, args.seed)
        path = os.path.join(root, "image.mat")
        write_raw(path, sp, labels)
        t = time.perf_counter()
        sp32, ptr, ids = read_mcg_raw(path)
        load_ms = (time.perf_counter() - t) * 1e3
        k = min(args.numpy_proposals, args.proposals)
        t = time.perf_counter()
        want = mcg_maskdb_numpy(sp32, ptr, ids, top_k=k)
        numpy_ms = (time.perf_counter() - t) * 1e3
        db = mcg_maskdb_device(sp32, ptr, ids)                     # warm-up: library load, stream, first launches
        same = bool(np.array_equal(db["boxes"][:k], want["boxes"]) and np.array_equal(db["masks"][:k], want["masks"]))
        times = []
        for _ in range(max(args.calls, 20)):
            t = time.perf_counter()
            db = mcg_maskdb_device(sp32, ptr, ids)
            times.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        write_maskdb(os.path.join(root, "out.mat"), db)
        save_ms = (time.perf_counter() - t) * 1e3
        line = {"task": "mcg_maskdb", "H": H, "W": W, "superpixels": int(sp.max()), "proposals": args.proposals,
                "labels_per_proposal": args.labels, "numpy_proposals_timed": k,
                "numpy_ms_per_image": round(numpy_ms * args.proposals / k, 1), "numpy_scaled_from_subset": k < args.proposals,
                "numpy_ms_per_proposal": round(numpy_ms / k, 3),
                "device_ms_per_image": round(statistics.median(times), 3), "device_ms_min": round(min(times), 3),
                "device_calls": len(times), "loadmat_ms_per_image": round(load_ms, 1), "savemat_ms_per_image": round(save_ms, 1),
                "device_equals_numpy_on_subset": same}
        line["speedup_vs_numpy"] = round(line["numpy_ms_per_image"] / line["device_ms_per_image"], 1)
        if not args.no_trace:
            for name, (calls, us) in kernel_trace(root, path, max(args.calls, 20)).items():
                line[name + "_calls"] = calls
                line[name + "_us"] = round(us, 2)
        print(json.dumps(line))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
