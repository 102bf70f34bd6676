#!/usr/bin/env python3
"""Time the surface distances between packed masks (mnc_amd/surface.py; csrc/mask_surface.hip) in four forms: the numpy statements
(surface_stats_numpy, surface_distances_numpy); the loop a user writes today -- per pair full(i, H, W) of both masks, their
surfaces by scipy.ndimage.binary_erosion, scipy.ndimage.distance_transform_edt of the other surface's complement read at the
surface pixels, then the maximum, the sum, the count within the tolerance and the roots -- the yardstick; the device calls with
their copies (PackedMasks.surface_stats and .surface_distances, host arrays in and out); and the kernels alone between HIP event
pairs (mnc_mask_surface_timing) -- on the --keep best instances of a 600x1000 and a 375x500 synthetic image (the sets of
tools/mask_boundary_bench.py), cropped to the image, against --gts synthetic ground truths: those of the instances, evenly spaced,
moved by (3, 2) and cropped to the image, so that full(i, H, W) holds every mask whole and the loop computes what the device does.  Two
pair sets: the pairs COCO's matching makes at IoU 0.5, and all pairs.  All sides are timed in this process, in this run: medians
over --iters device rounds after one warm-up; the host sides (the statements and the loop) take seconds a call and are timed
once, on --loop-pairs pairs of a pair set, evenly spaced through it, and scaled to the set.  The device results are compared with the
statements' and with the loop's; whether each device call beats the loop of the same run is reported, not asserted.  Prints one JSON line and writes it, under a heading, to --profile
(default profiles/surface_dist_bench.txt; "" writes nothing).

    python tools/surface_dist_bench.py [--iters 20] [--keep 100] [--gts 20] [--loop-pairs 40] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser, voted_instances

HEADING = """tools/surface_dist_bench.py --iters %d on one MI355X: per image, the %d best instances against %d synthetic
ground truths (those of the instances, evenly spaced, moved by (3, 2); all masks cropped to the image); pairs: the matches of COCO's matching at IoU 0.5, and all
pairs.  stats: count, greatest d2 and its place, sum of d2 and the count within surface.tolerance_sq(H, W) per pair and direction;
raw: every surface pixel's d2.  host: the numpy statements of mnc_amd/surface.py.  loop: what a user writes today -- per pair
full(i, H, W) of both masks, the surfaces by scipy.ndimage.binary_erosion, distance_transform_edt of the other surface's complement
read at the surface pixels -- the yardstick.  host and loop: one round on %d pairs of a pair set, evenly spaced through it, scaled to the set.
device: PackedMasks.surface_stats / .surface_distances (mnc_mask_surface_stats / mnc_mask_surface_dist), host arrays in and out, copies included.
kernels_us: the device time of the launches alone between HIP event pairs (mnc_mask_surface_timing).  All sides measured in the
same process and run.

"""


def loop_pair(a, b, i, j, H, W, tau2):
    """One pair as a user writes it today -> per direction (d2 of the source surface pixels in raster order, or None)."""
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(2, 1)
    surf = [m ^ ndimage.binary_erosion(m, cross) for m in (a.full(i, H, W), b.full(j, H, W))]
    out = []
    for src, dst in ((surf[0], surf[1]), (surf[1], surf[0])):
        if not dst.any():
            out.append(None)
            continue
        d = ndimage.distance_transform_edt(~dst)[src]
        out.append(np.rint(d * d).astype(np.int64))
    return out


def loop(a, b, pairs, H, W, tau2):
    """-> [(max, sum, within, hd95, assd) per pair]."""
    out = []
    for i, j in pairs.tolist():
        d = loop_pair(a, b, i, j, H, W, tau2)
        if d[0] is None or d[1] is None or not len(d[0]) or not len(d[1]):
            out.append(None)
            continue
        roots = np.sqrt(np.concatenate(d).astype(np.float64))
        out.append(([int(v.max()) for v in d], [int(v.sum()) for v in d], [int((v <= tau2).sum()) for v in d],
                    float(np.percentile(roots, 95)), float(roots.mean())))
    return out


def loop_equals(rows, st, sd):
    """The loop's figures of the picked pairs against the device's of the same pairs (masks wholly inside the image): st the
    first five fields of a SurfaceStats, sd a SurfaceDistances."""
    hd95, assd = sd.hd95(), sd.assd()
    for k, r in enumerate(rows):
        if r is None:
            continue
        if r[0] != st[1][k].tolist() or r[1] != st[3][k].tolist() or r[2] != st[4][k, :, 0].tolist():
            return False
        if abs(r[3] - hd95[k]) > 1e-9 or abs(r[4] - assd[k]) > 1e-9:
            return False
    return True


def measure(H, W, pm, args):
    from mnc_amd import surface as SF
    pm = pm.crop(0, 0, W - 1, H - 1)                                  # inside the image, where full(i, H, W) is the whole mask
    n = len(pm)
    gt = pm.take(np.linspace(0, n - 1, min(args.gts, n)).astype(int)).translate(3, 2).crop(0, 0, W - 1, H - 1)
    tau = [SF.tolerance_sq(H, W)]
    g = pm.match(gt, np.zeros(len(gt), np.uint8)).dt_match[0, 0]
    matched = np.stack([np.nonzero(g >= 0)[0], g[g >= 0]], axis=1).astype(np.int32)
    every = SF._check_pairs("surface_dist_bench", pm, gt, None)
    inside = bool((pm.bounds[:, :2] >= 0).all() and (pm.bounds[:, 2] < W).all() and (pm.bounds[:, 3] < H).all()
                  and (gt.bounds[:, :2] >= 0).all() and (gt.bounds[:, 2] < W).all() and (gt.bounds[:, 3] < H).all())
    same = lambda x, y: all(np.array_equal(p, q) for p, q in zip(x, y))               # noqa: E731
    entry = {"image": "%dx%d" % (H, W), "instances": n, "ground_truths": len(gt), "tolerance_sq": tau[0],
             "bits_bytes": int(pm.bits.nbytes), "surface_pixels": int(pm.surface().areas.sum()), "masks_inside_image": inside}
    for name, pairs in (("matched", matched), ("all", every)):
        pick = np.unique(np.linspace(0, len(pairs) - 1, min(args.loop_pairs, len(pairs))).astype(int)) if len(pairs) else np.zeros(0, int)
        few = pairs[pick]                                              # the host sides are timed on these, evenly spaced, and scaled
        scale, nf = len(pairs) / max(len(few), 1), len(few)
        t = lambda fn: median_ms(fn, 1)[0]                             # noqa: E731 (one round: seconds a call)
        keep = {}
        h_st = t(lambda: keep.update(st=SF.surface_stats_numpy(pm, gt, few, tau)))
        h_sd = t(lambda: keep.update(sd=SF.surface_distances_numpy(pm, gt, few)))
        lp = t(lambda: keep.update(rows=loop(pm, gt, few, H, W, tau[0])))
        got_st, got_sd = pm.surface_stats(gt, pairs, tau), pm.surface_distances(gt, pairs)      # (the warm-ups)
        # the picked pairs of the device's results, in the statements' form
        sub_st = [f[pick] for f in got_st[:5]]
        parts = [got_sd.slot(k, d) for k in pick for d in (0, 1)]
        sub_sd = SF.SurfaceDistances(np.concatenate([[0], np.cumsum([len(v) for v in parts])]).astype(np.int64),
                                     np.concatenate(parts) if parts else np.zeros(0, np.uint32))
        room = np.zeros(max(int(got_sd.ptr[-1]), 1), np.uint32)
        d_st = median_ms(lambda: pm.surface_stats(gt, pairs, tau), args.iters)
        d_sd = median_ms(lambda: pm.surface_distances(gt, pairs), args.iters)
        k_st = kernels_us("mnc_mask_surface_timing", lambda: pm.surface_stats(gt, pairs, tau), args.iters)
        k_sd = kernels_us("mnc_mask_surface_timing", lambda: SF.dist_call(pm, gt, pairs, room), args.iters)
        loop_ms = round(lp * scale, 3)
        entry.update({
            name + "_pairs": int(len(pairs)), name + "_raw_entries": int(got_sd.ptr[-1]), name + "_host_pairs_timed": int(nf),
            name + "_stats_equals_host": bool(same(sub_st, keep["st"][:5])),
            name + "_raw_equals_host": bool(same(sub_sd, keep["sd"])),
            name + "_loop_equals_device": bool(loop_equals(keep["rows"], sub_st, sub_sd)) if inside else None,
            name + "_mean_hausdorff": float(np.nanmean(got_st.hausdorff())) if len(pairs) else None,
            name + "_mean_boundary_f": float(got_st.boundary_f(0).mean()) if len(pairs) else None,
            name + "_stats_host_ms": round(h_st * scale, 3), name + "_raw_host_ms": round(h_sd * scale, 3), name + "_loop_ms": loop_ms,
            name + "_stats_device_ms_median": d_st[0], name + "_stats_device_ms_min": d_st[1],
            name + "_raw_device_ms_median": d_sd[0], name + "_raw_device_ms_min": d_sd[1],
            name + "_stats_kernels_us_median": k_st, name + "_raw_kernels_us_median": k_sd,
            name + "_stats_device_faster_than_loop": bool(d_st[0] < loop_ms), name + "_raw_device_faster_than_loop": bool(d_sd[0] < loop_ms),
            name + "_loop_over_stats_device": round(loop_ms / d_st[0], 1) if d_st[0] else None,
            name + "_loop_over_raw_device": round(loop_ms / d_sd[0], 1) if d_sd[0] else None})
    return entry


def main():
    ap = parser()
    ap.add_argument("--gts", type=int, default=20)
    ap.add_argument("--loop-pairs", type=int, default=40)
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "surface_dist_bench.txt"))
    args = ap.parse_args()
    sizes = [measure(H, W, pm.fetch(), args) for H, W, _, pm, _ in voted_instances("surface_dist_bench", args.keep, args.math)]
    emit({"workload": "surface distances (Hausdorff, HD95, ASSD, boundary F) between mnc 5-stage vgg16's voted instances and synthetic "
                      "ground truths at image resolution",
          "host": "surface_stats_numpy / surface_distances_numpy",
          "loop": "per pair: full(i, H, W), binary_erosion, distance_transform_edt of the other surface, read at the surface pixels",
          "device": "PackedMasks.surface_stats / .surface_distances, host arrays in and out",
          "device_rounds": max(args.iters, 1), "host_rounds": 1, "sizes": sizes},
         HEADING % (max(args.iters, 1), args.keep, args.gts, args.loop_pairs), args.profile)


if __name__ == "__main__":
    main()
