#!/usr/bin/env python3
"""Score a file of COCO results by COCO's `segm` protocol (mnc_amd/coco_eval.py; the matching on the GPU, csrc/mask_match.hip, and
the accumulation of the precision / recall tables too, csrc/coco_accum.hip).

    python tools/eval_coco.py --gt GT.json --dt RESULTS.json [--polygons] [--iou-type segm|boundary] [--dilation-ratio R] [--cpu]
                              [--surface [RATIO]] [--out FILE]

RESULTS.json is what tools/demo.py --save-coco writes: a JSON array of {image_id, category_id, segmentation: {size, counts},
score}.  GT.json holds `images` ({id, height, width}), `categories` ({id}) and `annotations` ({id, image_id, category_id,
segmentation, iscrowd, area, optional ignore}).  A ground-truth segmentation must be run-length encoded -- compressed, or an
uncompressed counts list -- which is what PackedMasks.from_rle accepts; a polygon is refused with the annotation's id
(nor are the bbox and keypoints protocols done here).  With --polygons a segmentation of a ground truth or of a result may also
be a list of polygons, as in standard COCO annotation files: it is rasterised by maskApi.c's rule (mnc_mask_from_polygons on the
GPU, mnc_amd.polygons.masks_from_polygons_numpy with --cpu), and an annotation without `area` still takes it from the mask.  The masks are decoded on the GPU
(mnc_mask_from_rle), matched there (mnc_mask_match) and the matches of all images accumulated there in one call
(mnc_coco_accumulate): the tool follows the evaluator, CocoSegmEval(device=True).  With --cpu everything runs in numpy -- the
statements of all three (mnc_amd.rle.masks_from_counts_numpy, mnc_amd.coco_eval.match_numpy, mnc_amd.coco_eval.accumulate) --
and no GPU is needed or touched.  With --iou-type boundary the matching runs on min(mask IoU, boundary IoU) (Boundary IoU, the
COCO toolkit's iouType "boundary": mnc_mask_match_boundary, csrc/mask_boundary.hip; mnc_amd.coco_eval.match_boundary_numpy with
--cpu), the bands --dilation-ratio (default 0.02) of each image's diagonal wide, H and W taken from the ground-truth file's
`images`.  Prints the twelve lines in COCO's
wording and writes them as JSON (--out, default: not written).  With --surface [RATIO] (off by default; RATIO 0.008 of the
diagonal, DAVIS's) the contours are scored as well, after the twelve lines: the detections matched at IoU 0.5 to a ground truth
that is no crowd, in the area range `all` at max_det 100, give the pairs of every image; PackedMasks.surface_stats and
.surface_distances (mnc_mask_surface_stats, mnc_mask_surface_dist, csrc/mask_surface.hip; the numpy statements of mnc_amd.surface
with --cpu) measure them, and the means over all pairs of the Hausdorff distance, HD95, the average symmetric surface distance and
the boundary F-measure at surface.tolerance_sq(H, W, RATIO) are printed and written under "surface" in --out."""
import argparse
import json
import sys

import numpy as np

import _init_paths  # noqa: F401


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="COCO segm evaluation of a results file")
    p.add_argument("--gt", required=True, help="ground truth: images, categories, annotations with RLE segmentations")
    p.add_argument("--dt", required=True, help="results: what tools/demo.py --save-coco writes")
    p.add_argument("--polygons", action="store_true", help="rasterise polygon segmentations instead of refusing them")
    p.add_argument("--iou-type", default="segm", choices=("segm", "boundary"), help="the overlap to match on (default segm)")
    p.add_argument("--dilation-ratio", type=float, default=0.02, metavar="R", help="boundary: the band's width as a share of the diagonal")
    p.add_argument("--cpu", action="store_true", help="the numpy statements instead of the GPU")
    p.add_argument("--surface", nargs="?", type=float, const=0.008, default=None, metavar="RATIO",
                   help="also score the contours of the matched pairs; the F-measure's tolerance as a share of the diagonal (0.008)")
    p.add_argument("--out", default=None, metavar="FILE", help="write the twelve numbers as JSON")
    return p.parse_args(argv)


def _rle_of(seg, what, ident, size=None):
    if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
        raise SystemExit("eval_coco: %s %r has a polygon (or no) segmentation; only RLE is accepted" % (what, ident))
    if size is not None and (int(seg["size"][0]), int(seg["size"][1])) != size:
        raise SystemExit("eval_coco: %s %r is of size %s, its image of %s" % (what, ident, list(seg["size"]), list(size)))
    return seg


def _seg_of(seg, what, ident, size):
    """--polygons: a list of polygons passes (mnc_amd.polygons checks its coordinates), anything else must be an RLE."""
    if isinstance(seg, (list, tuple)):
        return seg
    return _rle_of(seg, what, ident, size)


def _masks(rles, size, classes, scores, cpu, polygons=False):
    """RLEs of one image -> PackedMasks (an image without any gets an empty set of its size); polygons: polygon lists among them."""
    from mnc_amd import rle
    if polygons:
        from mnc_amd.polygons import masks_from_segmentations
        try:
            return masks_from_segmentations(rles, size[0], size[1], np.asarray(classes, np.int32), np.asarray(scores, np.float32), cpu=cpu)
        except ValueError as e:
            raise SystemExit("eval_coco: %s" % e)
    run_ptr, runs, _, _ = rle.counts_of_rles(rles)
    make = rle.masks_from_counts_numpy if cpu else rle.masks_from_counts
    return make(run_ptr, runs, size[0], size[1], np.asarray(classes, np.int32), np.asarray(scores, np.float32))


SURFACE_NAMES = ("hausdorff", "hd95", "assd", "boundary_f")


def _surface_of(dm, gm, match, crowd, size, ratio, cpu):
    """The contour measures of one image's matched pairs -> float64 [pairs, 4] in the order of SURFACE_NAMES."""
    from mnc_amd import surface
    g = match.dt_match[0, 0]                                   # area range `all`, IoU 0.5
    d = np.nonzero(g >= 0)[0]
    d = d[np.asarray(crowd, bool)[g[d]] == 0] if len(d) else d
    pairs = np.stack([d, g[d]], axis=1).astype(np.int32).reshape(-1, 2)
    if not len(pairs):
        return np.zeros((0, 4))
    tau = [surface.tolerance_sq(size[0], size[1], ratio)]
    if cpu:
        st, sd = surface.surface_stats_numpy(dm, gm, pairs, tau), surface.surface_distances_numpy(dm, gm, pairs)
    else:
        st, sd = dm.surface_stats(gm, pairs, tau), dm.surface_distances(gm, pairs)
    return np.stack([st.hausdorff(), sd.hd95(), sd.assd(), st.boundary_f(0)], axis=1)


def evaluate(gt, results, cpu=False, polygons=False, iou_type="segm", dilation_ratio=0.02, surface_ratio=None):
    """gt: the ground-truth file's dict, results: the list of results -> a summarised mnc_amd.coco_eval.CocoSegmEval; with a
    surface_ratio its .surface is {"ratio", "pairs", and the means named in SURFACE_NAMES (None without a pair)}."""
    check = _seg_of if polygons else _rle_of
    from mnc_amd.coco_eval import CocoSegmEval
    sizes = {im["id"]: (int(im["height"]), int(im["width"])) for im in gt["images"]}
    anns, dets = {i: [] for i in sizes}, {i: [] for i in sizes}
    for a in gt["annotations"]:
        if a["image_id"] not in sizes:
            raise SystemExit("eval_coco: annotation %r names the unknown image %r" % (a.get("id"), a["image_id"]))
        check(a.get("segmentation"), "annotation", a.get("id"), sizes[a["image_id"]])
        anns[a["image_id"]].append(a)
    for k, r in enumerate(results):
        if r["image_id"] not in sizes:
            raise SystemExit("eval_coco: result %d names the unknown image %r" % (k, r["image_id"]))
        check(r.get("segmentation"), "result", k, sizes[r["image_id"]])
        dets[r["image_id"]].append(r)
    ev = CocoSegmEval(device=not cpu, classes=sorted(c["id"] for c in gt["categories"]), iou_type=iou_type,
                      dilation_ratio=dilation_ratio)
    rows = []
    for i, size in sizes.items():
        a, d = anns[i], dets[i]
        gm = _masks([x["segmentation"] for x in a], size, [x["category_id"] for x in a], np.zeros(len(a)), cpu, polygons)
        dm = _masks([x["segmentation"] for x in d], size, [x["category_id"] for x in d], [x["score"] for x in d], cpu, polygons)
        crowd = [int(x.get("iscrowd", 0)) for x in a]
        m = ev.add(i, dm, gm, crowd, [int(x.get("ignore", 0)) for x in a],
                   [float(x["area"]) if "area" in x else float(gm.areas[k]) for k, x in enumerate(a)], image_size=size)
        if surface_ratio is not None and len(a) and len(d):
            rows.append(_surface_of(dm, gm, m, crowd, size, surface_ratio, cpu))
    ev.summarize()
    ev.surface = None
    if surface_ratio is not None:
        table = np.concatenate(rows) if rows else np.zeros((0, 4))
        ev.surface = dict({"ratio": float(surface_ratio), "pairs": int(len(table))},
                          **{k: (float(table[:, c].mean()) if len(table) else None) for c, k in enumerate(SURFACE_NAMES)})
    return ev


def surface_lines(s):
    """The four lines of --surface."""
    text = (("hausdorff", " Mean Hausdorff distance            (HD)   @[ IoU=0.50 matches | pairs=%6d ] = %s"),
            ("hd95", " Mean 95th-percentile distance      (HD95) @[ IoU=0.50 matches | pairs=%6d ] = %s"),
            ("assd", " Mean symmetric surface distance    (ASSD) @[ IoU=0.50 matches | pairs=%6d ] = %s"),
            ("boundary_f", " Mean boundary F-measure            (F)    @[ tolerance=%.4f of diagonal ] = %s"))
    fmt = lambda v: "%0.3f" % v if v is not None else "-1.000"                       # noqa: E731
    return [t % (s["ratio"] if k == "boundary_f" else s["pairs"], fmt(s[k])) for k, t in text]


def main(argv=None):
    args = parse_args(argv)
    with open(args.gt) as f:
        gt = json.load(f)
    with open(args.dt) as f:
        results = json.load(f)
    ev = evaluate(gt, results, args.cpu, args.polygons, args.iou_type, args.dilation_ratio, args.surface)
    for line in ev.lines():
        print(line)
    if ev.surface is not None:
        for line in surface_lines(ev.surface):
            print(line)
    if args.out:
        from mnc_amd.coco_eval import STAT_NAMES
        out = {"stats": dict(zip(STAT_NAMES, ev.stats.tolist())), "lines": ev.lines(), "images": len(gt["images"]),
               "results": len(results), "annotations": len(gt["annotations"])}
        if ev.surface is not None:
            out["surface"] = ev.surface
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote %s" % args.out, file=sys.stderr)
    return ev


if __name__ == "__main__":
    main()
