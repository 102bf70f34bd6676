#!/usr/bin/env python3
"""Score a file of COCO results by COCO's `segm` protocol (mnc_amd/coco_eval.py; the matching on the GPU, csrc/mask_match.hip, and
the accumulation of the precision / recall tables too, csrc/coco_accum.hip).

    python tools/eval_coco.py --gt GT.json --dt RESULTS.json [--polygons] [--iou-type segm|boundary] [--dilation-ratio R] [--cpu]
                              [--out FILE]

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
wording and writes them as JSON (--out, default: not written)."""
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


def evaluate(gt, results, cpu=False, polygons=False, iou_type="segm", dilation_ratio=0.02):
    """gt: the ground-truth file's dict, results: the list of results -> a summarised mnc_amd.coco_eval.CocoSegmEval."""
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
    for i, size in sizes.items():
        a, d = anns[i], dets[i]
        gm = _masks([x["segmentation"] for x in a], size, [x["category_id"] for x in a], np.zeros(len(a)), cpu, polygons)
        dm = _masks([x["segmentation"] for x in d], size, [x["category_id"] for x in d], [x["score"] for x in d], cpu, polygons)
        ev.add(i, dm, gm, [int(x.get("iscrowd", 0)) for x in a], [int(x.get("ignore", 0)) for x in a],
               [float(x["area"]) if "area" in x else float(gm.areas[k]) for k, x in enumerate(a)], image_size=size)
    ev.summarize()
    return ev


def main(argv=None):
    args = parse_args(argv)
    with open(args.gt) as f:
        gt = json.load(f)
    with open(args.dt) as f:
        results = json.load(f)
    ev = evaluate(gt, results, args.cpu, args.polygons, args.iou_type, args.dilation_ratio)
    for line in ev.lines():
        print(line)
    if args.out:
        from mnc_amd.coco_eval import STAT_NAMES
        with open(args.out, "w") as f:
            json.dump({"stats": dict(zip(STAT_NAMES, ev.stats.tolist())), "lines": ev.lines(), "images": len(gt["images"]),
                       "results": len(results), "annotations": len(gt["annotations"])}, f, indent=1)
        print("wrote %s" % args.out, file=sys.stderr)
    return ev


if __name__ == "__main__":
    main()
