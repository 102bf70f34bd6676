#!/usr/bin/env python3
"""Score COCO panoptic results -- what tools/demo.py --save-panoptic writes -- against panoptic ground truth (for SBD:
tools/sbd_to_panoptic.py) by panoptic quality.

    python tools/eval_panoptic.py --gt-json F --gt-dir D --dt-json F --dt-dir D [--cpu] [--out FILE]

Either side is a panoptic.json ({"annotations": [{image_id, file_name, segments_info}], "categories": [{id, isthing}]}) and the
directory of its PNGs, read with Pillow and decoded by labels.rgb_to_id (id = R + 256 G + 65536 B, 0 is void).  The categories are
the ground truth's.  Images are matched by image_id; an image of the ground truth without a result raises KeyError, as the
published evaluator does.  Per image the pairs of (gt id, predicted id) are counted on the GPU (mnc_amd.pairs.label_pairs,
csrc/label_pairs.hip; with --cpu the numpy statement, and no GPU is needed or touched) and matched by mnc_amd.panoptic's rule, that
of the published panopticapi.  Prints the PQ / SQ / RQ table for all categories, things and stuff; --out writes the summary, per
category included, as JSON."""
import argparse
import json
import os

import numpy as np

import _init_paths  # noqa: F401


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="panoptic quality of COCO panoptic PNGs against panoptic ground truth")
    p.add_argument("--gt-json", required=True)
    p.add_argument("--gt-dir", required=True)
    p.add_argument("--dt-json", required=True)
    p.add_argument("--dt-dir", required=True)
    p.add_argument("--cpu", action="store_true", help="the numpy statement instead of the GPU")
    p.add_argument("--out", default=None, metavar="FILE", help="write the summary as JSON")
    return p.parse_args(argv)


def read_panoptic(json_path, png_dir):
    """-> ({image_id: (ids int32 [H, W], segments_info)}, categories)."""
    from PIL import Image
    from mnc_amd import labels
    with open(json_path) as f:
        doc = json.load(f)
    maps = {}
    for ann in doc["annotations"]:
        rgb = np.asarray(Image.open(os.path.join(png_dir, ann["file_name"])).convert("RGB"))
        maps[ann["image_id"]] = (labels.rgb_to_id(rgb), ann["segments_info"])
    return maps, doc.get("categories", [])


def evaluate(gt_json, gt_dir, dt_json, dt_dir, cpu=False):
    """-> the PanopticEval with every image of the ground truth added."""
    from mnc_amd.panoptic import PanopticEval
    gt, categories = read_panoptic(gt_json, gt_dir)
    dt, _ = read_panoptic(dt_json, dt_dir)
    ev = PanopticEval(categories, device=not cpu)
    for image_id, (gt_map, gt_segments) in gt.items():
        if image_id not in dt:
            raise KeyError("eval_panoptic: no result for image %r" % (image_id,))
        ev.add(image_id, gt_map, gt_segments, *dt[image_id])
    return ev


def main(argv=None):
    args = parse_args(argv)
    ev = evaluate(args.gt_json, args.gt_dir, args.dt_json, args.dt_dir, args.cpu)
    out = ev.summarize()
    print("\n".join(ev.lines()))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({k: ({str(c): s for c, s in v.items()} if k == "per_class" else v) for k, v in out.items()}, f)
        print("wrote %s" % args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
