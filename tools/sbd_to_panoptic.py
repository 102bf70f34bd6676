#!/usr/bin/env python3
"""Write the ground truth of an SBD image set in the COCO panoptic format, so that tools/eval_panoptic.py can score what
tools/demo.py --save-panoptic writes against this project's own dataset.

    python tools/sbd_to_panoptic.py --devkit D --image-set FILE --out DIR [--cpu]

D holds SBD's inst/<id>.mat and cls/<id>.mat (GTinst / GTcls, each with a Segmentation map); FILE lists one image id per line.
Per image the two maps become a PackedMasks by PackedMasks.from_labels(inst, cls) -- the instances are the ids of inst other than
0, ascending, each with the class its pixels have in cls (on the GPU, csrc/mask_labels.hip; with --cpu
mnc_amd.labels.from_labels_numpy and no GPU is needed or touched).  DIR/<id>.png is the inst map by the panoptic id rule
(labels.id_to_rgb: id = R + 256 G + 65536 B, 0 is void; Pillow writes the file) and DIR/panoptic.json holds `annotations`
({image_id, file_name, segments_info} with labels.segments_info's entries: id, category_id, area, bbox, iscrowd 0) and `categories`:
the twenty VOC classes, ids 1 .. 20, all of them things."""
import argparse
import json
import os

import _init_paths  # noqa: F401
from sbd_to_coco import CLASSES, read_maps


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="SBD inst / cls maps -> COCO panoptic PNGs and panoptic.json")
    p.add_argument("--devkit", required=True, help="the directory that holds inst/ and cls/")
    p.add_argument("--image-set", required=True, help="a text file, one image id per line")
    p.add_argument("--out", required=True, help="the directory to write the PNGs and panoptic.json into")
    p.add_argument("--cpu", action="store_true", help="the numpy statement instead of the GPU")
    return p.parse_args(argv)


def annotation_of(out_dir, name, inst, cls, cpu=False):
    """Write <out_dir>/<name>.png -> the annotation entry of one image's maps."""
    from PIL import Image
    from mnc_amd import labels
    from mnc_amd.masks import PackedMasks
    pm, ids = labels.from_labels_numpy(inst, cls, 0) if cpu else PackedMasks.from_labels(inst, cls, 0)
    Image.fromarray(labels.id_to_rgb(inst), "RGB").save(os.path.join(out_dir, name + ".png"))
    return {"image_id": name, "file_name": name + ".png", "segments_info": labels.segments_info(pm, ids)}


def main(argv=None):
    args = parse_args(argv)
    with open(args.image_set) as f:
        names = [line.strip() for line in f if line.strip()]
    os.makedirs(args.out, exist_ok=True)
    annotations = [annotation_of(args.out, name, *(read_maps(args.devkit, name) + (args.cpu,))) for name in names]
    path = os.path.join(args.out, "panoptic.json")
    with open(path, "w") as f:
        json.dump({"annotations": annotations, "categories": [{"id": k + 1, "name": c, "isthing": 1} for k, c in enumerate(CLASSES)]}, f)
    print("wrote %s (%d segments of %d images)" % (path, sum(len(a["segments_info"]) for a in annotations), len(annotations)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
