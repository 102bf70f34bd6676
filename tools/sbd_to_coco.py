#!/usr/bin/env python3
"""Write the ground truth of an SBD image set as a COCO ground-truth file, so that tools/eval_coco.py can score the results of
tools/demo.py --save-coco against SBD by COCO's `segm` protocol and by Boundary IoU.

    python tools/sbd_to_coco.py --devkit D --image-set FILE --out gt.json [--cpu]

D holds SBD's inst/<id>.mat and cls/<id>.mat (GTinst / GTcls, each with a Segmentation map); FILE lists one image id per line.
Per image the two maps become a PackedMasks by PackedMasks.from_labels(inst, cls) -- the instances are the ids of inst other than
0, ascending, as utils.voc_eval.parse_inst takes them, each with the class its pixels have in cls (on the GPU,
csrc/mask_labels.hip; with --cpu mnc_amd.labels.from_labels_numpy and no GPU is needed or touched) -- and are run-length encoded
in the image by .rle(H, W) (csrc/mask_rle.hip; with --cpu mnc_amd.rle's numpy statement).  gt.json holds `images` ({id, file_name,
height, width}), `categories` (the twenty VOC classes, ids 1 .. 20) and `annotations` ({id, image_id, category_id, segmentation:
{size, counts}, area, bbox: [x, y, w, h], iscrowd: 0}); tools/eval_coco.py --gt reads it as it is."""
import argparse
import json
import os

import numpy as np

import _init_paths  # noqa: F401

CLASSES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog", "horse",
           "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="SBD inst / cls maps -> a COCO ground-truth file with RLE segmentations")
    p.add_argument("--devkit", required=True, help="the directory that holds inst/ and cls/")
    p.add_argument("--image-set", required=True, help="a text file, one image id per line")
    p.add_argument("--out", required=True, help="the COCO ground-truth file to write")
    p.add_argument("--cpu", action="store_true", help="the numpy statements instead of the GPU")
    return p.parse_args(argv)


def read_maps(devkit, name):
    """-> (inst, cls): the two Segmentation maps of one image, as utils.voc_eval.parse_inst reads them."""
    import scipy.io as sio
    inst = sio.loadmat(os.path.join(devkit, "inst", name + ".mat"))["GTinst"]["Segmentation"][0][0]
    cls = sio.loadmat(os.path.join(devkit, "cls", name + ".mat"))["GTcls"]["Segmentation"][0][0]
    return inst, cls


def annotations_of(name, inst, cls, first_id=1, cpu=False):
    """-> the COCO annotation entries of one image's maps."""
    from mnc_amd import labels, rle
    from mnc_amd.masks import PackedMasks
    H, W = inst.shape
    if cpu:
        pm, _ = labels.from_labels_numpy(inst, cls, 0)
        rles = rle._to_rles(*(rle.rle_counts_numpy(pm, H, W) + (H, W)))
    else:
        pm, _ = PackedMasks.from_labels(inst, cls, 0)
        rles = pm.rle(H, W)
    out = []
    for k, seg in enumerate(labels.segments_info(pm, np.arange(len(pm)))):
        out.append({"id": first_id + k, "image_id": name, "category_id": seg["category_id"], "segmentation": rles[k],
                    "area": seg["area"], "bbox": seg["bbox"], "iscrowd": 0})
    return out


def convert(devkit, names, cpu=False):
    """-> the ground-truth file's dict for these image ids."""
    images, annotations = [], []
    for name in names:
        inst, cls = read_maps(devkit, name)
        images.append({"id": name, "file_name": name + ".jpg", "height": int(inst.shape[0]), "width": int(inst.shape[1])})
        annotations.extend(annotations_of(name, inst, cls, len(annotations) + 1, cpu))
    return {"images": images, "categories": [{"id": k + 1, "name": c} for k, c in enumerate(CLASSES)], "annotations": annotations}


def main(argv=None):
    args = parse_args(argv)
    with open(args.image_set) as f:
        names = [line.strip() for line in f if line.strip()]
    gt = convert(args.devkit, names, args.cpu)
    with open(args.out, "w") as f:
        json.dump(gt, f)
    print("wrote %s (%d annotations of %d images)" % (args.out, len(gt["annotations"]), len(gt["images"])))
    return gt


if __name__ == "__main__":
    main()
