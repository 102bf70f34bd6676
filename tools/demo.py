#!/usr/bin/env python3
"""MNC demo on MI355X -- same flags and flow as the reference's tools/demo.py:
build the net, warm up twice on a grey image, then per image: im_detect (timed "forward time"), gpu_mask_voting,
optional visualisation.

    python tools/demo.py [--gpu 0] [--def test.prototxt] [--net weights.npz] [--images a.jpg b.jpg ...] [--no-vis] [--device-vis]
                         [--save-masks DIR] [--save-coco FILE] [--save-annotations FILE [--polygon-epsilon E] [--oriented-boxes] [--pixel-stats]]
                         [--min-component-area A [--largest-component]] [--smooth-radius R] [--exclusive]
                         [--flip-tta [--tta-nms T]] [--save-panoptic DIR]

Differences that are deliberate: weights come from an .npz (h5py is optional); without --net seeded synthetic weights
are used (the trained model cannot be fetched here), and --def defaults to the graph emitted by mnc_amd.models.
`--cpu` is accepted and ignored by the network, exactly as in the reference (demo.py:40-42 vs :126); with --save-masks it selects
the numpy form of the per-instance masks (transform.mask_transform.instance_masks_numpy) instead of the GPU's, with --save-coco
the numpy form of the run-length encoding as well (mnc_amd.rle.rle_counts_numpy).  --min-component-area A drops the 8-connected
components of fewer than A pixels from every mask that --save-masks / --save-coco write, --largest-component keeps the largest of
what is left (PackedMasks.select, csrc/mask_components.hip; with --cpu mnc_amd.components.select_numpy); without the two flags the
output is what it was.  --save-annotations FILE writes the same instances as a COCO annotation-format file (images, categories,
annotations) whose segmentations are polygons: the outer loops of the masks' outlines (PackedMasks.contours, csrc/mask_contours.hip;
with --cpu mnc_amd.contours.contours_numpy).  Polygons belong in annotation files; COCO results files carry RLE, which is what
--save-coco writes.  tools/eval_coco.py --gt FILE --polygons reads the file.  --polygon-epsilon E simplifies those polygons to E
pixels (Contours.simplify, csrc/contour_simplify.hip; with --cpu mnc_amd.contours.simplify_numpy); 0, the default, writes the exact
pixel staircase.  --smooth-radius R opens, then closes every written mask by the disc of radius R (PackedMasks.open / .close,
csrc/mask_distance.hip; with --cpu mnc_amd.distance.morph_numpy): spurs, necks and notches narrower than the disc and the resize
staircase go.  It runs before the component selection -- an opening can cut a neck, and the selection then drops the speck; 0, the
default, leaves the masks as they are.  --oriented-boxes adds to every annotation of --save-annotations "rbox": [cx, cy, w, h, angle]
-- the rectangle of least area around the written mask, the angle in degrees from +x towards +y (OrientedBoxes.rbox of
PackedMasks.oriented_boxes, csrc/mask_shape.hip; with --cpu mnc_amd.shape.oriented_numpy; null for a mask without a pixel) -- and
"solidity", its pixel count over the area of its convex hull; without the flag the file is what it was.  --exclusive makes the
written instances of an image pairwise disjoint: every pixel stays with the best-scoring instance that covers it
(PackedMasks.layered, csrc/mask_algebra.hip; with --cpu mnc_amd.algebra.layer_numpy), which is what the COCO panoptic format and an
object PNG want.  It runs after --smooth-radius and before the component selection, and leaves every instance tight bounds.
--flip-tta is test-time augmentation by the mirror image: every image is also run mirrored (im[:, ::-1]), the mirrored run's packed
masks are flipped back into the image's frame (PackedMasks.fliplr, csrc/mask_warp.hip; with --cpu mnc_amd.warp.isometry_numpy), the
two sets are concatenated and reduced by the class-aware mask NMS at IoU --tta-nms (default 0.5), before everything above.  Off by
default; without the flag the output is what it was.  --save-panoptic DIR writes, for every image, the label map of the masks the
other writers would write -- after --smooth-radius, --exclusive and the component selection -- as DIR/<name>.png in the COCO
panoptic encoding (PackedMasks.to_labels, csrc/mask_labels.hip; with --cpu mnc_amd.labels.to_labels_numpy; id = index + 1 through
mnc_amd.labels.id_to_rgb, Pillow writes the file), and one DIR/panoptic.json with every image's segments_info; without the flag
every output is what it was.  --pixel-stats adds to every annotation of --save-annotations "mean_color": [R, G, B] and "std_color",
the mean and the standard deviation of the image's colours under the written mask (PixelStats.mean / .std of
PackedMasks.pixel_stats, csrc/mask_pixels.hip; with --cpu mnc_amd.pixels.pixel_stats_numpy; both null for a mask without a pixel);
without the flag the file is byte for byte what it was."""
import argparse
import os
import time

import numpy as np

import _init_paths  # noqa: F401
import caffe
from mnc_config import cfg
from transform.bbox_transform import clip_boxes
from transform.mask_transform import gpu_mask_voting
from utils.blob import can_prep_on_device, im_list_to_blob, prep_im_for_blob, prep_im_for_blob_device

CLASSES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
           "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="MNC demo (MI355X)")
    p.add_argument("--gpu", dest="gpu_id", default=0, type=int, help="GPU device id to use [0]")
    p.add_argument("--cpu", dest="cpu_mode", action="store_true", help="accepted for compatibility; ignored")
    p.add_argument("--def", dest="prototxt", default=None, type=str, help="prototxt defining the network")
    p.add_argument("--net", dest="caffemodel", default=None, type=str, help="weights (.npz; .h5 needs h5py)")
    p.add_argument("--images", nargs="*", default=None, help="image files (default: data/demo/*.jpg if present)")
    p.add_argument("--no-vis", dest="vis", action="store_false", help="skip writing visualisations")
    p.add_argument("--out-dir", dest="out_dir", default=None, help="where the *_mnc.png visualisations go [next to each image]")
    p.add_argument("--vis-thresh", dest="vis_thresh", default=0.5, type=float,
                   help="score threshold of the drawn instances [0.5, the reference's constant, demo.py:103]")
    p.add_argument("--device-vis", dest="device_vis", action="store_true",
                   help="render the class image and its blend over the photo on the GPU (cfg.TEST.USE_GPU_VIS)")
    p.add_argument("--save-masks", dest="save_masks", default=None, metavar="DIR",
                   help="write <image>_masks.npz per image: one binary mask per instance scoring >= --vis-thresh at image "
                        "resolution, packed one bit per pixel (the arrays of mnc_amd.masks.PackedMasks)")
    p.add_argument("--save-coco", dest="save_coco", default=None, metavar="FILE",
                   help="write the instances scoring >= --vis-thresh of all images as one JSON array of COCO results: "
                        "{image_id, category_id, segmentation: {size, counts}, bbox, score}, the masks run-length encoded")
    p.add_argument("--save-annotations", dest="save_annotations", default=None, metavar="FILE",
                   help="write the instances scoring >= --vis-thresh of all images as one COCO annotation-format file: images, "
                        "categories and annotations {id, image_id, category_id, segmentation: [polygons], bbox, area, iscrowd: 0, "
                        "score}, the polygons being the outer outlines of the masks (holes are filled: COCO ORs the polygons)")
    p.add_argument("--polygon-epsilon", dest="polygon_epsilon", default=0.0, type=float, metavar="E",
                   help="simplify the polygons --save-annotations writes to E pixels (Douglas-Peucker on the closed loops) [0: the "
                        "exact outline]")
    p.add_argument("--oriented-boxes", dest="oriented_boxes", action="store_true",
                   help="add \"rbox\": [cx, cy, w, h, angle in degrees] (the rectangle of least area) and \"solidity\" (pixels over "
                        "convex hull area) to every annotation --save-annotations writes, after the smoothing and the selection")
    p.add_argument("--pixel-stats", dest="pixel_stats", action="store_true",
                   help="add \"mean_color\": [R, G, B] and \"std_color\" (the image's colours under the written mask) to every "
                        "annotation --save-annotations writes")
    p.add_argument("--min-component-area", dest="min_component_area", default=0, type=int, metavar="A",
                   help="drop the 8-connected components of fewer than A pixels from the masks --save-masks / --save-coco / "
                        "--save-annotations write")
    p.add_argument("--largest-component", dest="largest_component", action="store_true",
                   help="keep only the largest 8-connected component of every written mask")
    p.add_argument("--smooth-radius", dest="smooth_radius", default=0.0, type=float, metavar="R",
                   help="open, then close the masks --save-masks / --save-coco / --save-annotations write by the disc of radius R, "
                        "before the component selection [0: off]")
    p.add_argument("--exclusive", dest="exclusive", action="store_true",
                   help="make the masks --save-masks / --save-coco / --save-annotations write pairwise disjoint: each pixel goes to "
                        "the best-scoring instance that covers it; after --smooth-radius, before the component selection")
    p.add_argument("--save-panoptic", dest="save_panoptic", default=None, metavar="DIR",
                   help="write every image's instances as one COCO panoptic PNG (the label map of the written masks, id = R + 256 G "
                        "+ 65536 B) into DIR, and DIR/panoptic.json with their segments_info")
    p.add_argument("--flip-tta", dest="flip_tta", action="store_true",
                   help="also run every image mirrored, flip its masks back and merge the two sets by class-aware mask NMS, before "
                        "--smooth-radius, --exclusive and the component selection")
    p.add_argument("--tta-nms", dest="tta_nms", default=0.5, type=float, metavar="T",
                   help="mask IoU above which --flip-tta drops the lower-scoring of two instances of a class [0.5]")
    return p.parse_args(argv)


def prepare_mnc_args(im, net):
    """image (H,W,3 BGR) -> ({'data','im_info'} float32 blobs, [scale]); reshapes the two input blobs.  A uint8 image is
    mean-subtracted and resized on the GPU (cfg.TEST.DEVICE_PREP, default): `data` is then a DeviceArray holding the same
    values, which net.forward adopts without a host round trip."""
    if can_prep_on_device(net, im):
        data, im_scale = prep_im_for_blob_device(net, im, cfg.PIXEL_MEANS, cfg.TEST.SCALES[0], cfg.TRAIN.MAX_SIZE)
    else:
        im_scaled, im_scale = prep_im_for_blob(im, cfg.PIXEL_MEANS, cfg.TEST.SCALES[0], cfg.TRAIN.MAX_SIZE)
        data = im_list_to_blob([im_scaled]).astype(np.float32, copy=False)
    im_scales = [np.array(im_scale)]
    im_info = np.array([[data.shape[2], data.shape[3], im_scales[0]]], dtype=np.float32)
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(*im_info.shape)
    return {"data": data, "im_info": im_info}, im_scales


def im_detect(im, net):
    """-> boxes [2R,4] (original-image pixels), masks [2R,1,21,21], seg scores [2R,21] of stages 3 and 5.
    With cfg.TEST.DEVICE_RESULTS (default) the three results stay on the GPU as DeviceArrays -- gpu_mask_voting consumes them
    there, np.asarray() / indexing gives the reference's numpy arrays."""
    forward_kwargs, im_scales = prepare_mnc_args(im, net)
    net.forward(**forward_kwargs)
    scale = np.float32(im_scales[0])      # float32 un-scaling: what numpy-1.x value-based casting did in the reference
    if cfg.TEST.get("DEVICE_RESULTS", True) and hasattr(net, "detect_tail"):
        return net.detect_tail(scale, im.shape)
    stage_boxes = []
    for name in ("rois", "rois_ext"):
        rois = net.blobs[name].data.copy()
        stage_boxes.append(clip_boxes(rois[:, 1:5] / scale, im.shape)[0])
    masks = np.concatenate((net.blobs["mask_proposal"].data, net.blobs["mask_proposal_ext"].data), axis=0)
    scores = np.concatenate((net.blobs["seg_cls_prob"].data, net.blobs["seg_cls_prob_ext"].data), axis=0)
    return np.concatenate(stage_boxes, axis=0), masks, scores


def get_vis_dict(result_box, result_mask, img_name, cls_names, vis_thresh=0.5):
    boxes, masks, classes = [], [], []
    for cls_ind in range(len(cls_names)):
        det, seg = result_box[cls_ind], result_mask[cls_ind]
        for k in np.where(det[:, -1] >= vis_thresh)[0]:
            boxes.append(det[k])
            masks.append(seg[k][0])
            classes.append(cls_ind + 1)
    return {"image_name": img_name, "cls_name": classes, "boxes": boxes, "masks": masks}


def _read_image_bgr(path):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])


def _class_overlay(im_bgr, pred, view=None, vis_thresh=0.5):
    """-> PIL RGB image: the class-id image of the instances in VOC colours blended 0.8 over the photo.  With
    cfg.TEST.USE_GPU_VIS it comes from the GPU in one launch (csrc/render.hip) -- from the device records of `view` (the
    InstanceView of the voting; no lists() / get_vis_dict on this path) or else from `pred` -- with the same pixels."""
    from PIL import Image
    h, w = im_bgr.shape[:2]
    if cfg.TEST.USE_GPU_VIS:
        if view is not None:
            # the record's class id is get_vis_dict's cls_ind + 1 (over the foreground list) and vis_seg._prepare_dict's cls_ind
            # (over all classes): the same number
            res = view.render(h, w, vis_thresh=vis_thresh, image=np.ascontiguousarray(im_bgr), alpha=0.8)
        else:
            from mnc_amd.render import render_pred_dict
            res = render_pred_dict(w, h, pred, image=np.ascontiguousarray(im_bgr), alpha=0.8)
        return Image.fromarray(res.overlay)
    from utils.vis_seg import _convert_pred_to_image, _get_voc_color_map
    _, cls_img = _convert_pred_to_image(w, h, pred)
    cls_rgb = _get_voc_color_map().astype(np.uint8)[cls_img]
    background = Image.fromarray(np.ascontiguousarray(im_bgr[:, :, ::-1])).convert("RGBA")
    return Image.blend(background, Image.fromarray(cls_rgb).convert("RGBA"), 0.8).convert("RGB")


def _visualise(im_bgr, pred, out_path, view=None, vis_thresh=0.5):
    """The tail of the reference demo (tools/demo.py:150-191): class-id image of the voted instances
    (lib/utils/vis_seg.py:_convert_pred_to_image) in VOC colours, blended 0.8 over the photo, one "<class> <score>" label per
    instance at its box corner, saved as PNG (matplotlib; PIL-only without the labels when matplotlib is missing)."""
    blended = _class_overlay(im_bgr, pred, view, vis_thresh)
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        blended.save(out_path)
        return
    fig, ax = plt.subplots(figsize=(12, 12))
    ax.imshow(np.asarray(blended), aspect="equal")
    for box, cls_ind in zip(pred["boxes"], pred["cls_name"]):
        ax.text(box[0], box[1] - 8, "{:s} {:.4f}".format(CLASSES[cls_ind - 1], box[-1]), bbox=dict(facecolor="blue", alpha=0.5),
                fontsize=14, color="white")
    plt.axis("off")
    plt.tight_layout()
    fig.savefig(out_path)
    plt.close(fig)


def _packed_masks(im_shape, result_mask, result_box, view=None, score_thresh=0.5, cpu=False):
    """The instances scoring >= score_thresh as per-instance binary masks at image resolution (mnc_amd.masks.PackedMasks): from
    the device records of `view` (InstanceView.masks, csrc/inst_masks.hip) or else from the lists, on the GPU; cpu=True: the numpy
    loop, with the same arrays."""
    from mnc_amd.masks import from_lists
    from transform.mask_transform import instance_masks, instance_masks_numpy
    h, w = im_shape[:2]
    if view is not None and not cpu:
        return view.masks(h, w, score_thresh=score_thresh)
    bxs, mks, classes = from_lists(result_mask, result_box, score_thresh)
    return (instance_masks_numpy if cpu else instance_masks)(bxs, mks, h, w, clip=True, classes=classes)


def _select_components(packed, min_area, largest, cpu=False):
    """The written masks without their components of fewer than min_area pixels and, with `largest`, without all but the largest
    (on the GPU, csrc/mask_components.hip; cpu=True: the numpy statement).  A device-resident result is fetched first."""
    from mnc_amd import components
    args = (8, max(int(min_area), 1), 1 if largest else 0)
    return components.select_numpy(packed.fetch(), *args) if cpu else packed.select(*args)


def _smooth(packed, radius, cpu=False):
    """The written masks opened, then closed by the disc of that radius (on the GPU, csrc/mask_distance.hip; cpu=True: the numpy
    statement).  A device-resident result is fetched first."""
    from mnc_amd import distance
    r2 = distance.radius_sq(radius)
    if cpu:
        return distance.morph_numpy(distance.morph_numpy(packed.fetch(), "open", r2), "close", r2)
    return packed.open(r2=r2).close(r2=r2)


def _exclusive(packed, cpu=False):
    """The written masks made pairwise disjoint, each minus every better-scoring one (on the GPU, csrc/mask_algebra.hip; cpu=True:
    the numpy statement).  A device-resident result is fetched first."""
    from mnc_amd import algebra
    return algebra.layer_numpy(packed.fetch()) if cpu else packed.layered()


def _flip_tta(packed, mirrored, width, thresh=0.5, cpu=False):
    """The masks of an image merged with those of its mirror image: `mirrored` flipped back into the frame of the image `width`
    wide (on the GPU, csrc/mask_warp.hip; cpu=True: the numpy statement), the two sets concatenated, and the class-aware mask NMS
    at IoU `thresh` over both (cpu=True: mask_nms_numpy) -> a host PackedMasks of the kept instances, those of `packed` first,
    each part in its own order.  Device-resident results are fetched first."""
    from mnc_amd import warp
    from mnc_amd.masks import PackedMasks, mask_nms_numpy, merge_sets
    packed, mirrored = packed.fetch(), mirrored.fetch()
    back = warp.isometry_numpy(mirrored, 2, int(width) - 1, 0) if cpu else mirrored.fliplr(width)
    parts = (packed, back)
    bounds, offsets, areas, bits = merge_sets(parts, [(p, i) for p in (0, 1) for i in range(len(parts[p]))])
    both = PackedMasks(bounds, offsets, areas, np.concatenate((packed.classes, back.classes)),
                       np.concatenate((packed.scores, back.scores)), bits)
    keep = mask_nms_numpy(both, thresh, class_aware=True) if cpu else both.nms(thresh, class_aware=True)
    return both.take(np.sort(keep))


def _coco_results(image_id, im_shape, packed, cpu=False):
    """-> COCO result entries of one image's PackedMasks: the mask run-length encoded in the image (on the GPU where the masks
    lie, csrc/mask_rle.hip; cpu=True: mnc_amd.rle's numpy statement), bbox = [x, y, w, h] of the tight box of its pixels."""
    from mnc_amd import rle
    h, w = im_shape[:2]
    run_ptr, runs = rle.rle_counts_numpy(packed, h, w) if cpu else packed.rle_counts(h, w)
    out = []
    for i in range(len(packed)):
        c = runs[run_ptr[i]:run_ptr[i + 1]]
        # rleToBbox: the odd positions of the running sum are where the runs of 1 begin, the even ones where they end
        edge = np.cumsum(c.astype(np.int64))[:len(c) // 2 * 2].reshape(-1, 2)
        edge = edge[edge[:, 1] > edge[:, 0]]
        if len(edge):
            xs, xe = edge[:, 0] // h, (edge[:, 1] - 1) // h
            ys, ye = np.where(xs == xe, edge[:, 0] % h, 0), np.where(xs == xe, (edge[:, 1] - 1) % h, h - 1)
            bbox = [int(xs.min()), int(ys.min()), int(xe.max() - xs.min() + 1), int(ye.max() - ys.min() + 1)]
        else:
            bbox = [0, 0, 0, 0]
        out.append({"image_id": image_id, "category_id": int(packed.classes[i]),
                    "segmentation": {"size": [int(h), int(w)], "counts": rle.counts_to_string(c)}, "bbox": bbox,
                    "score": float(packed.scores[i])})
    return out


def _coco_annotations(image_id, packed, first_id=1, cpu=False, epsilon=0.0, oriented=False, image=None):
    """-> COCO annotation entries of one image's PackedMasks: segmentation = the outer loops of the 8-connected outline as polygons
    (on the GPU, csrc/mask_contours.hip; cpu=True: the numpy statement), bbox = [x, y, w, h] of the polygons' extent (the tight box
    of the mask's pixels; with epsilon > 0 the extent of the polygons written), area = the mask's pixel count, iscrowd 0.  An
    instance without a set pixel has no polygons.  epsilon > 0 simplifies the loops to that many pixels (csrc/contour_simplify.hip;
    cpu=True: simplify_numpy).  oriented: "rbox" = [cx, cy, w, h, angle] of the rectangle of least area (null for an instance
    without a set pixel) and "solidity" = area over convex hull area as well (csrc/mask_shape.hip; cpu=True: the numpy statements
    of mnc_amd.shape).  image, the uint8 BGR image [H, W, 3]: "mean_color" = [R, G, B] and "std_color", the mean and the standard
    deviation of its colours under the mask (csrc/mask_pixels.hip; cpu=True: pixel_stats_numpy), both null for an instance
    without a pixel.  A device-resident result is fetched first."""
    from mnc_amd import contours
    packed = packed.fetch()
    c = contours.contours_numpy(packed, 8) if cpu else packed.contours(8)
    if epsilon != 0:
        c = contours.simplify_numpy(c, epsilon) if cpu else c.simplify(epsilon)
    out = []
    for i in range(len(packed)):
        outer = [xy for xy, area in c.loops(i) if area > 0]
        if outer:
            lo, hi = np.min([xy.min(axis=0) for xy in outer], axis=0), np.max([xy.max(axis=0) for xy in outer], axis=0)
            bbox = [float(lo[0]), float(lo[1]), float(hi[0] - lo[0]), float(hi[1] - lo[1])]
        else:
            bbox = [0.0, 0.0, 0.0, 0.0]
        out.append({"id": first_id + i, "image_id": image_id, "category_id": int(packed.classes[i]), "segmentation": c.polygons(i),
                    "bbox": bbox, "area": float(packed.areas[i]), "iscrowd": 0, "score": float(packed.scores[i])})
    if oriented:
        from mnc_amd import shape
        hulls = shape.hull_numpy(packed) if cpu else packed.hull()
        rbox = (shape.oriented_numpy(packed, hulls) if cpu else packed.oriented_boxes()).rbox()
        for i, solidity in enumerate(hulls.solidity(packed.areas)):
            out[i]["rbox"] = [float(v) for v in rbox[i]] if hulls.area2[i] else None
            out[i]["solidity"] = float(solidity)
    if image is not None:
        from mnc_amd import pixels
        stats = pixels.pixel_stats_numpy(packed, image) if cpu else packed.pixel_stats(image)
        mean, std = stats.mean()[:, ::-1], stats.std()[:, ::-1]               # (BGR -> RGB)
        for i in range(len(packed)):
            out[i]["mean_color"] = [float(v) for v in mean[i]] if stats.count[i] else None
            out[i]["std_color"] = [float(v) for v in std[i]] if stats.count[i] else None
    return out


def _save_masks(out_dir, name, im_shape, result_mask, result_box, view=None, score_thresh=0.5, cpu=False, packed=None):
    """The instances scoring >= score_thresh (_packed_masks) -> <out_dir>/<name>_masks.npz (mnc_amd.masks.PackedMasks.load reads
    it back)."""
    if packed is None:
        packed = _packed_masks(im_shape, result_mask, result_box, view, score_thresh, cpu)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, name + "_masks.npz")
    np.savez(out, **packed.arrays())
    return out, packed


def _save_panoptic(out_dir, name, im_shape, packed, cpu=False):
    """The label map of one image's PackedMasks -- every pixel the index + 1 of the best-scoring instance that covers it, 0 where
    none does (on the GPU, csrc/mask_labels.hip; cpu=True: the numpy statement) -> <out_dir>/<name>.png by the panoptic id rule
    (id = R + 256 G + 65536 B) and the annotation entry {image_id, file_name, segments_info} of the segments that kept a pixel.
    A device-resident result is fetched first."""
    from PIL import Image
    from mnc_amd import labels
    h, w = im_shape[:2]
    packed = packed.fetch()
    seg = labels.to_labels_numpy(packed, h, w) if cpu else packed.to_labels(h, w)
    os.makedirs(out_dir, exist_ok=True)
    Image.fromarray(labels.id_to_rgb(seg), "RGB").save(os.path.join(out_dir, name + ".png"))
    area = np.bincount(seg.reshape(-1), minlength=len(packed) + 1)[1:]
    info = [dict(s, area=int(area[k])) for k, s in enumerate(labels.segments_info(packed, np.arange(1, len(packed) + 1))) if area[k]]
    return {"image_id": name, "file_name": name + ".png", "segments_info": info}


def build_net(args):
    from mnc_amd import models, synth
    prototxt = args.prototxt or models.write_mnc_5stage_test_prototxt()
    if args.caffemodel:
        weights = args.caffemodel
    else:
        print("no --net given: using seeded synthetic weights (detections are meaningless, timing is not)")
        weights = synth.synthetic_weights(prototxt, seed=0)
    caffe.set_mode_gpu()
    caffe.set_device(args.gpu_id)
    cfg.GPU_ID = args.gpu_id
    return caffe.Net(prototxt, weights, caffe.TEST)


def main(argv=None):
    args = parse_args(argv)
    if args.device_vis:
        cfg.TEST.USE_GPU_VIS = True
    net = build_net(args)
    warm = 128 * np.ones((300, 500, 3), dtype=np.float32)
    for _ in range(2):
        im_detect(warm, net)
    images = args.images
    if images is None:
        demo_dir = os.path.join(cfg.DATA_DIR, "demo")
        images = sorted(os.path.join(demo_dir, f) for f in os.listdir(demo_dir)) if os.path.isdir(demo_dir) else []
    if not images:
        print("no images given; running one synthetic 600x1000 image")
        images = [None]
    coco, annotations, image_entries, panoptic = [], [], [], []
    for path in images:
        print("~" * 35)
        print("Demo for {}".format(path or "<synthetic 600x1000>"))
        im = _read_image_bgr(path) if path else np.random.default_rng(0).integers(0, 256, (600, 1000, 3), dtype=np.uint8)
        start = time.time()
        boxes, masks, seg_scores = im_detect(im, net)
        print("forward time %f" % (time.time() - start))
        start = time.time()
        result_mask, result_box = gpu_mask_voting(masks, boxes, seg_scores, len(CLASSES) + 1, 100, im.shape[1], im.shape[0])
        print("mask voting time %f" % (time.time() - start))
        pred = get_vis_dict(result_box, result_mask, path or "synthetic", CLASSES, args.vis_thresh)
        print("%d instances with score >= %g" % (len(pred["boxes"]), args.vis_thresh))
        if args.save_masks or args.save_coco or args.save_annotations or args.save_panoptic:
            from mnc_amd.devarray import DeviceArray
            blk = getattr(boxes._net, "_inst", None) if isinstance(boxes, DeviceArray) else None
            name = os.path.splitext(os.path.basename(path))[0] if path else "synthetic"
            packed = _packed_masks(im.shape, result_mask, result_box, blk.view() if blk is not None else None, args.vis_thresh,
                                   args.cpu_mode)
            if args.flip_tta:
                packed = packed.fetch()                           # (the mirrored run reuses the device buffers)
                m_boxes, m_masks, m_scores = im_detect(np.ascontiguousarray(im[:, ::-1]), net)
                m_mask, m_box = gpu_mask_voting(m_masks, m_boxes, m_scores, len(CLASSES) + 1, 100, im.shape[1], im.shape[0])
                m_blk = getattr(m_boxes._net, "_inst", None) if isinstance(m_boxes, DeviceArray) else None
                mirrored = _packed_masks(im.shape, m_mask, m_box, m_blk.view() if m_blk is not None else None, args.vis_thresh,
                                         args.cpu_mode)
                packed = _flip_tta(packed, mirrored, im.shape[1], args.tta_nms, args.cpu_mode)
                print("%d instances after merging with the mirrored run" % len(packed))
            if args.smooth_radius > 0:
                packed = _smooth(packed, args.smooth_radius, args.cpu_mode)
            if args.exclusive:
                packed = _exclusive(packed, args.cpu_mode)
            if args.min_component_area > 0 or args.largest_component:
                packed = _select_components(packed, args.min_component_area, args.largest_component, args.cpu_mode)
            if args.save_coco:                                    # (first: a device-resident result is encoded where it lies)
                coco.extend(_coco_results(name, im.shape, packed, args.cpu_mode))
            if args.save_annotations:
                image_entries.append({"id": name, "file_name": os.path.basename(path) if path else name, "height": int(im.shape[0]),
                                      "width": int(im.shape[1])})
                annotations.extend(_coco_annotations(name, packed, len(annotations) + 1, args.cpu_mode, args.polygon_epsilon,
                                                     args.oriented_boxes, im if args.pixel_stats else None))
            if args.save_panoptic:
                panoptic.append(_save_panoptic(args.save_panoptic, name, im.shape, packed, args.cpu_mode))
                print("wrote %s.png (%d segments)" % (os.path.join(args.save_panoptic, name), len(panoptic[-1]["segments_info"])))
            if args.save_masks:
                out, packed = _save_masks(args.save_masks, name, im.shape, result_mask, result_box, packed=packed)
                print("wrote %s (%d masks, %d bytes of bits)" % (out, len(packed), packed.bits.nbytes))
        if args.vis and path:
            out = os.path.splitext(path)[0] + "_mnc.png"
            if args.out_dir:
                os.makedirs(args.out_dir, exist_ok=True)
                out = os.path.join(args.out_dir, os.path.basename(out))
            # with the results on the device, the overlay is rendered from the voting's own record block; `pred` (from the records
            # fetched for the count above) only places the text labels
            from mnc_amd.devarray import DeviceArray
            blk = getattr(boxes._net, "_inst", None) if isinstance(boxes, DeviceArray) else None
            # (after --flip-tta's mirrored run the block holds the mirror image's records: the overlay then is the host's)
            flipped = args.flip_tta and (args.save_masks or args.save_coco or args.save_annotations or args.save_panoptic)
            view = blk.view() if cfg.TEST.USE_GPU_VIS and blk is not None and im.dtype == np.uint8 and not flipped else None
            _visualise(im, pred, out, view, args.vis_thresh)
            print("wrote", out)
    if args.save_coco:
        import json
        with open(args.save_coco, "w") as f:
            json.dump(coco, f)
        print("wrote %s (%d instances)" % (args.save_coco, len(coco)))
    if args.save_panoptic:
        import json
        with open(os.path.join(args.save_panoptic, "panoptic.json"), "w") as f:
            json.dump({"annotations": panoptic, "categories": [{"id": k + 1, "name": c, "isthing": 1} for k, c in enumerate(CLASSES)]}, f)
        print("wrote %s (%d images)" % (os.path.join(args.save_panoptic, "panoptic.json"), len(panoptic)))
    if args.save_annotations:
        import json
        with open(args.save_annotations, "w") as f:
            json.dump({"images": image_entries, "categories": [{"id": k + 1, "name": c} for k, c in enumerate(CLASSES)],
                       "annotations": annotations}, f)
        print("wrote %s (%d annotations of %d images)" % (args.save_annotations, len(annotations), len(image_entries)))
    net.close()


if __name__ == "__main__":
    main()
