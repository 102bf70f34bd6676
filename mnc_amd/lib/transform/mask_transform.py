"""`transform.mask_transform.gpu_mask_voting` (reference: lib/transform/mask_transform.py:213-286).

Host orchestration only: 20 per-class NMS calls (HIP), a global score threshold, one IoU row per surviving box, then a
single call into the fused HIP mask-voting kernels (nms.mv.mv).  The reference's cv2-based cpu_mask_voting (image-space voting,
cfg.TEST.USE_GPU_MASK_MERGE = False) runs on the GPU as well: cpu_mask_voting below (csrc/mv_image.hip).  instance_masks turns the
voted instances into per-instance binary masks at image resolution on the GPU (csrc/inst_masks.hip); instance_masks_numpy is the
same rule as a plain loop on the host; mask_rle / masks_from_rle take them to COCO's run-length encoding and back (csrc/mask_rle.hip);
mask_match matches detections to ground truths by COCO's rule (csrc/mask_match.hip), mask_match_numpy is its statement on the host."""
import numpy as np

from mnc_config import cfg
from nms.gpu_nms import gpu_nms_batched
from nms.nms_wrapper import nms
from nms.mv import mv
from utils.cython_bbox import bbox_overlaps


def build_voting_candidates(boxes, scores, num_classes, max_per_image):
    """-> (candidate_inds i32[C], candidate_start i32[R] (END offsets), candidate_weights f32[C],
           candidate_scores f32[R], class_bar list[num_classes-1])."""
    boxes32 = boxes.astype(np.float32)
    kept = {}
    pool = []
    if cfg.USE_GPU_NMS and boxes32.shape[0] > 0:
        # the 20 per-class problems share the box set: one batched device call instead of 20 synchronous ones; only the
        # first max_per_image survivors of each class are used below, so the scan stops there (identical prefix)
        per_class = gpu_nms_batched(boxes32, scores[:, 1:num_classes], cfg.TEST.MASK_MERGE_NMS_THRESH,
                                    device_id=cfg.GPU_ID, max_keep=max_per_image)
    else:
        per_class = [nms(np.hstack((boxes32, scores[:, c:c + 1])), cfg.TEST.MASK_MERGE_NMS_THRESH)
                     for c in range(1, num_classes)]
    for c in range(1, num_classes):
        order = per_class[c - 1][:max_per_image]
        kept[c] = (boxes[order], scores[order, c])
        pool.extend(kept[c][1])
    if not pool:      # the reference would raise IndexError here (mask_transform.py:244); nothing to vote on
        z = np.zeros(0, np.int32)
        return z, z.copy(), np.zeros(0, np.float32), np.zeros(0, np.float32), [0] * (num_classes - 1)
    ranked = np.sort(pool)[::-1]
    thresh = ranked[min(len(ranked), max_per_image) - 1]
    boxes64 = boxes.astype(np.float64)
    inds, weights, ends, out_scores, class_bar = [], [], [], [], []
    for c in range(1, num_classes):
        cls_boxes, cls_scores = kept[c]
        sel = np.where(cls_scores >= thresh)[0]
        for b in cls_boxes[sel]:
            ov = bbox_overlaps(boxes64, b[np.newaxis].astype(np.float64))
            members = np.where(ov >= cfg.TEST.MASK_MERGE_IOU_THRESH)[0]
            w = scores[members, c]
            # python's sum() as the reference ran it (:266, numpy 1.x): sequential float64 accumulation (0 + np.float32 promoted
            # to float64), then a float32 division by that scalar (value-based casting)
            w = w / np.float32(sum(w.astype(np.float64)))
            inds.extend(members)
            weights.extend(w)
            ends.append(len(inds))
        out_scores.extend(cls_scores[sel])
        class_bar.append(len(out_scores))
    return (np.array(inds, dtype=np.int32), np.array(ends, dtype=np.int32), np.array(weights, dtype=np.float32),
            np.array(out_scores, dtype=np.float32), class_bar)


def mask_overlap(box1, box2, mask1, mask2):
    """Region IoU of two boolean masks that live inside different integer boxes (mask_transform.py:16-46; used by the
    mAP^r evaluation, utils/voc_eval.py)."""
    x1, y1 = max(box1[0], box2[0]), max(box1[1], box2[1])
    x2, y2 = min(box1[2], box2[2]), min(box1[3], box2[3])
    if x1 > x2 or y1 > y2:
        return 0
    w, h = x2 - x1 + 1, y2 - y1 + 1
    ya, xa = y1 - box1[1], x1 - box1[0]
    yb, xb = y1 - box2[1], x1 - box2[0]
    inter_a = mask1[ya: ya + h, xa: xa + w]
    inter_b = mask2[yb: yb + h, xb: xb + w]
    assert inter_a.shape == inter_b.shape
    inter = np.logical_and(inter_b, inter_a).sum()
    union = mask1.sum() + mask2.sum() - inter
    if union < 1.0:
        return 0
    return float(inter) / float(union)


def intersect_mask(ex_box, gt_box, gt_mask):
    """The mask regression target of one box (mask_transform.py:49-80): gt_mask, the ground-truth mask inside the integer box
    gt_box, pasted where it meets ex_box on a float32 canvas of ex_box's size, resized to cfg.MASK_SIZE x cfg.MASK_SIZE and
    binarised with >= cfg.BINARIZE_THRESH -> bool [S, S]; zeros (21 x 21 in the reference) when the boxes do not meet.  A thin
    host statement: mnc_amd.targets.mask_targets does all rows of a layer in one device call."""
    from utils.blob import resize_to
    x1, y1 = max(ex_box[0], gt_box[0]), max(ex_box[1], gt_box[1])
    x2, y2 = min(ex_box[2], gt_box[2]), min(ex_box[3], gt_box[3])
    if x1 > x2 or y1 > y2:
        return np.zeros((cfg.MASK_SIZE, cfg.MASK_SIZE), dtype=bool)
    w, h = x2 - x1 + 1, y2 - y1 + 1
    ey, ex, gy, gx = y1 - ex_box[1], x1 - ex_box[0], y1 - gt_box[1], x1 - gt_box[0]
    canvas = np.zeros((ex_box[3] - ex_box[1] + 1, ex_box[2] - ex_box[0] + 1))
    canvas[ey: ey + h, ex: ex + w] = gt_mask[gy: gy + h, gx: gx + w]
    return resize_to(canvas.astype(np.float32), cfg.MASK_SIZE, cfg.MASK_SIZE) >= cfg.BINARIZE_THRESH


def _fused_mask_voting(masks, boxes, scores, num_classes, max_per_image, im_width, im_height):
    """The whole of gpu_mask_voting in one C-ABI call (mnc_mask_voting): per-class score order, batched per-class NMS,
    candidate sets and the fused voting kernels, all on the device with no Python between the steps.  The per-class
    order is np.argsort(-scores[:, c], kind="stable") (ties in index order), computed by the library."""
    import ctypes
    from mnc_amd import _lib
    n = boxes.shape[0]
    S = masks.shape[3]
    B = num_classes - 1
    masks = np.ascontiguousarray(masks, dtype=np.float32)
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    cap = B * min(max_per_image, n)
    out_mask = np.zeros((cap, 1, S, S), dtype=np.float32)
    out_box = np.zeros((cap, 4), dtype=np.int32)
    out_score = np.zeros(cap, dtype=np.float32)
    counts = np.zeros(B, dtype=np.int32)
    R = ctypes.c_int(0)
    _lib.call("mnc_mask_voting", _lib.ptr(boxes), _lib.ptr(masks), _lib.ptr(scores), None, n, num_classes, S,
              int(max_per_image), float(cfg.TEST.MASK_MERGE_NMS_THRESH), float(cfg.TEST.MASK_MERGE_IOU_THRESH),
              int(im_height), int(im_width), _lib.ptr(out_mask), _lib.ptr(out_box), _lib.ptr(out_score),
              _lib.ptr(counts), ctypes.addressof(R), int(cfg.GPU_ID))
    return _split_results(out_mask, out_box, out_score, counts, R.value, B)


def _split_results(out_mask, out_box, out_score, counts, R, B):
    result_box = np.hstack((out_box[:R], out_score[:R, np.newaxis]))       # int32 | float32 -> float64, as the reference
    list_mask, list_box, lo = [], [], 0
    for c in range(B):
        hi = lo + int(counts[c])
        list_box.append(result_box[lo:hi, :])
        list_mask.append(out_mask[lo:hi])
        lo = hi
    return list_mask, list_box


def _device_mask_voting(masks, boxes, scores, num_classes, max_per_image, im_width, im_height):
    """gpu_mask_voting on the engine's own device-resident outputs (mnc_amd.devarray.DeviceArray, from Net.detect_tail):
    order, per-class NMS, threshold, result rows, candidate sets and voting as one asynchronous launch sequence on the net's
    stream (mnc_vote_instances); the only host contact is the copy of the final records."""
    blk = boxes._net.vote_instances(boxes, masks, scores, num_classes, max_per_image, im_width, im_height,
                                    cfg.TEST.MASK_MERGE_NMS_THRESH, cfg.TEST.MASK_MERGE_IOU_THRESH)
    return blk.lists()


def gpu_mask_voting(masks, boxes, scores, num_classes, max_per_image, im_width, im_height):
    """masks [n,1,S,S], boxes [n,4], scores [n,num_classes] -> (list_result_mask, list_result_box), one entry per
    foreground class; boxes rows are [x1, y1, x2, y2, score]."""
    from mnc_amd.devarray import DeviceArray
    if cfg.USE_GPU_NMS and all(isinstance(a, DeviceArray) for a in (masks, boxes, scores)) and boxes.shape[0] > 0:
        return _device_mask_voting(masks, boxes, scores, num_classes, max_per_image, im_width, im_height)
    masks, boxes, scores = (np.asarray(a) for a in (masks, boxes, scores))
    if (cfg.USE_GPU_NMS and boxes.dtype == np.float32 and scores.dtype == np.float32 and boxes.shape[0] > 0
            and boxes.shape[1] == 4 and masks.shape[2] == masks.shape[3]):
        return _fused_mask_voting(masks, boxes, scores, num_classes, max_per_image, im_width, im_height)
    # generic path (float64 boxes, CPU NMS, ...): the reference's step-by-step composition
    inds, ends, weights, out_scores, class_bar = build_voting_candidates(boxes, scores, num_classes, max_per_image)
    result_mask, result_box = mv(boxes.astype(np.float32), masks, inds, ends, weights, im_height, im_width,
                                 device_id=cfg.GPU_ID)
    result_box = np.hstack((result_box, out_scores[:, np.newaxis]))
    list_mask, list_box = [], []
    lo = 0
    for hi in class_bar:
        list_box.append(result_box[lo:hi, :])
        list_mask.append(result_mask[lo:hi, :, :, :])
        lo = hi
    return list_mask, list_box


def _image_voting_lists(rec, class_counts, S):
    """records [R, 6+S*S] -> (result_box, result_mask) as cpu_mask_voting returns them: per class boxes [k,5] float64 and masks
    [k,1,S,S] float64 (its float64 arrays, filled from float32 values)."""
    boxes = rec[:, :5].astype(np.float64)
    masks = rec[:, 6:].astype(np.float64).reshape(-1, 1, S, S)
    result_box, result_mask, lo = [], [], 0
    for k in class_counts:
        hi = lo + int(k)
        result_box.append(boxes[lo:hi])
        result_mask.append(masks[lo:hi])
        lo = hi
    return result_box, result_mask


def cpu_mask_voting(masks, boxes, scores, num_classes, max_per_image, im_width, im_height):
    """The reference's image-space mask voting (mask_transform.py:142-210, cfg.TEST.USE_GPU_MASK_MERGE = False) on the GPU:
    masks [n,1,S,S], boxes [n,4] float32, scores [n,num_classes] -> (result_box, result_mask), one entry per foreground class,
    boxes [k,5] = (x1, y1, x2, y2, score) and masks [k,1,S,S], both float64 (note the order: gpu_mask_voting returns masks first).
    Per-class NMS, threshold and candidate sets as gpu_mask_voting; a class's kept boxes re-sorted by argsort()[::-1] pinned as
    stable-ascending-reversed (equal scores in reverse keep order); each mask resized to its rounded box with cv2's bilinear
    rule, binarised at cfg.BINARIZE_THRESH and summed with its weight on a float64 image canvas (mnc_mask_voting_image /
    mnc_vote_instances_ex).  n == 0 gives empty classes."""
    import ctypes
    from mnc_amd import _lib
    from mnc_amd.devarray import DeviceArray
    if not cfg.USE_GPU_NMS:
        raise NotImplementedError("cpu_mask_voting with cfg.USE_GPU_NMS=False (cpu_nms.pyx's rule) is not provided")
    B = num_classes - 1
    S = masks.shape[-1]
    n = boxes.shape[0]
    if n == 0:
        return [np.zeros((0, 5)) for _ in range(B)], [np.zeros((0, 1, S, S)) for _ in range(B)]
    if all(isinstance(a, DeviceArray) for a in (masks, boxes, scores)):
        blk = boxes._net.vote_instances(boxes, masks, scores, num_classes, max_per_image, im_width, im_height,
                                        cfg.TEST.MASK_MERGE_NMS_THRESH, cfg.TEST.MASK_MERGE_IOU_THRESH, mode="image",
                                        binarize_thresh=cfg.BINARIZE_THRESH)
        counts, rec = blk.fetch()
        return _image_voting_lists(rec, counts[1:num_classes], S)
    masks = np.ascontiguousarray(np.asarray(masks), dtype=np.float32)
    boxes = np.ascontiguousarray(np.asarray(boxes), dtype=np.float32)
    scores = np.ascontiguousarray(np.asarray(scores), dtype=np.float32)
    cap = B * min(max_per_image, n)
    out_mask = np.zeros((cap, S * S), dtype=np.float32)
    out_box = np.zeros((cap, 4), dtype=np.int32)
    out_score = np.zeros(cap, dtype=np.float32)
    counts = np.zeros(B, dtype=np.int32)
    R = ctypes.c_int(0)
    _lib.call("mnc_mask_voting_image", _lib.ptr(boxes), _lib.ptr(masks), _lib.ptr(scores), n, num_classes, S,
              int(max_per_image), float(cfg.TEST.MASK_MERGE_NMS_THRESH), float(cfg.TEST.MASK_MERGE_IOU_THRESH),
              float(cfg.BINARIZE_THRESH), int(im_height), int(im_width), _lib.ptr(out_mask), _lib.ptr(out_box),
              _lib.ptr(out_score), _lib.ptr(counts), ctypes.addressof(R), int(cfg.GPU_ID))
    R = R.value
    rec = np.hstack((out_box[:R].astype(np.float32), out_score[:R, None], np.zeros((R, 1), np.float32), out_mask[:R]))
    return _image_voting_lists(rec, counts, S)


def instance_masks(boxes, masks, im_h, im_w, clip=True, binarize_thresh=None, classes=None, scores=None):
    """Per-instance binary masks at image resolution on the GPU (mnc_instance_masks): boxes [n, 4 or 5], masks [n, S, S] or
    [n, 1, S, S] -> mnc_amd.masks.PackedMasks.  Each box is rounded half to even and, with clip=True, clipped to the image
    (utils/vis_seg.py:_convert_pred_to_image; clip=False is utils/voc_eval.py:voc_eval_sds's rule); the mask is resized to it with
    cv2's INTER_LINEAR rule and binarised with >= float32(cfg.BINARIZE_THRESH)."""
    from mnc_amd.masks import instance_masks as device_masks
    return device_masks(boxes, masks, im_h, im_w, clip, binarize_thresh, classes, scores, cfg.GPU_ID)


def instance_masks_numpy(boxes, masks, im_h, im_w, clip=True, binarize_thresh=None, classes=None, scores=None):
    """instance_masks as the plain utils.blob.resize_to loop on the host: the CPU statement of the rule, the same PackedMasks."""
    from mnc_amd.masks import instance_masks_numpy as host_masks
    return host_masks(boxes, masks, im_h, im_w, clip, binarize_thresh, classes, scores)


def mask_overlaps(a, b=None):
    """mask_overlap of every pair of two mnc_amd.masks.PackedMasks (b None: a against itself) on the GPU (mnc_mask_overlaps):
    -> (inter int64 [na, nb], iou float64 [na, nb])."""
    from mnc_amd.masks import mask_overlaps as device_overlaps
    return device_overlaps(a, b, cfg.GPU_ID)


def masks_from_labels(label, cls=None, background=0, classes=None):
    """The instances of an integer label map (SBD's inst / cls arrays, Cityscapes' instanceIds, panoptic ids, superpixels) on the
    GPU (mnc_label_table + mnc_label_masks, csrc/mask_labels.hip) -> (mnc_amd.masks.PackedMasks, ids int32 [n])."""
    from mnc_amd.labels import from_labels as device_from_labels
    return device_from_labels(label, cls, background, classes, cfg.GPU_ID)


def masks_from_labels_numpy(label, cls=None, background=0, classes=None):
    """masks_from_labels as plain numpy on the host: the CPU statement of the rule."""
    from mnc_amd.labels import from_labels_numpy as host_from_labels
    return host_from_labels(label, cls, background, classes)


def mask_labels(pm, H, W, values=None, order=None, background=0):
    """The label map int32 [H, W] of a PackedMasks on the GPU (mnc_mask_to_labels): every pixel gets the value of the first
    instance in `order` (None: descending score) that covers it."""
    return pm.to_labels(H, W, values, order, background, device_id=cfg.GPU_ID)


def mask_labels_numpy(pm, H, W, values=None, order=None, background=0):
    """mask_labels as the plain painting loop on the host: the CPU statement of the rule."""
    from mnc_amd.labels import to_labels_numpy as host_to_labels
    return host_to_labels(pm, H, W, values, order, background)


def mask_overlaps_numpy(a, b=None):
    """mask_overlaps as the plain double loop over mask_overlap on the host: the CPU statement of the rule."""
    from mnc_amd.masks import mask_overlaps_numpy as host_overlaps
    return host_overlaps(a, b)


def mask_nms(pm, thresh, class_aware=False):
    """Greedy suppression of a PackedMasks by mask IoU in score order on the GPU (mnc_mask_nms) -> kept indices int32."""
    from mnc_amd.masks import mask_nms as device_nms
    return device_nms(pm, thresh, class_aware, cfg.GPU_ID)


def mask_nms_numpy(pm, thresh, class_aware=False):
    """mask_nms as a plain loop on the host: the CPU statement of the rule."""
    from mnc_amd.masks import mask_nms_numpy as host_nms
    return host_nms(pm, thresh, class_aware)


def mask_match(dt, gt, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, return_iou=False):
    """COCO's matching of one image's detections to its ground truths (two mnc_amd.masks.PackedMasks) on the GPU (mnc_mask_match /
    mnc_mask_match_dev, csrc/mask_match.hip) -> mnc_amd.coco_eval.Match."""
    return dt.match(gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, return_iou, cfg.GPU_ID)


def mask_match_numpy(dt, gt, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, return_iou=False):
    """mask_match as evaluateImg's plain loop on the host: the CPU statement of the rule."""
    from mnc_amd.coco_eval import match_numpy as host_match
    return host_match(dt, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, return_iou)


def mask_boundary(pm, H, W, d=None):
    """The boundary bands of a PackedMasks in an H x W image at distance d (None: 2 % of the image diagonal, rounded) on the GPU
    (mnc_mask_boundary, csrc/mask_boundary.hip) -> mnc_amd.masks.PackedMasks in the same layout."""
    return pm.boundary(H, W, d, device_id=cfg.GPU_ID)


def mask_distance(pm):
    """The squared Euclidean inside distances of a PackedMasks on the GPU (mnc_mask_distance, csrc/mask_distance.hip) ->
    mnc_amd.distance.DistanceMaps(dist_ptr, sq, shapes)."""
    return pm.distance(device_id=cfg.GPU_ID)


def mask_inscribed(pm):
    """The centre and squared radius of the largest inscribed disc of every instance on the GPU (mnc_mask_inscribed) -> (xy int32
    [n, 2], r2 int32 [n])."""
    return pm.inscribed(device_id=cfg.GPU_ID)


def mask_erode(pm, radius=None, r2=None):
    """A PackedMasks eroded by the disc of that radius (or exact squared radius r2) on the GPU (mnc_mask_morph) ->
    mnc_amd.masks.PackedMasks with the input's bounds."""
    return pm.erode(radius, r2, device_id=cfg.GPU_ID)


def mask_dilate(pm, radius=None, r2=None, H=None, W=None):
    """A PackedMasks dilated by the disc on the GPU (mnc_mask_morph) -> mnc_amd.masks.PackedMasks with the bounds grown by
    isqrt(r2), with H, W clipped to the image."""
    return pm.dilate(radius, r2, H, W, device_id=cfg.GPU_ID)


def mask_open(pm, radius=None, r2=None):
    """dilate(erode) of a PackedMasks by the disc on the GPU (mnc_mask_morph) -> mnc_amd.masks.PackedMasks with the input's bounds."""
    return pm.open(radius, r2, device_id=cfg.GPU_ID)


def mask_close(pm, radius=None, r2=None):
    """erode(dilate) of a PackedMasks by the disc on the GPU (mnc_mask_morph) -> mnc_amd.masks.PackedMasks with the input's bounds."""
    return pm.close(radius, r2, device_id=cfg.GPU_ID)


def mask_moments(pm):
    """The moments of order up to two of a PackedMasks on the GPU (mnc_mask_moments, csrc/mask_shape.hip) ->
    mnc_amd.shape.Moments(m int64 [n, 6], origin)."""
    return pm.moments(device_id=cfg.GPU_ID)


def mask_hull(pm):
    """The convex hulls of a PackedMasks on the GPU (mnc_mask_hull) -> mnc_amd.shape.Hulls(vert_ptr, xy, area2)."""
    return pm.hull(device_id=cfg.GPU_ID)


def mask_solidity(pm):
    """Pixel count over hull area of every instance of a PackedMasks on the GPU -> float64 [n]."""
    return pm.solidity(device_id=cfg.GPU_ID)


def mask_oriented_boxes(pm):
    """The rectangles of least area and the diameters of a PackedMasks on the GPU (mnc_mask_oriented) ->
    mnc_amd.shape.OrientedBoxes(box int64 [n, 8], diameter int64 [n, 3])."""
    return pm.oriented_boxes(device_id=cfg.GPU_ID)


def mask_pixel_stats(pm, image):
    """The pixel count, sums, extremes and their positions of an integer image [H, W] or [H, W, C] under every instance of a
    PackedMasks on the GPU (mnc_mask_pixel_stats, csrc/mask_pixels.hip) -> mnc_amd.pixels.PixelStats."""
    return pm.pixel_stats(image, device_id=cfg.GPU_ID)


def mask_histogram(pm, image, bins=256, lo=0, shift=0):
    """The histogram of an integer image's values under every instance of a PackedMasks on the GPU (mnc_mask_histogram) ->
    mnc_amd.pixels.MaskHistograms(hist int64 [n, C, bins], count, lo, shift, bins)."""
    return pm.histogram(image, bins, lo, shift, device_id=cfg.GPU_ID)


def mask_surface(pm):
    """The surfaces of a PackedMasks -- the pixels with an edge neighbour outside the mask -- on the GPU (mnc_mask_surface,
    csrc/mask_surface.hip) -> a host PackedMasks in the input's frames."""
    return pm.surface(device_id=cfg.GPU_ID)


def mask_surface_stats(a, b, pairs=None, tau2=()):
    """The distances between the surfaces of pairs (i, j) of instances of two PackedMasks, reduced, on the GPU
    (mnc_mask_surface_stats) -> mnc_amd.surface.SurfaceStats with .hausdorff(), .boundary_f(t) and .nsd(t)."""
    return a.surface_stats(b, pairs, tau2, device_id=cfg.GPU_ID)


def mask_surface_distances(a, b, pairs=None):
    """Those distances themselves on the GPU (mnc_mask_surface_dist) -> mnc_amd.surface.SurfaceDistances with .hd95() and
    .assd()."""
    return a.surface_distances(b, pairs, device_id=cfg.GPU_ID)


def mask_combine(a, b, op, window=None):
    """Two PackedMasks combined instance by instance on the GPU (mnc_mask_combine, csrc/mask_algebra.hip): op "and", "or",
    "xor", "minus", "copy" or "not", an optional window (x1, y1, x2, y2) -> a host PackedMasks with tight bounds."""
    return a.combine(b, op, window, device_id=cfg.GPU_ID)


def mask_merge(pm, groups=None, intersect=False, by=None):
    """The union (intersection) of groups of instances of a PackedMasks on the GPU (mnc_mask_merge): pycocotools' merge.  groups
    None: everything in one group; by="class": one group per distinct class -> a host PackedMasks, one instance per group."""
    return pm.merge(groups, intersect, by, device_id=cfg.GPU_ID)


def mask_layered(pm, order=None):
    """A PackedMasks made pairwise disjoint on the GPU (mnc_mask_layer): every pixel stays with the first instance in `order`
    (None: descending score) that covers it -> a host PackedMasks in the input's index order."""
    return pm.layered(order, device_id=cfg.GPU_ID)


def mask_isometry(pm, code, tx=0, ty=0):
    """A lattice isometry plus a translation of a PackedMasks on the GPU (mnc_mask_isometry, csrc/mask_warp.hip) -> a host
    PackedMasks with tight bounds."""
    return pm.isometry(code, tx, ty, device_id=cfg.GPU_ID)


def mask_fliplr(pm, W):
    """A PackedMasks mirrored left to right in an image W wide on the GPU (mnc_mask_isometry)."""
    return pm.fliplr(W, device_id=cfg.GPU_ID)


def mask_flipud(pm, H):
    """A PackedMasks mirrored top to bottom in an image H high on the GPU (mnc_mask_isometry)."""
    return pm.flipud(H, device_id=cfg.GPU_ID)


def mask_transpose(pm):
    """A PackedMasks with x and y exchanged on the GPU (mnc_mask_isometry)."""
    return pm.transpose(device_id=cfg.GPU_ID)


def mask_rot90(pm, k, H, W):
    """A PackedMasks of an H x W image turned by k quarter turns in numpy's direction on the GPU (mnc_mask_isometry)."""
    return pm.rot90(k, H, W, device_id=cfg.GPU_ID)


def mask_resize(pm, H, W, H2, W2):
    """A PackedMasks of an H x W image in its centre-aligned nearest-neighbour resize to H2 x W2 on the GPU (mnc_mask_warp)."""
    return pm.resize(H, W, H2, W2, device_id=cfg.GPU_ID)


def mask_warp_affine(pm, M, H2, W2, frac_bits=16, inverse=False):
    """A PackedMasks under a 2 x 3 matrix in cv2.warpAffine's convention, nearest neighbour, into an H2 x W2 image on the GPU
    (mnc_mask_warp)."""
    return pm.warp_affine(M, H2, W2, frac_bits, inverse, device_id=cfg.GPU_ID)


def mask_warp(pm, coef, den, window):
    """The nearest-neighbour gather of a PackedMasks through an integer affine inverse map on the GPU (mnc_mask_warp) -> a host
    PackedMasks with tight bounds inside the window."""
    return pm.warp(coef, den, window, device_id=cfg.GPU_ID)


def mask_match_boundary(dt, gt, H, W, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, d=None,
                        ratio=0.02, return_iou=False):
    """mask_match on the overlap min(mask IoU, boundary IoU) in an H x W image -- COCO's iouType "boundary" -- on the GPU
    (mnc_mask_match_boundary) -> mnc_amd.coco_eval.Match, with return_iou (Match, biou)."""
    return dt.match_boundary(gt, H, W, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, d, ratio, return_iou, cfg.GPU_ID)


def mask_components(pm, connectivity=8):
    """The connected components of a PackedMasks on the GPU (mnc_mask_components, csrc/mask_components.hip) ->
    mnc_amd.components.Components(comp_ptr, area, bbox, anchor)."""
    return pm.components(connectivity, device_id=cfg.GPU_ID)


def mask_select(pm, connectivity=8, min_area=1, keep=0):
    """The components of area >= min_area, with keep > 0 the `keep` largest of each instance, on the GPU (mnc_mask_select) ->
    mnc_amd.masks.PackedMasks in the input's layout."""
    return pm.select(connectivity, min_area, keep, device_id=cfg.GPU_ID)


def mask_fill_holes(pm, connectivity=4):
    """The masks OR their holes (background of this connectivity that does not reach the box's outside) on the GPU
    (mnc_mask_fill_holes) -> mnc_amd.masks.PackedMasks in the input's layout."""
    return pm.fill_holes(connectivity, device_id=cfg.GPU_ID)


def mask_split(pm, connectivity=8):
    """One instance per connected component on the GPU (mnc_mask_split) -> (mnc_amd.masks.PackedMasks, source int32 [C])."""
    return pm.split(connectivity, device_id=cfg.GPU_ID)


def mask_contours(pm, connectivity=8):
    """The outlines of a PackedMasks as closed rectilinear loops on the GPU (mnc_mask_contours, csrc/mask_contours.hip) ->
    mnc_amd.contours.Contours(loop_ptr, vert_ptr, area, xy)."""
    return pm.contours(connectivity, device_id=cfg.GPU_ID)


def mask_polygons(pm, connectivity=8, epsilon=0.0):
    """One COCO `segmentation` (a list of flat [x0, y0, x1, y1, ...] lists) per instance of a PackedMasks on the GPU: its outer
    loops, the holes dropped; with epsilon > 0 simplified to that many pixels (mnc_contours_simplify, csrc/contour_simplify.hip)."""
    return pm.polygons(connectivity, device_id=cfg.GPU_ID, epsilon=epsilon)


def mask_rle(pm, H, W):
    """COCO RLEs of a PackedMasks in an H x W image on the GPU (mnc_mask_rle / mnc_mask_rle_dev): -> [{"size": [H, W], "counts":
    str}] per instance."""
    from mnc_amd.rle import mask_rle as device_rle
    return device_rle(pm, H, W, cfg.GPU_ID)


def masks_from_rle(rles, classes=None, scores=None):
    """COCO RLEs of one image size -> mnc_amd.masks.PackedMasks with tight bounds on the GPU (mnc_mask_from_rle)."""
    from mnc_amd.rle import masks_from_rle as device_from_rle
    return device_from_rle(rles, classes, scores, cfg.GPU_ID)


def rle_counts_numpy(pm, H, W):
    """The run-length counts as plain numpy on the host: the CPU statement of the rule -> (run_ptr, runs)."""
    from mnc_amd.rle import rle_counts_numpy as host_counts
    return host_counts(pm, H, W)


def masks_from_counts_numpy(run_ptr, runs, H, W, classes=None, scores=None):
    """The reverse as plain numpy on the host: the CPU statement of the rule -> PackedMasks."""
    from mnc_amd.rle import masks_from_counts_numpy as host_masks
    return host_masks(run_ptr, runs, H, W, classes, scores)
