"""Training targets on packed ground-truth masks (include/mnc_hip.h n23, csrc/mask_targets.hip): the non-differentiable half of
the reference's training graph -- target assignment, mask regression targets and mask-overlap labels -- on
mnc_amd.masks.PackedMasks.

    mask_targets_numpy(gt, ex_boxes, gt_index, S=None, thresh=None)   -> uint8 [K, S, S]: the CPU statement of the reference's
                                                         intersect_mask (lib/transform/mask_transform.py:49-80) for K rows
    mask_targets(...)                                    the same through mnc_mask_targets (the GPU); PackedMasks.targets is the method
    mask_pred_overlaps_numpy(gt, boxes, preds, gt_index, thresh=None) -> (inter int64 [K], area_pred int64 [K], iou float64 [K]):
                                                         what MaskLayer.forward_train counts (lib/pylayer/mask_layer.py:68-83), as
                                                         the composition of instance_masks_numpy and mask_overlaps_numpy
    mask_pred_overlaps(...)                              the same through mnc_mask_pred_overlaps; PackedMasks.pred_overlaps
    pack_gt_masks(gt_boxes, gt_masks, mask_info, im_scale)   the reference's gt_masks / mask_info blobs -> the ground-truth set
    sample_rois(...) / stage_bridge_targets(...)         the logic of ProposalTargetLayer's _sample_rois and StageBridgeLayer's
                                                         _sample_output: box IoU through mnc_bbox_overlaps, the sampling and the
                                                         box regression targets in numpy on the host, the mask targets of all
                                                         foreground rows from one mask_targets call

The rules.  Ground truth is a PackedMasks whose bounds are the rounded, unscaled ground-truth boxes and whose masks have the
boxes' sizes.

    mask_targets   row k, with e = ex_boxes[k] (x1, y1, x2, y2 inclusive, int32), g = gt.bounds[gt_index[k]] and M =
                   gt.dense(gt_index[k]): all zeros when e and g do not intersect (an instance without rows intersects nothing);
                   else utils.blob.resize_to(C, S, S) >= np.float32(thresh), C the float32 canvas of e's size that is M on e & g
                   and 0 elsewhere.  S defaults to cfg.MASK_SIZE, thresh to cfg.BINARIZE_THRESH.
    pred_overlaps  row k is the mask of instance_masks_numpy(boxes[k:k+1], preds[k:k+1], clip=False, binarize_thresh=thresh):
                   np.round on the box, no clipping.  area_pred[k] = its set pixels, inter[k] = the pixels it shares with
                   instance gt_index[k]; a row with gt_index -1 (background) is skipped and gets zeros.  iou[k] follows on the
                   host by the reference's mask_overlap: union = area_pred + gt.areas[j] - inter, 0.0 where union < 1, else
                   inter / union.

Refused with ValueError, by the statements and the device functions alike (the library says MNC_ERR_INVALID, before anything is
launched): K outside [0, 65536]; S outside [1, 32]; a NaN thresh (mask_targets); a box with x2 < x1 or y2 < y1 (once rounded, for
pred_overlaps); a coordinate with |c| >= 2^24; a box of more than 2^26 pixels; gt_index outside [0, G), resp. [-1, G).  There is no
fallback: without the library or a GPU the device functions raise.  They read host arrays: a device-resident PackedMasks is
fetched first.  The box regression targets stay numpy on purpose: four floats for a few hundred rows, whose np.log runs on float32
in ProposalTargetLayer and on float64 in StageBridgeLayer."""
import numpy as np
import numpy.random as npr

from . import _lib
from .masks import MAX_AREA, MAX_COORD, MAX_MASK, PackedMasks, _device_id, _set_args

MAX_ROWS = 65536


def _defaults(S, thresh):
    from mnc_config import cfg
    return int(cfg.MASK_SIZE if S is None else S), float(cfg.BINARIZE_THRESH if thresh is None else thresh)


def _check_rows(who, K, S):
    if not 0 <= K <= MAX_ROWS:
        raise ValueError("%s: K=%d not in [0, %d]" % (who, K, MAX_ROWS))
    if not 1 <= S <= MAX_MASK:
        raise ValueError("%s: mask_size %d not in [1, %d]" % (who, S, MAX_MASK))


def _check_int_boxes(who, boxes):
    """boxes int [K, 4], already rounded: the coordinate, emptiness and pixel limits, the first offender named."""
    b = boxes.astype(np.int64)
    bad = np.nonzero((np.abs(b) >= MAX_COORD).any(1))[0]
    if bad.size:
        raise ValueError("%s: box %d coordinate out of range %s" % (who, bad[0], boxes[bad[0]]))
    w, h = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    bad = np.nonzero((w < 1) | (h < 1))[0]
    if bad.size:
        raise ValueError("%s: box %d %s is empty (cv2.resize would raise)" % (who, bad[0], boxes[bad[0]]))
    bad = np.nonzero(w * h > MAX_AREA)[0]
    if bad.size:
        raise ValueError("%s: box %d covers %d pixels (limit %d)" % (who, bad[0], (w * h)[bad[0]], MAX_AREA))


def _check_index(who, gt_index, lo, G):
    bad = np.nonzero((gt_index < lo) | (gt_index >= G))[0]
    if bad.size:
        raise ValueError("%s: gt_index[%d] = %d not in [%d, %d)" % (who, bad[0], gt_index[bad[0]], lo, G))


def _target_args(who, gt, ex_boxes, gt_index, S, thresh):
    S, thresh = _defaults(S, thresh)
    ex_boxes = np.ascontiguousarray(np.asarray(ex_boxes).reshape(-1, 4))
    if ex_boxes.size and not np.issubdtype(ex_boxes.dtype, np.integer):
        raise ValueError("%s: ex_boxes is not an integer array (dtype %s); round the boxes first" % (who, ex_boxes.dtype))
    gt_index = np.asarray(gt_index).reshape(-1)
    K = ex_boxes.shape[0]
    if gt_index.shape[0] != K:
        raise ValueError("%s: %d boxes and %d ground-truth indices" % (who, K, gt_index.shape[0]))
    _check_rows(who, K, S)
    if thresh != thresh:
        raise ValueError("%s: thresh is NaN" % who)
    _check_int_boxes(who, ex_boxes)
    _check_index(who, gt_index.astype(np.int64), 0, len(gt))
    return ex_boxes.astype(np.int32), np.ascontiguousarray(gt_index, np.int32), K, S, thresh


def _pred_args(who, gt, boxes, preds, gt_index):
    boxes = np.asarray(boxes, np.float64)
    boxes = np.ascontiguousarray(boxes.reshape(-1, boxes.shape[-1] if boxes.ndim > 1 else 4)[:, :4])
    K = boxes.shape[0]
    preds = np.asarray(preds, np.float32)
    from mnc_config import cfg
    S = int(preds.shape[-1]) if preds.ndim >= 3 and K else int(cfg.MASK_SIZE)
    gt_index = np.asarray(gt_index).reshape(-1)
    if gt_index.shape[0] != K or preds.size != K * S * S:
        raise ValueError("%s: %d boxes, %d ground-truth indices and predictions of shape %s" % (who, K, gt_index.shape[0], preds.shape))
    _check_rows(who, K, S)
    return boxes, np.ascontiguousarray(preds.reshape(K, S, S)), np.ascontiguousarray(gt_index, np.int32), K, S


def _iou(inter, area_pred, gt, gt_index):
    """The reference's mask_overlap from the counts: 0.0 where the union is below 1."""
    live = gt_index >= 0
    union = area_pred.copy()
    union[live] += gt.areas[gt_index[live]] - inter[live]
    iou = np.zeros(len(inter), np.float64)
    some = live & (union >= 1)
    iou[some] = inter[some] / union[some].astype(np.float64)
    return iou


# ---- the statements ----

def mask_targets_numpy(gt, ex_boxes, gt_index, S=None, thresh=None):
    """The mask regression targets as a plain loop on the host -- the specification csrc/mask_targets.hip is tested against.
    -> uint8 [K, S, S] of 0 / 1."""
    from utils.blob import resize_to
    ex_boxes, gt_index, K, S, thresh = _target_args("mask_targets_numpy", gt, ex_boxes, gt_index, S, thresh)
    thr = np.float32(thresh)
    out = np.zeros((K, S, S), np.uint8)
    for k in range(K):
        e = [int(v) for v in ex_boxes[k]]
        g = [int(v) for v in gt.bounds[gt_index[k]]]
        x1, y1, x2, y2 = max(e[0], g[0]), max(e[1], g[1]), min(e[2], g[2]), min(e[3], g[3])
        if x1 > x2 or y1 > y2:
            continue
        canvas = np.zeros((e[3] - e[1] + 1, e[2] - e[0] + 1), np.float32)
        canvas[y1 - e[1]:y2 - e[1] + 1, x1 - e[0]:x2 - e[0] + 1] = gt.dense(gt_index[k])[y1 - g[1]:y2 - g[1] + 1, x1 - g[0]:x2 - g[0] + 1]
        out[k] = resize_to(canvas, S, S) >= thr
    return out


def mask_pred_overlaps_numpy(gt, boxes, preds, gt_index, thresh=None):
    """What MaskLayer.forward_train counts, as the composition of the two existing statements: instance_masks_numpy(clip=False)
    of every row, mask_overlaps_numpy of row k against instance gt_index[k].  -> (inter, area_pred, iou)."""
    from .masks import instance_masks_numpy, mask_overlaps_numpy
    boxes, preds, gt_index, K, S = _pred_args("mask_pred_overlaps_numpy", gt, boxes, preds, gt_index)
    _check_index("mask_pred_overlaps_numpy", gt_index.astype(np.int64), -1, len(gt))
    inter, area_pred = np.zeros(K, np.int64), np.zeros(K, np.int64)
    if K:
        pm = instance_masks_numpy(boxes, preds, 0, 0, clip=False, binarize_thresh=_defaults(S, thresh)[1])
        for k in np.nonzero(gt_index >= 0)[0]:
            area_pred[k] = pm.areas[k]
            inter[k] = mask_overlaps_numpy(pm.take([k]), gt.take([gt_index[k]]))[0][0, 0]
    return inter, area_pred, _iou(inter, area_pred, gt, gt_index)


# ---- the device ----

def _call(name, *args):
    try:
        _lib.call(name, *args)
    except _lib.MncError as e:
        if e.code == 1:
            raise ValueError(str(e))
        raise


def mask_targets(gt, ex_boxes, gt_index, S=None, thresh=None, device_id=None):
    """mask_targets_numpy on the GPU (mnc_mask_targets): the same bytes.  The ground-truth words, K boxes and K indices go up,
    K * S * S bytes come back.  ValueError for what the statement refuses."""
    gt = gt.fetch()
    ex_boxes, gt_index, K, S, thresh = _target_args("mask_targets", gt, ex_boxes, gt_index, S, thresh)
    out = np.zeros((K, S, S), np.uint8)
    _call("mnc_mask_targets", *(_set_args(gt) + (_lib.ptr(ex_boxes), _lib.ptr(gt_index), K, S, thresh, _lib.ptr(out),
                                                 _device_id(device_id))))
    return out


def mask_pred_overlaps(gt, boxes, preds, gt_index, thresh=None, device_id=None):
    """mask_pred_overlaps_numpy on the GPU (mnc_mask_pred_overlaps): the same three arrays.  The predictions and the ground-truth
    words go up, two counts per row come back; no mask bit crosses the bus.  ValueError for what the statement refuses."""
    gt = gt.fetch()
    boxes, preds, gt_index, K, S = _pred_args("mask_pred_overlaps", gt, boxes, preds, gt_index)
    _check_index("mask_pred_overlaps", gt_index.astype(np.int64), -1, len(gt))
    inter, area_pred = np.zeros(K, np.int64), np.zeros(K, np.int64)
    _call("mnc_mask_pred_overlaps", *(_set_args(gt) + (_lib.ptr(boxes), _lib.ptr(preds), _lib.ptr(gt_index), K, S,
                                                       _defaults(S, thresh)[1], _lib.ptr(inter), _lib.ptr(area_pred),
                                                       _device_id(device_id))))
    return inter, area_pred, _iou(inter, area_pred, gt, gt_index)


# ---- ground truth and the two samplers ----

def pack_gt_masks(gt_boxes, gt_masks, mask_info, im_scale):
    """The reference's ground-truth blobs -> the set the entries read: gt_boxes [G, 4 or 5] (scaled by im_scale, in their own
    dtype: the division below is the layers'), gt_masks [G, Hmax, Wmax] of 0 / 1, mask_info [G, 2] = (h, w) of every mask.
    Bounds are np.around(gt_boxes[:, :4] / float(im_scale)); instance i is gt_masks[i, :h, :w].  ValueError naming the instance
    when mask_info disagrees with the rounded box's size (the reference would fail in a broadcast there) or a mask holds a value
    other than 0 and 1."""
    gt_boxes, gt_masks, mask_info = np.asarray(gt_boxes), np.asarray(gt_masks), np.asarray(mask_info)
    bounds = np.around(gt_boxes[:, :4] / float(im_scale)).astype(int)
    dense = []
    for i, (b, m) in enumerate(zip(bounds, gt_masks)):
        h, w = int(mask_info[i][0]), int(mask_info[i][1])
        if (h, w) != (b[3] - b[1] + 1, b[2] - b[0] + 1):
            raise ValueError("pack_gt_masks: instance %d: mask_info says %d x %d, its rounded box %s is %d x %d"
                             % (i, h, w, b, b[3] - b[1] + 1, b[2] - b[0] + 1))
        m = m[:h, :w]
        if m.shape != (h, w) or not ((m == 0) | (m == 1)).all():
            raise ValueError("pack_gt_masks: instance %d: the mask is smaller than mask_info's %d x %d or holds a value other than "
                             "0 and 1" % (i, h, w))
        dense.append(m != 0)
    return PackedMasks.from_dense(bounds, dense, classes=gt_boxes[:, 4] if gt_boxes.shape[1] > 4 else None)


def _assign(all_rois, gt_boxes):
    from utils.cython_bbox import bbox_overlaps
    overlaps = bbox_overlaps(np.ascontiguousarray(all_rois[:, 1:5], dtype=np.float64),
                             np.ascontiguousarray(gt_boxes[:, :4], dtype=np.float64))
    assignment = overlaps.argmax(axis=1)
    return assignment, overlaps.max(axis=1), gt_boxes[assignment, 4]


def _draw(max_overlaps, total, fractions, lows, highs):
    """One band after the other: npr.choice(candidates, size=min(count, np.round(total * fraction)), replace=False), drawn
    whenever the band has a candidate (a draw of size 0 still advances the generator), the union kept sorted -- the reference's
    calls in the reference's order, so one seed gives its sample."""
    picked = []
    for fraction, lo, hi in zip(fractions, lows, highs):
        band = np.where((max_overlaps >= lo) & (max_overlaps <= hi))[0]
        if band.size > 0:
            band = npr.choice(band, size=int(min(band.size, np.round(total * fraction))), replace=False)
        picked = np.unique(np.hstack((picked, band)))
    return picked


def _box_targets(rois, gt_boxes, assignment, keep_inds, labels, num_classes):
    from transform.bbox_transform import bbox_compute_targets, get_bbox_regression_label
    data = bbox_compute_targets(rois[:, 1:5], gt_boxes[assignment[keep_inds], :4], normalize=True)
    data = np.hstack((labels[:, np.newaxis], data)).astype(np.float32, copy=False)
    return get_bbox_regression_label(data, num_classes)


def _mask_part(rois, fg_inds, n_rows, assignment, labels, gt, im_scale, device_id):
    """pos_masks [n, 1, S, S] and the 12 columns of gt_masks_info: (gt index, h, w, label, ex_box, gt_box), -1 in background rows."""
    from mnc_config import cfg
    S = int(cfg.MASK_SIZE)
    n_fg = len(fg_inds)
    scaled = rois[:, 1:5] / float(im_scale)
    ex_boxes = np.around(scaled[:n_fg]).astype(int).reshape(n_fg, 4)
    index = assignment[np.asarray(fg_inds, int)]
    pos_masks = np.zeros((n_rows, 1, S, S))
    info = np.zeros((n_rows, 12))
    info[n_fg:, :] = -1
    if n_fg:
        pos_masks[:n_fg, 0] = mask_targets(gt, ex_boxes, index, S, cfg.BINARIZE_THRESH, device_id)
        info[:n_fg, 0] = index
        info[:n_fg, 1:3] = [gt.size(j) for j in index]
        info[:n_fg, 3] = labels[:n_fg]
        info[:n_fg, 4:8] = ex_boxes
        info[:n_fg, 8:12] = gt.bounds[index]
    return pos_masks, info


def sample_rois(all_rois, gt_boxes, rois_per_image, num_classes, gt, im_scale, device_id=None):
    """ProposalTargetLayer's sample (lib/pylayer/proposal_target_layer.py:118-216): all_rois [N, 5] and gt_boxes [G, 5] as the
    layer holds them, gt the PackedMasks of pack_gt_masks (None without cfg.MNC_MODE) -> (blobs, fg_inds, bg_inds, keep_inds)."""
    from mnc_config import cfg
    T = cfg.TRAIN
    assignment, max_overlaps, labels = _assign(all_rois, gt_boxes)
    fg_inds = _draw(max_overlaps, rois_per_image, T.FG_FRACTION, T.FG_THRESH_LO, T.FG_THRESH_HI)
    n_fg = fg_inds.size
    bg_inds = _draw(max_overlaps, rois_per_image - n_fg, T.BG_FRACTION, T.BG_THRESH_LO, T.BG_THRESH_HI)
    keep_inds = np.append(fg_inds, bg_inds).astype(int)
    labels = labels[keep_inds]
    labels[n_fg:] = 0
    rois = all_rois[keep_inds]
    bbox_targets, inside = _box_targets(rois, gt_boxes, assignment, keep_inds, labels, num_classes)
    blobs = {"rois": rois, "labels": labels, "bbox_targets": bbox_targets, "bbox_inside_weights": inside,
             "bbox_outside_weights": np.array(inside > 0).astype(np.float32)}
    if cfg.MNC_MODE:
        pos_masks, info = _mask_part(rois, fg_inds, len(keep_inds), assignment, labels, gt, im_scale, device_id)
        weight = np.zeros((rois.shape[0], 1, cfg.MASK_SIZE, cfg.MASK_SIZE))
        weight[:n_fg] = 1
        blobs.update(mask_targets=pos_masks, mask_weight=weight, gt_masks_info=info)
    return blobs, fg_inds, bg_inds, keep_inds


def stage_bridge_targets(all_rois, gt_boxes, im_scale, gt, num_classes, device_id=None):
    """StageBridgeLayer's sample (lib/pylayer/stage_bridge_layer.py:187-235): every RoI is kept, those with box IoU >=
    cfg.TRAIN.BBOX_THRESH first -> (labels, rois, fg_inds, keep_inds, mask_targets, gt_mask_info, bbox_targets,
    bbox_inside_weights)."""
    from mnc_config import cfg
    assignment, max_overlaps, labels = _assign(all_rois, gt_boxes)
    fg_inds = np.where(max_overlaps >= cfg.TRAIN.BBOX_THRESH)[0]
    bg_inds = np.where(max_overlaps < cfg.TRAIN.BBOX_THRESH)[0]
    keep_inds = np.append(fg_inds, bg_inds).astype(int)
    labels = labels[keep_inds]
    labels[len(fg_inds):] = 0
    rois = all_rois[keep_inds]
    bbox_targets, inside = _box_targets(rois, gt_boxes, assignment, keep_inds, labels, num_classes)
    pos_masks, info = _mask_part(rois, fg_inds, len(keep_inds), assignment, labels, gt, im_scale, device_id)
    return labels, rois, fg_inds, keep_inds, pos_masks, info, bbox_targets, inside


def timing(on):
    """mnc_mask_targets_timing: switch the event pair on or off -> the kernel's milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_targets_timing", on)
