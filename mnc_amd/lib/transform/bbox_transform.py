"""Box decoding / clipping used on the inference path (reference: lib/transform/bbox_transform.py:64-130), and the box encoding
of the training targets (:39-61, :133-203).  Arithmetic follows the reference operation by operation in the dtype of `deltas`
(float32 on the inference path) resp. of the boxes given (float32 in ProposalTargetLayer and AnchorTargetLayer's anchors in
float64, float64 in StageBridgeLayer), so the results are bit-identical to it."""
import numpy as np

from mnc_config import cfg


def bbox_transform(ex_rois, gt_rois):
    """The regression targets (dx, dy, dw, dh) [N, 4] that take ex_rois to gt_rois: centre offsets over the ex size, log of the
    size ratios, with +1 widths; in the dtype numpy gives the operands."""
    ew = ex_rois[:, 2] - ex_rois[:, 0] + 1.0
    eh = ex_rois[:, 3] - ex_rois[:, 1] + 1.0
    ecx = ex_rois[:, 0] + 0.5 * ew
    ecy = ex_rois[:, 1] + 0.5 * eh
    gw = gt_rois[:, 2] - gt_rois[:, 0] + 1.0
    gh = gt_rois[:, 3] - gt_rois[:, 1] + 1.0
    gcx = gt_rois[:, 0] + 0.5 * gw
    gcy = gt_rois[:, 1] + 0.5 * gh
    return np.vstack(((gcx - ecx) / ew, (gcy - ecy) / eh, np.log(gw / ew), np.log(gh / eh))).transpose()


def bbox_compute_targets(ex_rois, gt_rois, normalize):
    """bbox_transform as float32, with cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED and `normalize` standardised by the
    configured means and deviations first."""
    assert ex_rois.shape == gt_rois.shape
    targets = bbox_transform(ex_rois, gt_rois)
    if cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED and normalize:
        targets = (targets - np.array(cfg.TRAIN.BBOX_NORMALIZE_MEANS)) / np.array(cfg.TRAIN.BBOX_NORMALIZE_STDS)
    return targets.astype(np.float32, copy=False)


def scale_boxes(boxes, alpha):
    """Boxes with +1 width and height multiplied by alpha around their centres."""
    w = boxes[:, 2] - boxes[:, 0] + 1
    h = boxes[:, 3] - boxes[:, 1] + 1
    cx = boxes[:, 0] + 0.5 * w
    cy = boxes[:, 1] + 0.5 * h
    w, h = w * alpha, h * alpha
    out = np.zeros(boxes.shape, dtype=boxes.dtype)
    out[:, 0] = cx - 0.5 * w
    out[:, 1] = cy - 0.5 * h
    out[:, 2] = cx + 0.5 * w
    out[:, 3] = cy + 0.5 * h
    return out


def get_bbox_regression_label(bbox_target_data, num_class):
    """Compact targets [N, 5] = (class, tx, ty, tw, th) -> (bbox_targets, bbox_inside_weights), both float32 [N, 4 num_class]:
    the four targets resp. cfg.TRAIN.BBOX_INSIDE_WEIGHTS in the columns of the row's class, zeros in background rows."""
    assert bbox_target_data.shape[1] == 5
    classes = bbox_target_data[:, 0]
    targets = np.zeros((classes.size, 4 * num_class), dtype=np.float32)
    inside = np.zeros(targets.shape, dtype=np.float32)
    for row in np.where(classes > 0)[0]:
        lo = 4 * int(classes[row])
        targets[row, lo:lo + 4] = bbox_target_data[row, 1:]
        inside[row, lo:lo + 4] = cfg.TRAIN.BBOX_INSIDE_WEIGHTS
    return targets, inside


def bbox_transform_inv(boxes, deltas):
    """Apply (dx, dy, dw, dh) deltas; `deltas` may hold K classes per row as [N, 4K]."""
    if boxes.shape[0] == 0:
        return np.zeros((0, deltas.shape[1]), dtype=deltas.dtype)
    boxes = boxes.astype(deltas.dtype, copy=False)
    w = boxes[:, 2] - boxes[:, 0] + 1.0
    h = boxes[:, 3] - boxes[:, 1] + 1.0
    cx = boxes[:, 0] + 0.5 * w
    cy = boxes[:, 1] + 0.5 * h
    w, h, cx, cy = w[:, None], h[:, None], cx[:, None], cy[:, None]
    pcx = deltas[:, 0::4] * w + cx
    pcy = deltas[:, 1::4] * h + cy
    pw = np.exp(deltas[:, 2::4]) * w
    ph = np.exp(deltas[:, 3::4]) * h
    out = np.empty(deltas.shape, dtype=deltas.dtype)
    out[:, 0::4] = pcx - 0.5 * pw
    out[:, 1::4] = pcy - 0.5 * ph
    out[:, 2::4] = pcx + 0.5 * pw        # no "-1" on the far edge (bbox_transform.py:94-97)
    out[:, 3::4] = pcy + 0.5 * ph
    return out


def clip_boxes(boxes, im_shape):
    """Clamp x to [0, W-1], y to [0, H-1]; also returns the row indices that were already inside."""
    xmax, ymax = im_shape[1] - 1, im_shape[0] - 1
    x1, y1, x2, y2 = boxes[:, 0::4], boxes[:, 1::4], boxes[:, 2::4], boxes[:, 3::4]
    inside = np.where((x1 >= 0) & (x2 <= xmax) & (y1 >= 0) & (y2 <= ymax))[0]
    out = np.empty(boxes.shape, dtype=boxes.dtype)
    out[:, 0::4] = np.maximum(np.minimum(x1, xmax), 0)
    out[:, 1::4] = np.maximum(np.minimum(y1, ymax), 0)
    out[:, 2::4] = np.maximum(np.minimum(x2, xmax), 0)
    out[:, 3::4] = np.maximum(np.minimum(y2, ymax), 0)
    return out, inside


def filter_small_boxes(boxes, min_size):
    """Indices of boxes whose +1 width and height are both >= min_size."""
    return np.where(((boxes[:, 2] - boxes[:, 0] + 1) >= min_size) & ((boxes[:, 3] - boxes[:, 1] + 1) >= min_size))[0]
