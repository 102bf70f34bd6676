#!/usr/bin/env python3
"""Time the training-target entries (mnc_amd/targets.py; csrc/mask_targets.hip) against their numpy statements on this machine's
CPU, in this process and run: mask_targets for 64 and 300 foreground rows against 10 ground-truth instances of a 600x1000 image;
mask_pred_overlaps for 300 rows with VOC-sized boxes, also against the existing device entries composed (instance_masks(clip=False),
then mask_overlaps, picked at [k, gt_index[k]]); and the forwards of ProposalTargetLayer + MaskLayer + StageBridgeLayer end to end
(300 RoIs, cfg.TRAIN.BATCH_SIZE 64), once with the device entries and once with the statements in their place.  Medians over --iters
device rounds and --host-iters host rounds after one warm-up each.  kernels_us is the device time of the launch alone between a HIP
event pair (mnc_mask_targets_timing); copies_share is the rest of the call -- the upload of the ground-truth words, rows and
predictions, the read-back, and the host's checks -- as a share of it.  The results are compared; nothing about speed is asserted.
Prints one JSON line and writes it, under a heading, to --profile (default profiles/train_targets_bench.txt; "" writes nothing).

    python tools/train_targets_bench.py [--iters 20] [--host-iters 3] [--profile FILE]
"""
import os

import numpy as np

from _task_harness import emit, kernels_us, median_ms, parser

HEADING = """tools/train_targets_bench.py --iters %d --host-iters %d on one MI355X.  targets_K: PackedMasks.targets (mnc_mask_targets) for K
foreground rows against 10 ground-truth instances of a 600x1000 image; pred_overlaps: PackedMasks.pred_overlaps
(mnc_mask_pred_overlaps) for 300 rows with VOC-sized boxes, `composed` the existing entries instance_masks(clip=False) +
mask_overlaps on the same rows; layers: ProposalTargetLayer + MaskLayer + StageBridgeLayer forwards on 300 RoIs.  host: the numpy
statements of mnc_amd/targets.py on this machine's CPU.  device: host arrays in and out, copies included.  kernels_us: the launch
alone between a HIP event pair; copies_share: the rest of the call over the call.  All sides measured in the same process and run.

"""
H, W = 600, 1000


def ground_truth(rng, n=10):
    """n instances of an H x W image: ellipses under noise in boxes of VOC sizes -> (gt_boxes float32 [n, 5], PackedMasks)."""
    from mnc_amd.masks import PackedMasks
    bounds, dense = [], []
    for _ in range(n):
        w, h = int(rng.integers(80, 500)), int(rng.integers(80, 400))
        x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        yy, xx = np.mgrid[0:h, 0:w]
        dense.append((((xx - w / 2.0) / (0.5 * w)) ** 2 + ((yy - h / 2.0) / (0.5 * h)) ** 2 < 1.0) ^ (rng.random((h, w)) < 0.05))
        bounds.append([x, y, x + w - 1, y + h - 1])
    bounds = np.array(bounds, np.int32)
    boxes = np.hstack((bounds, rng.integers(1, 21, (n, 1)))).astype(np.float32)
    return boxes, PackedMasks.from_dense(bounds, dense, classes=boxes[:, 4])


def jittered(rng, bounds, K, amp=0.15):
    j = rng.integers(0, len(bounds), K)
    b = bounds[j].astype(np.float64)
    size = np.stack([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]] * 2, 1)
    out = b + rng.uniform(-amp, amp, (K, 4)) * size
    out[:, 2:] = np.maximum(out[:, 2:], out[:, :2] + 8)
    return out, j.astype(np.int32)


def figures(name, host, device, args, timed=True):
    h, d = median_ms(host, args.host_iters), median_ms(device, args.iters)
    out = {name + "_host_ms_median": h[0], name + "_host_ms_min": h[1], name + "_device_ms_median": d[0], name + "_device_ms_min": d[1],
           name + "_host_over_device": round(h[0] / d[0], 1) if d[0] else None}
    if timed:
        us = kernels_us("mnc_mask_targets_timing", device, args.iters)
        out.update({name + "_kernels_us_median": us, name + "_copies_share": round(1.0 - us / 1e3 / d[0], 3) if us and d[0] else None})
    return out


def layer_blobs(rng, gt_boxes, gt):
    """The bottoms of the three layers at im_scale 1: 300 RoIs, the dense ground-truth blobs, predictions and deltas."""
    rois = np.zeros((300, 5), np.float32)
    rois[:, 1:] = np.clip(jittered(rng, gt.bounds, 300, 0.25)[0], 0, [W - 1, H - 1, W - 1, H - 1])
    sizes = np.array([gt.size(i) for i in range(len(gt))])
    gt_masks = np.zeros((len(gt), sizes[:, 0].max(), sizes[:, 1].max()), np.float32)
    for i, (h, w) in enumerate(sizes):
        gt_masks[i, :h, :w] = gt.dense(i)
    return {"rois": rois, "gt_boxes": gt_boxes, "im_info": np.array([[H, W, 1.0]], np.float32), "gt_masks": gt_masks,
            "mask_info": sizes.astype(np.float32), "index": np.arange(300, dtype=np.float32)[None, :]}


class Blob(object):
    def __init__(self, a=None):
        self.data = np.zeros((1,), np.float32) if a is None else np.ascontiguousarray(a, np.float32)

    def reshape(self, *d):
        if tuple(d) != self.data.shape:
            self.data = np.zeros(d, np.float32)


def run(cls, bottoms, ntop, param_str=""):
    layer = cls()
    layer.param_str_, layer.phase = param_str, "TRAIN"
    bottom, top = [Blob(b) for b in bottoms], [Blob() for _ in range(ntop)]
    layer.setup(bottom, top)
    layer.forward(bottom, top)
    return [t.data for t in top]


def three_layers(b, pred_rng):
    from pylayer.mask_layer import MaskLayer
    from pylayer.proposal_target_layer import ProposalTargetLayer
    from pylayer.stage_bridge_layer import StageBridgeLayer
    np.random.seed(3)
    pt = run(ProposalTargetLayer, [b["rois"], b["gt_boxes"], b["im_info"], b["gt_masks"], b["mask_info"], b["index"]], 10,
             "{'num_classes': 21}")
    rng = np.random.default_rng(pred_rng)
    n = len(pt[0])
    pred = (0.7 * pt[5].reshape(n, -1) + 0.3 * rng.random((n, 441))).astype(np.float32)
    mk = run(MaskLayer, [pred, b["gt_masks"], pt[7]], 2)
    sb = run(StageBridgeLayer, [pt[0], rng.normal(0, 0.05, (n, 84)).astype(np.float32), rng.random((n, 21)).astype(np.float32),
                                b["gt_boxes"], b["gt_masks"], b["im_info"], b["mask_info"]], 8,
             "{'use_clip': 1, 'feat_stride': 16, 'num_classes': 21}")
    return pt + mk + sb


def main():
    ap = parser()
    ap.add_argument("--profile", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "train_targets_bench.txt"))
    args = ap.parse_args()
    import mnc_amd
    mnc_amd.install_paths()
    from mnc_amd import targets as T
    from mnc_amd.masks import instance_masks, mask_overlaps
    rng = np.random.default_rng(5)
    gt_boxes, gt = ground_truth(rng)
    line = {"workload": "training targets: mask regression targets and mask-overlap labels on 10 packed ground-truth instances of a 600x1000 image",
            "host": "mask_targets_numpy / mask_pred_overlaps_numpy / the layers on them", "device": "mnc_mask_targets / mnc_mask_pred_overlaps, host arrays in and out",
            "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "gt_bits_bytes": int(gt.bits.nbytes)}
    for K in (64, 300):
        boxes, index = jittered(rng, gt.bounds, K)
        boxes = np.around(boxes).astype(np.int32)
        name = "targets_%d" % K
        line[name + "_equals_host"] = bool(np.array_equal(gt.targets(boxes, index), T.mask_targets_numpy(gt, boxes, index)))
        line.update(figures(name, lambda: T.mask_targets_numpy(gt, boxes, index), lambda: gt.targets(boxes, index), args))
    boxes, index = jittered(rng, gt.bounds, 300)
    index[::7] = -1
    preds = rng.random((300, 21, 21)).astype(np.float32)
    got, want = gt.pred_overlaps(boxes, preds, index), T.mask_pred_overlaps_numpy(gt, boxes, preds, index)
    line["pred_overlaps_equals_host"] = bool(all(np.array_equal(a, b) for a, b in zip(got, want)))
    line["pred_overlaps_box_pixels"] = int(sum((np.rint(b[2]) - np.rint(b[0]) + 1) * (np.rint(b[3]) - np.rint(b[1]) + 1) for b in boxes))
    line.update(figures("pred_overlaps", lambda: T.mask_pred_overlaps_numpy(gt, boxes, preds, index),
                        lambda: gt.pred_overlaps(boxes, preds, index), args))

    def composed():
        pm = instance_masks(boxes, preds, 0, 0, clip=False)
        return mask_overlaps(pm, gt)[0][np.arange(300), np.maximum(index, 0)], pm

    inter, pm = composed()
    line["pred_overlaps_equals_composed"] = bool(np.array_equal(np.where(index >= 0, inter, 0), got[0]))
    line["composed_mask_bytes_over_the_bus"] = int(2 * pm.bits.nbytes)
    c = median_ms(composed, args.iters)
    line.update({"composed_device_ms_median": c[0], "composed_device_ms_min": c[1],
                 "pred_overlaps_faster_than_composed": bool(line["pred_overlaps_device_ms_median"] < c[0])})
    blobs = layer_blobs(rng, gt_boxes, gt)
    device_tops = three_layers(blobs, 9)
    saved = T.mask_targets, T.mask_pred_overlaps
    on_host = lambda: (setattr(T, "mask_targets", lambda g, b, j, S=None, thresh=None, device_id=None: T.mask_targets_numpy(g, b, j, S, thresh)),      # noqa: E731
                       setattr(T, "mask_pred_overlaps", lambda g, b, p, j, thresh=None, device_id=None: T.mask_pred_overlaps_numpy(g, b, p, j, thresh)))
    on_device = lambda: (setattr(T, "mask_targets", saved[0]), setattr(T, "mask_pred_overlaps", saved[1]))      # noqa: E731

    def host_layers():
        on_host()
        try:
            return three_layers(blobs, 9)
        finally:
            on_device()

    line["layers_equal_host"] = bool(all(np.array_equal(a, b) for a, b in zip(device_tops, host_layers())))
    line["layers_rows"] = [int(len(device_tops[0])), int(len(device_tops[12]))]
    line.update(figures("layers", host_layers, lambda: three_layers(blobs, 9), args, timed=False))
    emit(line, HEADING % (max(args.iters, 1), max(args.host_iters, 1)), args.profile)


if __name__ == "__main__":
    main()
