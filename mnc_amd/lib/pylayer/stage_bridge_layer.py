"""`pylayer.stage_bridge_layer.StageBridgeLayer` -- refine each RoI with a box regressor of its own and clip; forward only.

TEST   the regressor of the arg-max segmentation class, background column included (reference:
       lib/pylayer/stage_bridge_layer.py:25-31, 52-55, 237-255).
       bottom: rois [R,5], bbox_pred [R,4K], seg_cls_prob [R,K], im_info [1,3]      top: rois_ext [R,5] float32
TRAIN  the regressor of the arg-max foreground class; the refined RoIs and the ground-truth boxes are then labelled by box IoU
       (>= cfg.TRAIN.BBOX_THRESH first, every row is kept) and get box and mask regression targets as in ProposalTargetLayer
       (:131-235) -- mnc_amd.targets.stage_bridge_targets, the mask targets of all foreground rows from one device call.
       bottom: rois [R,5], bbox_pred [R,4K], seg_cls_prob [R,K], gt_boxes [G,5], gt_masks [G,Hmax,Wmax], im_info [1,3], mask_info [G,2]
       top: rois [N,5], labels [N], mask_targets / mask_weight [N,1,S,S], gt_mask_info [N,12], bbox_targets /
            bbox_inside_weights / bbox_outside_weights [N,4K];  N = R + G
       param_str: use_clip, clip_base (64), feat_stride, num_classes.  Sets _keep_inds, _clip_keep and _bbox_reg_labels."""
import numpy as np
import yaml

import caffe
from mnc_config import cfg
from transform.bbox_transform import bbox_transform_inv, clip_boxes

TRAIN_TOPS = ("rois", "labels", "mask_targets", "mask_weight", "gt_mask_info", "bbox_targets", "bbox_inside_weights",
              "bbox_outside_weights")


class StageBridgeLayer(caffe.Layer):
    def setup(self, bottom, top):
        params = yaml.safe_load(self.param_str_ or "") or {}      # the TEST phase takes no parameters (empty param_str)
        phase = str(self.phase)
        if phase not in ("TEST", "TRAIN"):
            raise NotImplementedError("StageBridgeLayer: unrecognized phase %r" % phase)
        top[0].reshape(1, 5)
        if phase == "TRAIN":
            self._use_clip = params["use_clip"]
            self._clip_denominator = float(params.get("clip_base", 64))
            self._clip_thresh = 1.0 / self._clip_denominator
            self._feat_stride = params["feat_stride"]
            self._num_classes = params["num_classes"]
            K, S = self._num_classes, cfg.MASK_SIZE
            for t, shape in zip(top[1:], [(1, 1), (1, 1, S, S), (1, 1, S, S), (1, 4), (1, 4 * K), (1, 4 * K), (1, 4 * K)]):
                t.reshape(*shape)

    def reshape(self, bottom, top):
        pass

    def forward(self, bottom, top):
        if str(self.phase) == "TRAIN":
            for t, blob in zip(top, self._forward_train(bottom)):
                t.reshape(*blob.shape)
                t.data[...] = blob.astype(np.float32, copy=False)
            return
        rois = bottom[0].data
        decoded = bbox_transform_inv(rois[:, 1:5], bottom[1].data)          # [R, 4K]
        best = bottom[2].data.argmax(axis=1)
        cols = 4 * best[:, None] + np.arange(4)[None, :]
        picked = np.take_along_axis(decoded, cols, axis=1)
        out = np.zeros((rois.shape[0], 5), dtype=np.float64)                # float64 staging, stored as float32
        out[:, 1:5], _ = clip_boxes(picked.astype(np.float64), bottom[3].data[0, :2])
        top[0].reshape(*out.shape)
        top[0].data[...] = out.astype(np.float32, copy=False)

    def _forward_train(self, bottom):
        """-> the eight tops in TRAIN_TOPS' order."""
        from mnc_amd.targets import pack_gt_masks, stage_bridge_targets
        rois, deltas, gt_boxes = bottom[0].data, bottom[1].data, bottom[3].data
        im_info = bottom[5].data[0, :]
        self._bbox_reg_labels = bottom[2].data[:, 1:].argmax(axis=1) + 1
        # the four deltas of every row's class, decoded in float64
        cols = 4 * self._bbox_reg_labels[:, None] + np.arange(4)[None, :]
        picked = np.take_along_axis(deltas, cols, axis=1).astype(np.float64)
        all_rois = np.zeros((rois.shape[0], 5))
        all_rois[:, 1:5] = bbox_transform_inv(rois[:, 1:5], picked)
        all_rois = np.vstack((all_rois, np.hstack((np.zeros((gt_boxes.shape[0], 1), dtype=gt_boxes.dtype), gt_boxes[:, :-1]))))
        all_rois[:, 1:5], self._clip_keep = clip_boxes(all_rois[:, 1:5], im_info[:2])
        gt = pack_gt_masks(gt_boxes, bottom[4].data, bottom[6].data, im_info[2])
        labels, rois_out, fg_inds, keep_inds, mask_targets, info, bbox_targets, inside = stage_bridge_targets(
            all_rois, gt_boxes, im_info[2], gt, self._num_classes, cfg.GPU_ID)
        self._keep_inds = keep_inds
        weight = np.zeros((rois_out.shape[0], 1, cfg.MASK_SIZE, cfg.MASK_SIZE))
        weight[0:len(fg_inds)] = 1
        return (rois_out, labels, mask_targets, weight, info, bbox_targets, inside, np.array(inside > 0).astype(np.float32))

    def backward(self, top, propagate_down, bottom):
        raise NotImplementedError("StageBridgeLayer.backward is not implemented: the layers of this package run forward only")
