"""`pylayer.proposal_target_layer.ProposalTargetLayer` -- forward only: RoIs + ground truth -> a sampled batch with class labels,
box regression targets and, with cfg.MNC_MODE, mask regression targets (reference: lib/pylayer/proposal_target_layer.py:27-107,
118-216).  The sample, the box targets and the index bookkeeping run on the host in numpy, with the reference's npr.choice calls in
the reference's order (one seed gives its sample); the mask targets of all foreground rows come from one device call
(mnc_amd.targets.sample_rois, csrc/mask_targets.hip).

bottom: rois [R,5], gt_boxes [G,5], im_info [1,3], gt_masks [G,Hmax,Wmax], mask_info [G,2], with cfg.TRAIN.MIX_INDEX proposal_index [1,R]
top:    rois [N,5], labels [N], bbox_targets / bbox_inside_weights / bbox_outside_weights [N,4K], with cfg.MNC_MODE mask_targets /
        mask_weight [N,1,S,S] and gt_masks_info [N,12], with cfg.TRAIN.MIX_INDEX fg_inds and bg_inds (anchor indices)"""
import numpy as np
import yaml

import caffe
from mnc_config import cfg
from transform.anchors import generate_anchors

TOPS = ("rois", "labels", "bbox_targets", "bbox_inside_weights", "bbox_outside_weights", "mask_targets", "mask_weight",
        "gt_masks_info", "fg_inds", "bg_inds")


class ProposalTargetLayer(caffe.Layer):
    def setup(self, bottom, top):
        params = yaml.safe_load(self.param_str_) or {}
        self._anchors = generate_anchors()
        self._num_anchors = self._anchors.shape[0]
        self._num_classes = params["num_classes"]
        self._bp_all = params.get("bp_all", True)
        K, S = self._num_classes, cfg.MASK_SIZE
        shapes = [(1, 5), (1, 1), (1, 4 * K), (1, 4 * K), (1, 4 * K)]
        if cfg.MNC_MODE:
            shapes += [(1, 1, S, S), (1, 1, S, S), (1, 4)]
            if cfg.TRAIN.MIX_INDEX:
                shapes += [(1, 4), (1, 4)]
        self._top_name_map = {name: i for i, name in enumerate(TOPS[:len(shapes)])}
        for t, shape in zip(top, shapes):
            t.reshape(*shape)

    def reshape(self, bottom, top):
        pass  # shapes are data dependent; the tops are reshaped in forward

    def forward(self, bottom, top):
        from mnc_amd.targets import pack_gt_masks, sample_rois
        gt_boxes = bottom[1].data
        im_scale = bottom[2].data[0, :][2]
        gt = pack_gt_masks(gt_boxes, bottom[3].data, bottom[4].data, im_scale) if cfg.MNC_MODE else None
        # the ground-truth boxes are candidates too
        all_rois = np.vstack((bottom[0].data, np.hstack((np.zeros((gt_boxes.shape[0], 1), dtype=gt_boxes.dtype), gt_boxes[:, :-1]))))
        assert np.all(all_rois[:, 0] == 0), "Only single item batches are supported"
        blobs, fg_inds, bg_inds, keep_inds = sample_rois(all_rois, gt_boxes, cfg.TRAIN.BATCH_SIZE, self._num_classes, gt, im_scale,
                                                         cfg.GPU_ID)
        self._keep_ind = keep_inds if self._bp_all else fg_inds
        if cfg.TRAIN.MIX_INDEX:
            # RoI rows -> the anchors they came from; the appended ground-truth rows have none
            index = bottom[5].data
            fg_inds = fg_inds[fg_inds < index.shape[1]].astype(int)
            blobs["fg_inds"] = index[0, fg_inds]
            blobs["bg_inds"] = index[0, bg_inds.astype(int)]
        for name, blob in blobs.items():
            t = top[self._top_name_map[name]]
            t.reshape(*blob.shape)
            t.data[...] = blob.astype(np.float32, copy=False)

    def backward(self, top, propagate_down, bottom):
        raise NotImplementedError("ProposalTargetLayer.backward is not implemented: the layers of this package run forward only")
