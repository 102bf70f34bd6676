"""`pylayer.anchor_target_layer.AnchorTargetLayer` -- forward only: ground-truth boxes -> RPN labels and box regression targets for
every anchor of the feature map (reference: lib/pylayer/anchor_target_layer.py:25-233).  A host port: the anchor x ground-truth IoU
comes from mnc_bbox_overlaps, everything else is numpy with the reference's np.random.choice calls in the reference's order.

bottom: rpn_cls_score [1,2A,H,W] (its shape only), gt_boxes [G,5], im_info [1,3], with cfg.TRAIN.MIX_INDEX fg_inds and bg_inds of
        ProposalTargetLayer (anchor indices that are forced to 1 resp. 0)
top:    labels [1,1,A*H,W] (1 positive, 0 negative, -1 ignored), bbox_targets / bbox_inside_weights / bbox_outside_weights [1,4A,H,W]
Semantics kept from the reference: only anchors inside the image (+- allowed_border) take part; for each ground truth every anchor
that ties its best IoU is positive (overlaps == gt_max_overlaps), as are anchors at or above RPN_POSITIVE_OVERLAP; negatives are
set before the positives, or after them with RPN_CLOBBER_POSITIVES; surplus positives, then surplus negatives, are switched to -1
by a random draw; RPN_POSITIVE_WEIGHT < 0 weights every example 1 / #examples, else positives and negatives share p and 1 - p."""
import numpy as np
import yaml

import caffe
from mnc_config import cfg
from transform.anchors import generate_anchors
from transform.bbox_transform import bbox_transform
from utils.cython_bbox import bbox_overlaps
from utils.unmap import unmap


class AnchorTargetLayer(caffe.Layer):
    def setup(self, bottom, top):
        params = yaml.safe_load(self.param_str_) or {}
        self._anchors = generate_anchors()
        self._num_anchors = self._anchors.shape[0]
        self._feat_stride = params["feat_stride"]
        self._allowed_border = params.get("allowed_border", 0)
        height, width = bottom[0].data.shape[-2:]
        A = self._num_anchors
        top[0].reshape(1, 1, A * height, width)
        for t in top[1:4]:
            t.reshape(1, A * 4, height, width)

    def reshape(self, bottom, top):
        pass  # the tops are reshaped in forward

    def _inside_anchors(self, height, width, im_info):
        """-> (indices into the K * A grid anchors, rows ordered (h, w, a), of those inside the image; their boxes; K * A)."""
        sx, sy = np.meshgrid(np.arange(0, width) * self._feat_stride, np.arange(0, height) * self._feat_stride)
        shifts = np.vstack((sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel())).transpose()
        A, K = self._num_anchors, shifts.shape[0]
        grid = (self._anchors.reshape((1, A, 4)) + shifts.reshape((1, K, 4)).transpose((1, 0, 2))).reshape((K * A, 4))
        border = self._allowed_border
        inside = np.where((grid[:, 0] >= -border) & (grid[:, 1] >= -border) & (grid[:, 2] < im_info[1] + border) &
                          (grid[:, 3] < im_info[0] + border))[0]
        return inside, grid[inside, :], int(K * A)

    def forward(self, bottom, top):
        T = cfg.TRAIN
        assert bottom[0].data.shape[0] == 1, "Only single item batches are supported"
        height, width = bottom[0].data.shape[-2:]
        gt_boxes = bottom[1].data
        inside, anchors, total = self._inside_anchors(height, width, bottom[2].data[0, :])
        n = len(inside)

        overlaps = bbox_overlaps(np.ascontiguousarray(anchors, dtype=np.float64), np.ascontiguousarray(gt_boxes, dtype=np.float64))
        best_gt = overlaps.argmax(axis=1)
        best = overlaps[np.arange(n), best_gt]
        gt_best = overlaps[overlaps.argmax(axis=0), np.arange(overlaps.shape[1])]
        gt_winners = np.where(overlaps == gt_best)[0]           # every anchor that ties a ground truth's best, not one per column

        labels = np.full((n,), -1, dtype=np.float32)
        if not T.RPN_CLOBBER_POSITIVES:
            labels[best < T.RPN_NEGATIVE_OVERLAP] = 0
        labels[gt_winners] = 1
        labels[best >= T.RPN_POSITIVE_OVERLAP] = 1
        if T.RPN_CLOBBER_POSITIVES:
            labels[best < T.RPN_NEGATIVE_OVERLAP] = 0

        def thin(value, room):
            at = np.where(labels == value)[0]
            if len(at) > room:
                labels[np.random.choice(at, size=int(len(at) - room), replace=False)] = -1

        thin(1, int(T.RPN_FG_FRACTION * T.RPN_BATCHSIZE))
        thin(0, T.RPN_BATCHSIZE - np.sum(labels == 1))

        if T.MIX_INDEX:
            # the anchors behind the RoIs that ProposalTargetLayer sampled keep their side (positives win)
            def rows_of(indices):
                hits = [np.where(i == inside)[0] for i in list(indices)]
                return [h[0] for h in hits if len(h) > 0]
            forced_fg, forced_bg = rows_of(bottom[3].data), rows_of(bottom[4].data)
            labels[forced_bg] = 0
            labels[forced_fg] = 1

        targets = bbox_transform(anchors, gt_boxes[best_gt, :][:, :4]).astype(np.float32, copy=False)
        w_in = np.zeros((n, 4), dtype=np.float32)
        w_in[labels == 1, :] = np.array(T.RPN_BBOX_INSIDE_WEIGHTS)
        w_out = np.zeros((n, 4), dtype=np.float32)
        if T.RPN_POSITIVE_WEIGHT < 0:
            w_pos = w_neg = np.ones((1, 4)) * 1.0 / np.sum(labels >= 0)
        else:
            assert 0 < T.RPN_POSITIVE_WEIGHT < 1
            w_pos = T.RPN_POSITIVE_WEIGHT / np.sum(labels == 1)
            w_neg = (1.0 - T.RPN_POSITIVE_WEIGHT) / np.sum(labels == 0)
        w_out[labels == 1, :] = w_pos
        w_out[labels == 0, :] = w_neg

        # back to all K * A anchors (outside ones: label -1, weights 0), then to NCHW
        A = self._num_anchors
        labels = unmap(labels, total, inside, fill=-1).reshape((1, height, width, A)).transpose(0, 3, 1, 2)
        blobs = [labels.reshape((1, 1, A * height, width))]
        for data in (targets, w_in, w_out):
            blobs.append(unmap(data, total, inside, fill=0).reshape((1, height, width, A * 4)).transpose(0, 3, 1, 2))
        for t, blob in zip(top, blobs):
            t.reshape(*blob.shape)
            t.data[...] = blob

    def backward(self, top, propagate_down, bottom):
        raise NotImplementedError("AnchorTargetLayer.backward is not implemented: the layers of this package run forward only")
