"""`pylayer.mask_layer.MaskLayer` -- sigmoid mask vector [R, S*S] -> mask_proposal [R,1,S,S] (reference:
lib/pylayer/mask_layer.py:22-29, 95-102), and in the TRAIN phase the label of every mask for the segmentation classifier (:56-93):
the prediction resized to its box, binarised and compared with its ground-truth mask -- on the GPU, all rows in one call
(mnc_amd.targets.mask_pred_overlaps, csrc/mask_targets.hip).  Forward only.

TEST   bottom: mask_pred [R, S*S]                                            top: mask_proposal [R,1,S,S]
TRAIN  bottom: mask_pred [R, S*S], gt_masks [G,Hmax,Wmax], gt_masks_info [R,12] (ProposalTargetLayer's: gt index or -1, h, w,
               label, ex_box, gt_box)                                        top: mask_proposal, mask_proposal_label [R,1]
The label is 0 where the row is background (gt index -1) or the mask IoU is below cfg.TRAIN.FG_SEG_THRESH, else the row's class."""
import numpy as np

import caffe
from mnc_config import cfg


def _gt_of_info(gt_masks, info):
    """The ground-truth set behind gt_masks_info: instance j has the rounded gt_box and the (h, w) of the rows that name it; an
    instance no row names has no rows."""
    from mnc_amd.masks import PackedMasks
    G = gt_masks.shape[0]
    bounds, dense = np.tile(np.array([0, 0, -1, -1]), (G, 1)), [None] * G
    index = info[:, 0].astype(int)
    for j in np.unique(index[index >= 0]):
        row = info[np.nonzero(index == j)[0][0]]
        bounds[j] = np.round(row[8:12]).astype(int)
        dense[j] = gt_masks[j][0:int(row[1]), 0:int(row[2])] != 0
    return PackedMasks.from_dense(bounds, dense), index


class MaskLayer(caffe.Layer):
    def setup(self, bottom, top):
        phase = str(self.phase)
        if phase not in ("TEST", "TRAIN"):
            raise NotImplementedError("MaskLayer: unrecognized phase %r" % phase)
        top[0].reshape(1, 1, cfg.MASK_SIZE, cfg.MASK_SIZE)
        if phase == "TRAIN":
            top[1].reshape(1, 1)

    def reshape(self, bottom, top):
        pass

    def forward(self, bottom, top):
        pred = bottom[0].data
        out = pred.reshape((pred.shape[0], 1, cfg.MASK_SIZE, cfg.MASK_SIZE))
        top[0].reshape(*out.shape)
        top[0].data[...] = out.astype(np.float32, copy=False)
        if str(self.phase) == "TRAIN":
            label = self._labels(pred, bottom[1].data, bottom[2].data)
            top[1].reshape(*label.shape)
            top[1].data[...] = label.astype(np.float32, copy=False)

    def _labels(self, pred, gt_masks, info):
        from mnc_amd.targets import mask_pred_overlaps
        S = cfg.MASK_SIZE
        gt, index = _gt_of_info(gt_masks, info)
        iou = mask_pred_overlaps(gt, info[:, 4:8], pred.reshape((pred.shape[0], S, S)), index, cfg.BINARIZE_THRESH, cfg.GPU_ID)[2]
        label = np.zeros((info.shape[0], 1))
        live = (index >= 0) & ~(iou < cfg.TRAIN.FG_SEG_THRESH)
        label[live, 0] = info[live, 3]
        self.pos_sample = np.where(label > 0)[0]
        return label

    def backward(self, top, propagate_down, bottom):
        raise NotImplementedError("MaskLayer.backward is not implemented: the layers of this package run forward only")
