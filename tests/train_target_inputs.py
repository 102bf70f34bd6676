"""Deterministic inputs of the training-target tests (tests/test_train_targets_host.py, tests/test_gpu_train_targets.py) and of
the fixture generator tests/golden/make_golden_train.py, which stores their sha256 digests: the tests regenerate the inputs and
check the digest before they compare anything with the fixture."""
import hashlib

import numpy as np

THRESH = 0.4            # cfg.BINARIZE_THRESH
LAYER_SEED = 7          # np.random.seed of every layer run
SAMPLE_SEEDS = (0, 1)   # np.random.seed of the direct _sample_rois / _sample_output runs
SCALES = (1.0, 1.6)
NUM_CLASSES = 21
FEAT = (10, 16)         # feature map of the layer cases: 1440 anchors, a 160 x 256 network input
ANCHOR_VARIANTS = {     # cfg.TRAIN keys of the AnchorTargetLayer runs
    "default": {},
    "clobber": {"RPN_CLOBBER_POSITIVES": True, "RPN_POSITIVE_WEIGHT": 0.25, "RPN_BATCHSIZE": 16},
}


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# ---- ground truth of the kernel cases -----------------------------------------------------------------------------------

def _checker(h, w):
    return (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(bool)


def gt_corpus():
    """-> (bounds int32 [G, 4], dense: list of bool [h, w] or None).  Instances 1-5 are 63, 64, 65, 128 and 129 wide; 6 is a
    42 x 42 checkerboard; 7 has no rows; 8 has rows and no pixel; 9 is 300 x 200 for the scaling cases; 10 is 1000 x 600."""
    rng = np.random.default_rng(23)
    spec = [(10, 20, 21, 21), (5, 3, 63, 9), (-3, -2, 64, 7), (100, 40, 65, 5), (0, 50, 128, 6), (7, 60, 129, 6)]
    bounds = [[x, y, x + w - 1, y + h - 1] for x, y, w, h in spec]
    dense = [rng.random((h, w)) < 0.55 for _, _, w, h in spec]
    bounds.append([50, 60, 91, 101])
    dense.append(_checker(42, 42))
    bounds.append([0, 0, -1, -1])
    dense.append(None)
    bounds.append([20, 5, 29, 14])
    dense.append(np.zeros((10, 10), bool))
    yy, xx = np.mgrid[0:200, 0:300]
    bounds.append([30, 10, 329, 209])
    dense.append((((xx - 150) / 140.0) ** 2 + ((yy - 100) / 90.0) ** 2 < 1.0) ^ (rng.random((200, 300)) < 0.1))
    yy, xx = np.mgrid[0:600, 0:1000]
    bounds.append([0, 0, 999, 599])
    dense.append(((xx // 37 + yy // 29) % 3 != 0) ^ (rng.random((600, 1000)) < 0.05))
    return np.array(bounds, np.int32), dense


def _grow(b, d):
    return [b[0] - d, b[1] - d, b[2] + d, b[3] + d]


def target_cases():
    """tag -> {"ex_boxes" int32 [K, 4], "gt_index" int32 [K], "S", "thresh"} on gt_corpus()."""
    B = [[int(v) for v in b] for b in gt_corpus()[0]]
    g0 = B[0]
    rows = {}
    rows["identity"] = [(g0, 0)]
    rows["touch"] = [([40, 20, 60, 40], 0),                         # disjoint
                     ([0, 0, 40, 20], 0), ([0, 40, 40, 60], 0),     # one row: the first, the last
                     ([0, 10, 10, 50], 0), ([30, 10, 50, 50], 0),   # one column
                     ([0, 0, 10, 20], 0), ([30, 40, 47, 55], 0)]    # one pixel
    rows["thin"] = [([15, 25, 15, 25], 0), ([12, 30, 28, 30], 0), ([20, 22, 20, 38], 0), ([3, 52, 120, 52], 4),
                    ([64, 45, 64, 60], 4)]
    words = []
    for j in (1, 2, 3, 4, 5):
        x, y1, _, y2 = B[j]
        for lo in (63, 64):
            for hi in (63, 64, 127, 128):
                if lo <= hi:
                    words.append(([x + lo, y1 - 1, x + hi, y2 + 1], j))
        words.append(([x - 2, y1, x + 70, y2], j))
    rows["words"] = words
    rows["overhang"] = [(_grow(B[3], 4), 3), ([20, 51, 90, 54], 4),
                        ([-10, -2, 20, 4], 2), ([40, -2, 70, 4], 2), ([-3, -9, 60, 0], 2), ([-3, 2, 60, 12], 2),
                        ([-40, -30, -1, 1], 2)]
    rows["scale"] = [([100, 80, 104, 86], 9), ([150, 60, 156, 64], 9), ([60, 40, 359, 239], 9), ([0, 0, 299, 199], 9)]
    rows["empty"] = [([0, 0, 20, 20], 7), ([18, 3, 31, 16], 8)]
    cases = {}
    for tag, r in rows.items():
        cases[tag] = {"ex_boxes": np.array([b for b, _ in r], np.int32).reshape(-1, 4), "gt_index": np.array([j for _, j in r], np.int32),
                      "S": 21, "thresh": THRESH}
    # every tap fraction is exactly 0.5 (inv = 2.0, src = 2 d + 0.5): the cells sit on the threshold and >= keeps them
    cases["checker"] = {"ex_boxes": np.array([B[6]], np.int32), "gt_index": np.array([6], np.int32), "S": 21, "thresh": 0.5}
    cases["none"] = {"ex_boxes": np.zeros((0, 4), np.int32), "gt_index": np.zeros(0, np.int32), "S": 21, "thresh": THRESH}
    rng = np.random.default_rng(29)
    x1, y1 = rng.integers(20, 300, 3000), rng.integers(0, 190, 3000)
    many = np.stack([x1, y1, x1 + rng.integers(0, 40, 3000), y1 + rng.integers(0, 40, 3000)], 1)
    cases["many"] = {"ex_boxes": many.astype(np.int32), "gt_index": np.full(3000, 9, np.int32), "S": 21, "thresh": THRESH}
    return cases


def target_case_digest(c):
    return digest(c["ex_boxes"], c["gt_index"], np.array([c["S"]]), np.array([c["thresh"]]))


def corpus_digest():
    bounds, dense = gt_corpus()
    return digest(bounds, *[np.zeros((0, 0), bool) if m is None else m for m in dense])


def label_cases():
    """tag -> {"boxes" float64 [K, 4], "preds" float32 [K, 21, 21], "gt_index" int32 [K], "thresh"} on gt_corpus()."""
    rng = np.random.default_rng(31)
    S = 21

    def smooth(k):
        p = rng.random((k, S, S)).astype(np.float32)
        return (0.25 * (p + np.roll(p, 1, 1) + np.roll(p, 1, 2) + np.roll(p, (1, 1), (1, 2)))).astype(np.float32)

    cases = {}
    boxes = [[10.5, 20.5, 30.5, 40.5], [11.5, 21.5, 31.5, 41.5], [9.5, 18.5, 28.5, 42.5],           # np.round is half to even
             [-8.2, -6.0, 30.0, 3.1], [40.0, -9.7, 90.3, 1.0], [-60.0, -40.0, -10.0, -5.0],          # partly, wholly outside
             [130.0, 38.0, 130.0, 46.0], [90.0, 38.0, 153.0, 46.0], [101.0, 41.0, 165.0, 43.0], [2.0, 58.0, 130.0, 66.0],
             [-1.0, -1.0, -1.0, -1.0], [60.0, 45.0, 70.0, 58.0]]
    index = [0, 0, 0, 2, 2, 2, 3, 3, 3, 5, -1, 4]
    cases["boxes"] = {"boxes": np.array(boxes), "preds": smooth(len(boxes)), "gt_index": np.array(index, np.int32)}
    cases["large"] = {"boxes": np.array([[0.0, 0.0, 999.0, 599.0]]), "preds": smooth(1), "gt_index": np.array([10], np.int32)}
    flat = np.stack([np.zeros((S, S), np.float32), np.ones((S, S), np.float32), np.full((S, S), np.float32(THRESH)),
                     np.zeros((S, S), np.float32)])
    cases["flat"] = {"boxes": np.array([[12.0, 18.0, 33.0, 44.0]] * 3 + [[18.0, 3.0, 31.0, 16.0]]), "preds": flat,
                     "gt_index": np.array([0, 0, 0, 8], np.int32)}                       # the last row: both masks empty
    for c in cases.values():
        c["thresh"] = THRESH
    return cases


def label_case_digest(c):
    return digest(c["boxes"], c["preds"], c["gt_index"], np.array([c["thresh"]]))


# ---- the layer cases ----------------------------------------------------------------------------------------------------

def layer_case(im_scale):
    """The bottoms that do not depend on another layer's tops: 40 RoIs and 3 ground-truth instances in a network input of
    160 x 256 (the unscaled image is that over im_scale), as float32 blobs."""
    rng = np.random.default_rng(41)
    H, W = FEAT[0] * 16, FEAT[1] * 16
    h0, w0 = int(H / im_scale), int(W / im_scale)
    raw = np.array([[10, 8, 70, 60], [60, 30, 140, 95], [5, 50, 50, 99]]) * min(h0 / 100.0, w0 / 160.0)
    raw = np.floor(raw).astype(int)
    gt_boxes = np.hstack((raw * np.float32(im_scale), np.array([[3], [12], [7]]))).astype(np.float32)
    back = np.around(gt_boxes[:, :4] / float(im_scale)).astype(int)
    sizes = np.stack([back[:, 3] - back[:, 1] + 1, back[:, 2] - back[:, 0] + 1], 1)
    gt_masks = np.zeros((3, sizes[:, 0].max(), sizes[:, 1].max()), np.float32)
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        inside = ((xx - w / 2.0) / (0.5 * w)) ** 2 + ((yy - h / 2.0) / (0.45 * h)) ** 2 < 1.0
        gt_masks[i, :h, :w] = inside ^ (rng.random((h, w)) < 0.08)
    rois = np.zeros((40, 5), np.float32)
    for k in range(40):
        if k < 28:
            b = gt_boxes[k % 3, :4]
            bw, bh = b[2] - b[0], b[3] - b[1]
            amp = 0.06 if k < 14 else 0.3
            rois[k, 1:] = b + rng.uniform(-amp, amp, 4) * np.array([bw, bh, bw, bh])
        else:
            x, y = rng.uniform(0, W - 40), rng.uniform(0, H - 40)
            rois[k, 1:] = [x, y, x + rng.uniform(16, 120), y + rng.uniform(16, 100)]
    rois[:, 1::2] = np.clip(rois[:, 1::2], 0, W - 1)
    rois[:, 2::2] = np.clip(rois[:, 2::2], 0, H - 1)
    return {"rois": rois, "gt_boxes": gt_boxes, "im_info": np.array([[H, W, im_scale]], np.float32), "gt_masks": gt_masks,
            "mask_info": sizes.astype(np.float32),
            "proposal_index": rng.permutation(FEAT[0] * FEAT[1] * 9)[:40].astype(np.float32)[None, :],
            "rpn_cls_score": np.zeros((1, 18, FEAT[0], FEAT[1]), np.float32)}


def layer_case_digest(c):
    return digest(*[c[k] for k in sorted(c)])


def mask_pred_for(mask_targets, gt_masks_info):
    """The MaskLayer's mask_pred [N, 441] from ProposalTargetLayer's tops: the target under noise for every other foreground row
    (a high overlap), noise alone elsewhere."""
    rng = np.random.default_rng(43)
    n = mask_targets.shape[0]
    noise = rng.random((n, 441)).astype(np.float32)
    near = (np.arange(n) % 2 == 0) & (gt_masks_info[:, 0] >= 0)
    pred = noise.copy()
    pred[near] = (0.7 * mask_targets.reshape(n, 441)[near] + 0.3 * noise[near]).astype(np.float32)
    return pred


def bridge_inputs(n):
    """bbox_pred [n, 84] and seg_cls_prob [n, 21] of the StageBridgeLayer's TRAIN phase."""
    rng = np.random.default_rng(47)
    return rng.normal(0, 0.08, (n, 4 * NUM_CLASSES)).astype(np.float32), rng.random((n, NUM_CLASSES)).astype(np.float32)


BRIDGE_PARAMS = "{'use_clip': 1, 'clip_base': 64, 'feat_stride': 16, 'num_classes': 21}"
TARGET_PARAMS = "{'num_classes': 21}"
ANCHOR_PARAMS = "{'feat_stride': 16, 'allowed_border': 160}"       # (without a border 6 of the 1440 anchors lie inside 160 x 256)
