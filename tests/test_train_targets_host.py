"""CPU: the training-target code against the reference's own outputs (tests/golden/reference_train_targets.npz, made by
tests/golden/make_golden_train.py) -- the numpy statements of mnc_amd.targets, the ported helpers, and the forward passes of the
four layers with the C ABI replaced by tests/fake_backend.py (mnc_bbox_overlaps) and the two device entries by their numpy
statements.  Every comparison is exact: array_equal plus dtype and shape.  The inputs are regenerated from
tests/train_target_inputs.py and checked against the digests the fixture stores."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import fake_backend  # noqa: E402
import mnc_amd  # noqa: E402
import train_target_inputs as TI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import targets as T  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

mnc_amd.install_paths()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(REPO, "tests", "golden", "reference_train_targets.npz"))


@pytest.fixture(scope="module")
def corpus(fixture):
    assert TI.corpus_digest() == str(fixture["corpus_digest"])
    return PackedMasks.from_dense(*TI.gt_corpus())


@pytest.fixture()
def numpy_entries(monkeypatch):
    """The library behind the layers: the box IoU from the test double, the two device entries from their statements."""
    import gc
    fake_backend.install(monkeypatch)
    monkeypatch.setattr(T, "mask_targets", lambda gt, b, j, S=None, thresh=None, device_id=None: T.mask_targets_numpy(gt, b, j, S, thresh))
    monkeypatch.setattr(T, "mask_pred_overlaps",
                        lambda gt, b, p, j, thresh=None, device_id=None: T.mask_pred_overlaps_numpy(gt, b, p, j, thresh))
    yield
    gc.collect()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def unpack(f, key):
    shape = tuple(int(v) for v in f[key + "_shape"])
    return np.unpackbits(f[key + "_bits"])[:int(np.prod(shape))].reshape(shape)


class Blob(object):
    def __init__(self, a=None):
        self.data = np.zeros((1,), np.float32) if a is None else np.ascontiguousarray(a, np.float32)

    def reshape(self, *d):
        if tuple(d) != self.data.shape:
            self.data = np.zeros(d, np.float32)


def run_layer(cls, bottoms, ntop, param_str="", phase="TRAIN"):
    layer = cls()
    layer.param_str_, layer.phase = param_str, phase
    bottom, top = [Blob(b) for b in bottoms], [Blob() for _ in range(ntop)]
    layer.setup(bottom, top)
    layer.reshape(bottom, top)
    layer.forward(bottom, top)
    return layer, [t.data.copy() for t in top]


def tops_of(f, prefix, n, packed=()):
    return [unpack(f, "%s_top%d" % (prefix, i)).astype(np.float32) if i in packed else f["%s_top%d" % (prefix, i)] for i in range(n)]


# ---- the statements ----

@pytest.mark.parametrize("tag", sorted(TI.target_cases()))
def test_mask_targets_statement_is_the_references_intersect_mask(fixture, corpus, tag):
    c = TI.target_cases()[tag]
    assert TI.target_case_digest(c) == str(fixture["tg_%s_digest" % tag])
    got = T.mask_targets_numpy(corpus, c["ex_boxes"], c["gt_index"], c["S"], c["thresh"])
    assert same(got, unpack(fixture, "tg_" + tag))


def test_intersect_mask_port_on_the_small_cases(fixture, corpus):
    from mnc_config import cfg
    from transform.mask_transform import intersect_mask
    for tag in ("identity", "touch", "thin", "words", "overhang", "empty"):
        c = TI.target_cases()[tag]
        want = unpack(fixture, "tg_" + tag).astype(bool)
        for k, (e, j) in enumerate(zip(c["ex_boxes"], c["gt_index"])):
            got = intersect_mask([int(v) for v in e], [int(v) for v in corpus.bounds[j]], corpus.dense(j))
            assert same(got, want[k]) and cfg.BINARIZE_THRESH == c["thresh"]


@pytest.mark.parametrize("tag", sorted(TI.label_cases()))
def test_pred_overlaps_statement_is_mask_layers_lines(fixture, corpus, tag):
    c = TI.label_cases()[tag]
    assert TI.label_case_digest(c) == str(fixture["lb_%s_digest" % tag])
    inter, area, iou = T.mask_pred_overlaps_numpy(corpus, c["boxes"], c["preds"], c["gt_index"], c["thresh"])
    assert same(iou, fixture["lb_%s_iou" % tag])
    assert inter.dtype == area.dtype == np.int64 and (inter <= area).all()
    dead = c["gt_index"] < 0
    assert not inter[dead].any() and not area[dead].any()
    if tag == "flat":                                      # all 0, all 1, all on the threshold (>= keeps them), both masks empty
        assert area.tolist() == [0, 22 * 27, 22 * 27, 0] and iou[0] == 0.0 and iou[3] == 0.0


def test_unmap_and_box_helpers():
    from transform.bbox_transform import bbox_compute_targets, bbox_transform, get_bbox_regression_label, scale_boxes
    from utils.unmap import unmap
    got = unmap(np.array([5.0, 6.0]), 4, np.array([3, 1]), fill=-1)
    assert same(got, np.array([-1, 6, -1, 5], np.float32))
    assert same(unmap(np.ones((2, 4)), 3, [0, 2], fill=0), np.array([[1] * 4, [0] * 4, [1] * 4], np.float32))
    ex = np.array([[0, 0, 9, 19], [10, 10, 29, 29]], np.float32)
    t = bbox_transform(ex, ex)
    assert t.dtype == np.float32 and not t.any()
    gt = np.array([[0, 0, 19, 19], [15, 10, 34, 29]], np.float32)
    t = bbox_compute_targets(ex, gt, normalize=True)
    assert same(t, np.array([[0.5, 0.0, np.log(np.float32(2.0)), 0.0], [0.25, 0.0, 0.0, 0.0]], np.float32))
    assert bbox_transform(ex.astype(np.float64), gt).dtype == np.float64
    tg, w = get_bbox_regression_label(np.hstack((np.array([[2.0], [0.0]], np.float32), t)), 3)
    assert same(tg[0, 8:12], t[0]) and tg[:, :8].sum() == 0 and not tg[1].any() and same(w[0], np.array([0] * 8 + [1] * 4, np.float32))
    assert same(scale_boxes(ex, 2.0), np.array([[-5, -10, 15, 30], [0, 0, 40, 40]], np.float32))


# ---- the samplers and the layers ----

@pytest.mark.parametrize("scale", TI.SCALES)
def test_samplers_against_the_reference(fixture, numpy_entries, scale):
    s = "s%d" % round(scale * 10)
    c = TI.layer_case(scale)
    assert TI.layer_case_digest(c) == str(fixture["%s_digest" % s])
    gt = T.pack_gt_masks(c["gt_boxes"], c["gt_masks"], c["mask_info"], c["im_info"][0, 2])
    all_rois = np.vstack((c["rois"], np.hstack((np.zeros((3, 1), np.float32), c["gt_boxes"][:, :-1]))))
    for seed in TI.SAMPLE_SEEDS:
        np.random.seed(seed)
        blobs, fg, bg, keep = T.sample_rois(all_rois, c["gt_boxes"], 64, TI.NUM_CLASSES, gt, c["im_info"][0, 2])
        key = "%s_sr%d_" % (s, seed)
        for name, v in blobs.items():
            if name in ("mask_targets", "mask_weight"):
                assert v.dtype == np.float64 and same(v.astype(np.uint8), unpack(fixture, key + name)), name
            else:
                assert same(v, fixture[key + name]), name
        assert same(fg, fixture[key + "fg"]) and same(bg, fixture[key + "bg"]) and same(keep, fixture[key + "keep"])
    out = T.stage_bridge_targets(all_rois.astype(np.float64), c["gt_boxes"], c["im_info"][0, 2], gt, TI.NUM_CLASSES)
    for name, v in zip(("labels", "rois", "fg", "keep", "mask_targets", "info", "bbox_targets", "inside"), out):
        if name == "mask_targets":
            assert v.dtype == np.float64 and same(v.astype(np.uint8), unpack(fixture, "%s_so_%s" % (s, name)))
        else:
            assert same(v, fixture["%s_so_%s" % (s, name)]), name


def layers_against_the_fixture(fixture, scale):
    """The four layers on the fixture's inputs, every top equal (shared with tests/test_gpu_train_targets.py)."""
    from mnc_config import cfg
    from pylayer.anchor_target_layer import AnchorTargetLayer
    from pylayer.mask_layer import MaskLayer
    from pylayer.proposal_target_layer import ProposalTargetLayer
    from pylayer.stage_bridge_layer import StageBridgeLayer
    s = "s%d" % round(scale * 10)
    c = TI.layer_case(scale)
    assert TI.layer_case_digest(c) == str(fixture["%s_digest" % s])
    want = tops_of(fixture, s + "_pt", 10, packed=(5, 6))
    np.random.seed(TI.LAYER_SEED)
    layer, pt = run_layer(ProposalTargetLayer, [c["rois"], c["gt_boxes"], c["im_info"], c["gt_masks"], c["mask_info"],
                                                c["proposal_index"]], 10, TI.TARGET_PARAMS)
    for i in range(10):
        assert same(pt[i], want[i]), "ProposalTargetLayer top %d" % i
    assert len(layer._keep_ind) == len(pt[0])
    for variant, keys in TI.ANCHOR_VARIANTS.items():
        old = {k: cfg.TRAIN[k] for k in keys}
        cfg.TRAIN.update(keys)
        try:
            np.random.seed(TI.LAYER_SEED)
            _, at = run_layer(AnchorTargetLayer, [c["rpn_cls_score"], c["gt_boxes"], c["im_info"], want[8], want[9]], 4,
                              TI.ANCHOR_PARAMS)
        finally:
            cfg.TRAIN.update(old)
        for i, w in enumerate(tops_of(fixture, "%s_at_%s" % (s, variant), 4)):
            assert same(at[i], w), "AnchorTargetLayer %s top %d" % (variant, i)
    pred = TI.mask_pred_for(want[5], want[7])
    layer, mk = run_layer(MaskLayer, [pred, c["gt_masks"], want[7]], 2)
    assert same(mk[0], pred.reshape(-1, 1, 21, 21)) and same(mk[1], fixture["%s_mk_top1" % s])
    assert same(layer.pos_sample, np.where(mk[1] > 0)[0]) and len(layer.pos_sample) > 0
    bbox_pred, seg_prob = TI.bridge_inputs(len(want[0]))
    layer, sb = run_layer(StageBridgeLayer, [want[0], bbox_pred, seg_prob, c["gt_boxes"], c["gt_masks"], c["im_info"], c["mask_info"]],
                          8, TI.BRIDGE_PARAMS)
    for i, w in enumerate(tops_of(fixture, s + "_sb", 8, packed=(2, 3))):
        assert same(sb[i], w), "StageBridgeLayer top %d" % i
    assert len(layer._keep_inds) == len(sb[0]) and same(layer._bbox_reg_labels, seg_prob[:, 1:].argmax(1) + 1)
    assert set(layer._clip_keep.tolist()) <= set(range(len(sb[0])))
    for cls in (ProposalTargetLayer, AnchorTargetLayer, MaskLayer, StageBridgeLayer):
        with pytest.raises(NotImplementedError):
            cls().backward([], [], [])


@pytest.mark.parametrize("scale", TI.SCALES)
def test_the_four_layers_against_the_reference(fixture, numpy_entries, scale):
    layers_against_the_fixture(fixture, scale)


def test_anchor_draws_are_exercised(fixture):
    """The fixture's anchor cases have more anchors inside the border than a batch holds, so the random draws run: the labelled
    anchors are at most the batch plus the rows that cfg.TRAIN.MIX_INDEX forces afterwards."""
    for s in ("s10", "s16"):
        forced = len(fixture["%s_pt_top8" % s]) + len(fixture["%s_pt_top9" % s])
        for variant, batch in (("default", 256), ("clobber", 16)):
            labels, targets = fixture["%s_at_%s_top0" % (s, variant)], fixture["%s_at_%s_top1" % (s, variant)]
            inside = int(targets.reshape(9, 4, -1).any(1).sum())
            assert inside > 256 + forced and 0 < (labels >= 0).sum() <= batch + forced and (labels == 1).any() and (labels == 0).any()


def test_test_phase_of_the_two_layers_is_unchanged(golden, numpy_entries):
    from pylayer.mask_layer import MaskLayer
    from pylayer.stage_bridge_layer import StageBridgeLayer
    _, (out,) = run_layer(StageBridgeLayer, [golden["sb_rois"], golden["sb_bbox_pred"], golden["sb_scores"], golden["sb_im_info"]], 1,
                          phase="TEST")
    assert same(out, golden["sb_rois_ext"])
    _, (out,) = run_layer(MaskLayer, [golden["ml_in"]], 1, phase="TEST")
    assert same(out, golden["ml_out"])
    for cls in (MaskLayer, StageBridgeLayer):
        layer = cls()
        layer.phase = "VALIDATE"
        with pytest.raises(NotImplementedError):
            layer.setup([], [Blob()])


# ---- refusals ----

def _gone(*a, **k):
    raise AssertionError("the library was looked for")


@pytest.mark.parametrize("device", [False, True])
def test_refusals_name_the_offending_number(corpus, monkeypatch, device):
    """By the statements, and by the device functions before the library is looked for."""
    monkeypatch.setattr(_lib, "call", _gone)
    monkeypatch.setattr(_lib, "load", _gone)
    tg = T.mask_targets if device else T.mask_targets_numpy
    po = T.mask_pred_overlaps if device else T.mask_pred_overlaps_numpy
    box, one = np.array([[0, 0, 9, 9]], np.int32), np.array([0])
    bad = [(dict(ex_boxes=[[5, 0, 4, 9]]), "box 0"), (dict(ex_boxes=[[0, 7, 9, 6]]), "box 0"),
           (dict(ex_boxes=[[0, 0, 2 ** 24, 9]]), "out of range"), (dict(ex_boxes=[[-2 ** 24, 0, 9, 9]]), "out of range"),
           (dict(ex_boxes=[[0, 0, 8192, 8191]]), "%d pixels" % (8193 * 8192)), (dict(gt_index=[len(corpus)]), "= %d" % len(corpus)),
           (dict(gt_index=[-1]), "= -1"), (dict(S=0), "mask_size 0"), (dict(S=33), "mask_size 33"), (dict(thresh=float("nan")), "NaN"),
           (dict(ex_boxes=np.zeros((65537, 4), np.int32), gt_index=np.zeros(65537, np.int32)), "K=65537")]
    for kw, message in bad:
        args = dict(ex_boxes=box, gt_index=one, S=21, thresh=0.4)
        args.update(kw)
        with pytest.raises(ValueError, match=message):
            tg(corpus, np.asarray(args["ex_boxes"], np.int64), args["gt_index"], args["S"], args["thresh"])
    pred = np.zeros((1, 21, 21), np.float32)
    with pytest.raises(ValueError, match="= %d" % len(corpus)):
        po(corpus, [[0.0, 0, 9, 9]], pred, [len(corpus)])
    with pytest.raises(ValueError, match="= -2"):
        po(corpus, [[0.0, 0, 9, 9]], pred, [-2])
    with pytest.raises(ValueError, match="mask_size 33"):
        po(corpus, [[0.0, 0, 9, 9]], np.zeros((1, 33, 33), np.float32), [0])
    with pytest.raises(ValueError, match="K=65537"):
        po(corpus, np.zeros((65537, 4)), np.zeros((65537, 1, 1), np.float32), np.zeros(65537, np.int32))
    if not device:                                       # (the boxes of the device function are checked by the library)
        for b in ([[5.4, 0, 4.4, 9]], [[0, 0, 2.0 ** 24, 9]], [[0, 0, 8192, 8191]]):
            with pytest.raises(ValueError, match="box 0"):
                po(corpus, b, pred, [0])


def test_pack_gt_masks_names_the_instance_that_disagrees():
    c = TI.layer_case(1.6)
    gt = T.pack_gt_masks(c["gt_boxes"], c["gt_masks"], c["mask_info"], 1.6)
    assert len(gt) == 3 and same(gt.areas, np.array([int(m.sum()) for m in c["gt_masks"]], np.int64))
    assert same(gt.bounds, np.around(c["gt_boxes"][:, :4] / 1.6).astype(np.int32)) and same(gt.classes, np.array([3, 12, 7], np.int32))
    info = c["mask_info"].copy()
    info[1, 1] += 1
    with pytest.raises(ValueError, match="instance 1"):
        T.pack_gt_masks(c["gt_boxes"], c["gt_masks"], info, 1.6)
    masks = c["gt_masks"].copy()
    masks[2, 0, 0] = 0.5
    with pytest.raises(ValueError, match="instance 2"):
        T.pack_gt_masks(c["gt_boxes"], masks, c["mask_info"], 1.6)
