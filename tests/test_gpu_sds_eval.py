"""The SDS mAP^r evaluation with its pixel counting on the GPU (csrc/sds_eval.hip, mnc_sds_best_overlap, utils/voc_eval.py:
voc_eval_sds_device): the reference's own APs on the synthetic devkit, per-prediction equality with voc_eval_sds's loop and its
APs on a random case, the pinned rules, and one whole-dataset-sized call."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import golden_inputs as GI  # noqa: E402
import sds_eval_inputs as E  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from datasets.pascal_voc_seg import CLASSES  # noqa: E402

pytestmark = pytest.mark.gpu

S = 21


def test_golden_devkit_matches_the_reference(tmp_path):
    from datasets.pascal_voc_seg import PascalVOCSeg
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_eval_outputs.npz"))
    case = GI.sds_case()
    root = str(tmp_path / "VOCdevkitSDS")
    GI.write_sds_devkit(root, case)
    imdb = PascalVOCSeg("val", "2012", root, image_ext=".npy")
    out = str(tmp_path / "out")
    os.mkdir(out)
    with np.errstate(all="ignore"):
        res = imdb.evaluate_segmentation(case["pred_boxes"], case["pred_masks"], out, on_device=True)
    assert np.array_equal(np.array(res[0.5]), ref["eval_ap_05"], equal_nan=True)
    assert np.array_equal(np.array(res[0.7]), ref["eval_ap_07"], equal_nan=True)


def test_random_case_per_prediction_and_aps(tmp_path):
    from utils.voc_eval import sds_best_overlap, sds_device_inputs, voc_eval_sds_device
    case = E.random_case()
    out, cache, lst = E.write_case(str(tmp_path), case)
    d = sds_device_inputs(os.path.join(out, "{}_det.pkl"), os.path.join(out, "{}_seg.pkl"), case["names"], CLASSES, cache)
    assert len(d["boxes"]) == 3000
    w = np.round(d["boxes"][:, 2]) - np.round(d["boxes"][:, 0]) + 1
    assert (w < S).any() and (w > S).any() and (d["boxes"] % 1 == 0.5).any()
    assert (d["boxes"].astype(np.float32).astype(np.float64) != d["boxes"]).any()
    assert (d["gt_begin"] == d["gt_end"]).any() and not all(d["num_pos"])
    got = sds_best_overlap(d["boxes"], d["masks"], d["gt_begin"], d["gt_end"], d["gt_bounds"], d["gt_offsets"], d["gt_bits"],
                           d["gt_areas"], 0.4)
    want = E.loop_best_overlap(d["boxes"], d["masks"], d["gt_begin"], d["gt_end"], d["gt_dicts"])
    for g, wv in zip(got, want[:3]):
        assert np.array_equal(g, wv)
    threshs = (0.3, 0.5, 0.7, 0.9)
    with np.errstate(all="ignore"):
        res = voc_eval_sds_device(os.path.join(out, "{}_det.pkl"), os.path.join(out, "{}_seg.pkl"), out, lst, CLASSES, cache,
                                  ov_threshs=threshs)
    for thr in threshs:
        assert np.array_equal(np.array(res[thr]), np.array(E.cpu_aps(out, cache, lst, thr)), equal_nan=True), thr


def _full_gt(x1, y1, x2, y2):
    return {"mask": np.ones((y2 - y1 + 1, x2 - x1 + 1), bool), "mask_bound": np.array([x1, y1, x2, y2], np.float64),
            "mask_cls": 1, "already_detect": False}


def _one_class_case(tmp_path, gts, preds):
    """Class 1 (aeroplane) of one image: GT instances and (box, score) predictions with full masks."""
    case = {"names": ["img"], "gt": {1: {"img": gts} if gts else {}},
            "boxes": [[np.zeros((0, 5))] for _ in range(21)], "masks": [[np.zeros((0, S, S), bool)] for _ in range(21)]}
    case["boxes"][1][0] = np.array([list(b) + [s] for b, s in preds], np.float64)
    case["masks"][1][0] = np.ones((len(preds), S, S), bool)
    return E.write_case(str(tmp_path), case)


def _device_ap1(paths, threshs):
    from utils.voc_eval import voc_eval_sds_device
    out, cache, lst = paths
    with np.errstate(all="ignore"):
        return voc_eval_sds_device(os.path.join(out, "{}_det.pkl"), os.path.join(out, "{}_seg.pkl"), out, lst, CLASSES, cache,
                                   ov_threshs=threshs)


def test_exact_half_and_seven_tenths_are_true_positives(tmp_path):
    from utils.voc_eval import sds_best_overlap
    boxes = np.array([[0, 0, 9, 9], [0, 0, 9, 9]], np.float64)
    gts = [_full_gt(0, 0, 9, 19), _full_gt(0, 0, 9, 6)]                # 100 / 200 and 70 / 100
    from utils.voc_eval import pack_sds_gt
    bounds, offs, bits, areas, _ = pack_sds_gt(gts)
    bg, bi, bu = sds_best_overlap(boxes, np.ones((2, S * S), np.uint8), [0, 1], [1, 2], bounds, offs, bits, areas, 0.4)
    assert bg.tolist() == [0, 1] and bi.tolist() == [100, 70] and bu.tolist() == [200, 100]
    for gt, thr in ((gts[0], 0.5), (gts[1], 0.7)):
        paths = _one_class_case(tmp_path / str(thr), [gt], [([0, 0, 9, 9], 0.9)])
        ap = _device_ap1(paths, (thr,))[thr][0]
        assert ap == E.cpu_aps(*paths, thr)[0] and ap > 0.9                # a false positive would give 0


def test_empty_rounded_box_raises(tmp_path):
    from utils.voc_eval import sds_best_overlap
    for box in ([10, 0, 9, 9], [10, 0, 7, 9]):                             # width 0 and width -2 once rounded
        with pytest.raises(_lib.MncError):
            sds_best_overlap(np.array([box], np.float64), np.ones((1, S * S), np.uint8), [0], [0], np.zeros((0, 4)),
                             np.zeros(0), np.zeros(0), np.zeros(0), 0.4)
        paths = _one_class_case(tmp_path / str(box[2]), [_full_gt(0, 0, 9, 9)], [([0, 0, 9, 9], 0.9), (box, 0.5)])
        with pytest.raises(_lib.MncError):
            _device_ap1(paths, (0.5,))


def test_identical_gts_first_wins_and_matched_gt_makes_fp(tmp_path):
    from utils.voc_eval import pack_sds_gt, sds_best_overlap, sds_match
    gts = [_full_gt(0, 0, 9, 9), _full_gt(0, 0, 9, 9), _full_gt(40, 0, 49, 9)]
    bounds, offs, bits, areas, pre = pack_sds_gt(gts)
    boxes = np.array([[0, 0, 9, 9], [0, 0, 11, 9]], np.float64)
    bg, bi, bu = sds_best_overlap(boxes, np.ones((2, S * S), np.uint8), [0, 0], [3, 3], bounds, offs, bits, areas, 0.4)
    assert bg.tolist() == [0, 0] and bi.tolist() == [100, 100] and bu.tolist() == [100, 120]
    tp, fp = sds_match(bg, bi / bu, 0.5, pre)
    assert tp.tolist() == [1, 0] and fp.tolist() == [0, 1]             # GTs 1 and 2 are free, but the second's best is GT 0
    paths = _one_class_case(tmp_path, gts, [([0, 0, 9, 9], 0.9), ([0, 0, 11, 9], 0.8)])
    got = _device_ap1(paths, (0.5, 0.7))
    for thr in (0.5, 0.7):
        assert got[thr][0] == E.cpu_aps(*paths, thr)[0]


def test_whole_dataset_sized_call():
    from utils.voc_eval import pack_sds_gt, sds_best_overlap
    rng = np.random.default_rng(9)
    G, P = 10000, 200000
    gts = []
    for _ in range(G):
        w, h = int(rng.integers(1, 120)), int(rng.integers(1, 120))
        x1, y1 = int(rng.integers(0, 400)), int(rng.integers(0, 300))
        gts.append({"mask": rng.random((h, w)) < 0.7, "mask_bound": np.array([x1, y1, x1 + w - 1, y1 + h - 1], np.float64)})
    bounds, offs, bits, areas, _ = pack_sds_gt(gts)
    xy = rng.uniform(-20, 420, (P, 2))
    wh = rng.uniform(0.6, 250, (P, 2))
    boxes = np.hstack([xy, xy + wh])
    masks = (rng.random((P, S * S)) < 0.5).astype(np.uint8)
    begin = rng.integers(0, G - 6, P).astype(np.int32)
    end = (begin + rng.integers(0, 6, P)).astype(np.int32)
    bg, bi, bu = sds_best_overlap(boxes, masks, begin, end, bounds, offs, bits, areas, 0.4)
    empty = begin == end
    assert np.all(bg[empty] == -1) and np.all(bi[empty] == 0) and np.all(bu[empty] == 0)
    assert np.all((bg[~empty] >= begin[~empty]) & (bg[~empty] < end[~empty]))
    assert np.all((bi >= 0) & (bi <= bu))
    sample = rng.choice(P, 2000, replace=False)
    want = E.loop_best_overlap(boxes[sample], masks[sample], begin[sample], end[sample], gts)
    assert np.array_equal(bg[sample], want[0]) and np.array_equal(bi[sample], want[1]) and np.array_equal(bu[sample], want[2])


def test_eval_seg_tool_on_the_device(tmp_path):
    """tools/eval_seg.py re-evaluates the result pickles of a run on the GPU: the reference's APs."""
    import pickle
    from datasets.pascal_voc_seg import PascalVOCSeg
    from db.imdb import add_imdb
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_seg
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_eval_outputs.npz"))
    case = GI.sds_case()
    root = str(tmp_path / "VOCdevkitSDS")
    GI.write_sds_devkit(root, case)
    add_imdb("sds_eval_golden_gpu", lambda: PascalVOCSeg("val", "2012", root, image_ext=".npy"))
    out = str(tmp_path / "run")
    os.mkdir(out)
    with open(os.path.join(out, "res_boxes.pkl"), "wb") as f:
        pickle.dump(case["pred_boxes"], f)
    with open(os.path.join(out, "res_masks.pkl"), "wb") as f:
        pickle.dump(case["pred_masks"], f)
    with np.errstate(all="ignore"):
        res = eval_seg.main(["--imdb", "sds_eval_golden_gpu", "--output-dir", out])
    assert np.array_equal(np.array(res[0.5]), ref["eval_ap_05"], equal_nan=True)
    assert np.array_equal(np.array(res[0.7]), ref["eval_ap_07"], equal_nan=True)
