"""The SDS evaluation with its pixel counting on the device (utils/voc_eval.py:voc_eval_sds_device, mnc_sds_best_overlap) without
a GPU: the GT packing, the vectorised matching fed by a numpy stand-in for the entry built from the CPU loop's own resize_to +
mask_overlap, the argument checks that run before any device work, no CPU fallback, and the public surface."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import golden_inputs as GI  # noqa: E402
import sds_eval_inputs as E  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from datasets.pascal_voc_seg import CLASSES  # noqa: E402

THRESHS = (0.3, 0.5, 0.7, 0.9)


@pytest.fixture(scope="module")
def rnd(tmp_path_factory):
    case = E.random_case()
    root = str(tmp_path_factory.mktemp("sds_rnd"))
    return case, E.write_case(root, case)


def _inputs(case, paths):
    from utils.voc_eval import sds_device_inputs
    out, cache, _ = paths
    return sds_device_inputs(os.path.join(out, "{}_det.pkl"), os.path.join(out, "{}_seg.pkl"), case["names"], CLASSES, cache)


def test_gt_packing_round_trips(rnd):
    case, paths = rnd
    d = _inputs(case, paths)
    G = len(d["gt_dicts"])
    assert G > 200 and d["gt_bounds"].shape == (G, 4) and d["gt_bits"].dtype == np.uint8
    assert d["gt_offsets"][0] == 0 and np.all(np.diff(d["gt_offsets"]) > 0)
    for gd, b, m, a in zip(d["gt_dicts"], d["gt_bounds"], E.unpack_gt(d["gt_bounds"], d["gt_offsets"], d["gt_bits"]),
                           d["gt_areas"]):
        assert np.array_equal(b, np.round(gd["mask_bound"]).astype(int)) and np.array_equal(m, gd["mask"]) and a == gd["mask"].sum()
    # per prediction: the range is exactly the cached list of its (class, image), empty without one
    assert sum(hi - lo for lo, hi in d["slices"]) == len(d["boxes"]) == sum(len(b) for cl in case["boxes"] for b in cl)
    for ci, (lo, hi) in enumerate(d["slices"]):
        c = ci + 1
        for p in range(lo, hi, 7):
            box = d["boxes"][p]
            ii = next(i for i in range(len(case["names"])) if any(np.array_equal(box, r[:4]) for r in case["boxes"][c][i]))
            want = case["gt"].get(c, {}).get(case["names"][ii], [])
            got = d["gt_dicts"][d["gt_begin"][p]:d["gt_end"][p]]
            assert len(got) == len(want) and all(g is w or np.array_equal(g["mask"], w["mask"]) for g, w in zip(got, want))
    assert any(d["gt_begin"][lo:hi].size and np.all(d["gt_begin"][lo:hi] == d["gt_end"][lo:hi]) for lo, hi in d["slices"])


def _greedy(best_gt, ov, thr):
    """voc_eval_sds's own matching loop on given best GTs / overlaps."""
    seen, tp = set(), np.zeros(len(best_gt))
    for i, (g, o) in enumerate(zip(best_gt, ov)):
        if g >= 0 and o >= thr and g not in seen:
            tp[i] = 1
            seen.add(g)
    return tp, 1 - tp


def test_vectorised_matching_reproduces_the_cpu_loop(rnd, monkeypatch):
    from utils import voc_eval
    case, paths = rnd
    out, cache, lst = paths
    d = _inputs(case, paths)
    bg, bi, bu, bo = E.loop_best_overlap(d["boxes"], d["masks"], d["gt_begin"], d["gt_end"], d["gt_dicts"])
    ov = np.where(bu >= 1, bi / np.maximum(bu, 1), 0.0)
    assert np.array_equal(ov, bo)                                    # inter / union is mask_overlap's value
    for thr in THRESHS:
        for lo, hi in d["slices"]:
            tp, fp = voc_eval.sds_match(bg[lo:hi], ov[lo:hi], thr, d["gt_pre"])
            wtp, wfp = _greedy(bg[lo:hi], ov[lo:hi], thr)
            assert np.array_equal(tp, wtp) and np.array_equal(fp, wfp)
    monkeypatch.setattr(voc_eval, "sds_best_overlap", E.numpy_entry)
    with np.errstate(all="ignore"):
        got = voc_eval.voc_eval_sds_device(os.path.join(out, "{}_det.pkl"), os.path.join(out, "{}_seg.pkl"), out, lst, CLASSES,
                                           cache, ov_threshs=THRESHS)
    for thr in THRESHS:
        want = E.cpu_aps(out, cache, lst, thr)
        assert np.array_equal(np.array(got[thr]), np.array(want), equal_nan=True), thr
    assert 0.05 < got[0.7][0] < 0.95


def test_pre_matched_gt_is_never_a_true_positive():
    from utils.voc_eval import sds_match
    tp, fp = sds_match(np.array([0, 1, 1, -1, 0]), np.array([0.9, 0.8, 0.6, 0.0, 0.95]), 0.5, np.array([True, False]))
    assert tp.tolist() == [0, 1, 0, 0, 0] and fp.tolist() == [1, 0, 1, 1, 1]


def test_golden_devkit_with_the_numpy_entry(tmp_path, monkeypatch):
    from datasets.pascal_voc_seg import PascalVOCSeg
    from utils import voc_eval
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_eval_outputs.npz"))
    case = GI.sds_case()
    root = str(tmp_path / "VOCdevkitSDS")
    GI.write_sds_devkit(root, case)
    monkeypatch.setattr(voc_eval, "sds_best_overlap", E.numpy_entry)
    imdb = PascalVOCSeg("val", "2012", root, image_ext=".npy")
    out = str(tmp_path / "out")
    os.mkdir(out)
    with np.errstate(all="ignore"):
        res = imdb.evaluate_segmentation(case["pred_boxes"], case["pred_masks"], out, on_device=True)
    assert np.array_equal(np.array(res[0.5]), ref["eval_ap_05"], equal_nan=True)
    assert np.array_equal(np.array(res[0.7]), ref["eval_ap_07"], equal_nan=True)


def test_switch_defaults_to_the_cpu_evaluator(tmp_path, monkeypatch):
    from datasets.pascal_voc_seg import PascalVOCSeg
    from mnc_config import cfg
    from utils import voc_eval
    assert cfg.TEST.USE_GPU_SDS_EVAL is False
    case = GI.sds_case()
    root = str(tmp_path / "VOCdevkitSDS")
    GI.write_sds_devkit(root, case)
    calls = []
    monkeypatch.setattr(voc_eval, "sds_best_overlap", lambda *a, **k: calls.append(1) or E.numpy_entry(*a, **k))
    imdb = PascalVOCSeg("val", "2012", root, image_ext=".npy")
    out = str(tmp_path / "out")
    os.mkdir(out)
    with np.errstate(all="ignore"):
        a = imdb.evaluate_segmentation(case["pred_boxes"], case["pred_masks"], out)
        assert not calls
        monkeypatch.setitem(cfg.TEST, "USE_GPU_SDS_EVAL", True)
        b = imdb.evaluate_segmentation(case["pred_boxes"], case["pred_masks"], out)
    assert calls == [1] and a == b


def test_non_binary_masks_are_refused(tmp_path):
    import pickle
    from utils.voc_eval import sds_class_predictions
    with open(str(tmp_path / "d.pkl"), "wb") as f:
        pickle.dump([np.array([[0, 0, 5, 5, 0.9]])], f)
    with open(str(tmp_path / "s.pkl"), "wb") as f:
        pickle.dump([np.full((1, 21, 21), 0.5)], f)
    with pytest.raises(ValueError):
        sds_class_predictions(str(tmp_path / "d.pkl"), str(tmp_path / "s.pkl"), 1)


def _entry(boxes, masks, begin, end, bounds=None, offsets=None, bits=None, areas=None, device_id=0):
    boxes = np.ascontiguousarray(boxes, np.float64)
    P = len(boxes)
    masks = np.ascontiguousarray(masks, np.uint8)
    begin, end = np.ascontiguousarray(begin, np.int32), np.ascontiguousarray(end, np.int32)
    G = 0 if bounds is None else len(bounds)
    out = np.zeros(P, np.int32), np.zeros(P, np.int64), np.zeros(P, np.int64)
    _lib.call("mnc_sds_best_overlap", _lib.ptr(boxes), _lib.ptr(masks), P, 21, _lib.ptr(begin), _lib.ptr(end), G,
              _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(bits), 0 if bits is None else bits.size, _lib.ptr(areas), 0.4,
              _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), device_id)
    return out


def test_entry_checks_arguments_before_any_device_work():
    ones = np.ones((1, 441), np.uint8)
    z = np.zeros(1, np.int32)
    _entry(np.zeros((0, 4)), np.zeros((0, 441)), np.zeros(0), np.zeros(0))              # P == 0: nothing to do, no device
    for box in ([10, 0, 9, 9], [10, 0, 7, 9], [0, 10.5, 5, 9.4], [0, 0, np.nan, 5]):      # width 0, width -2, height 0, NaN
        with pytest.raises(_lib.MncError) as e:
            _entry(np.array([box], np.float64), ones, z, z)
        assert e.value.code == 1
    with pytest.raises(_lib.MncError) as e:
        _entry(np.array([[0, 0, 5, 5]], np.float64), ones, z, z + 1)                   # GT range past G = 0
    assert e.value.code == 1
    bounds = np.array([[0, 0, 9, 9]], np.int32)
    with pytest.raises(_lib.MncError) as e:                                             # bit rows past the buffer
        _entry(np.array([[0, 0, 5, 5]], np.float64), ones, z, z + 1, bounds, np.zeros(1, np.int64), np.zeros(10, np.uint8),
               np.zeros(1, np.int64))
    assert e.value.code == 1


@pytest.mark.skipif(_lib.device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_errors_not_fallbacks(rnd):
    from utils.voc_eval import voc_eval_sds_device
    case, (out, cache, lst) = rnd
    with pytest.raises(_lib.MncError) as e:
        _entry(np.array([[0, 0, 5, 5]], np.float64), np.ones((1, 441), np.uint8), np.zeros(1), np.zeros(1))
    assert e.value.code in (1, 2) and str(e.value)
    with pytest.raises(_lib.MncError):
        voc_eval_sds_device(os.path.join(out, "{}_det.pkl"), os.path.join(out, "{}_seg.pkl"), out, lst, CLASSES, cache)


def test_entry_is_exported_and_declared():
    decls = _lib.parse_header()
    assert decls["mnc_sds_best_overlap"][2] == ["boxes", "masks", "P", "mask_size", "gt_begin", "gt_end", "G", "gt_bounds",
                                                "gt_offsets", "gt_bits", "gt_bytes", "gt_areas", "binarize_thresh", "best_gt",
                                                "best_inter", "best_union", "device_id"]
    assert decls["mnc_sds_best_overlap"][1][10] is ctypes.c_size_t and decls["mnc_sds_best_overlap"][1][12] is ctypes.c_double
    _lib.load()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T mnc_sds_best_overlap" in syms


def _golden_run(tmp_path):
    """The synthetic devkit registered as an imdb, and the result pickles a seg run on it would leave."""
    import pickle
    from datasets.pascal_voc_seg import PascalVOCSeg
    from db.imdb import add_imdb
    case = GI.sds_case()
    root = str(tmp_path / "VOCdevkitSDS")
    GI.write_sds_devkit(root, case)
    add_imdb("sds_eval_golden", lambda: PascalVOCSeg("val", "2012", root, image_ext=".npy"))
    out = str(tmp_path / "run")
    os.mkdir(out)
    with open(os.path.join(out, "res_boxes.pkl"), "wb") as f:
        pickle.dump(case["pred_boxes"], f)
    with open(os.path.join(out, "res_masks.pkl"), "wb") as f:
        pickle.dump(case["pred_masks"], f)
    return out


def test_eval_seg_tool_reevaluates_a_run(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_seg
    from utils import voc_eval
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_eval_outputs.npz"))
    out = _golden_run(tmp_path)
    assert eval_seg.parse_args(["--output-dir", out]).cpu is False
    calls = []
    monkeypatch.setattr(voc_eval, "sds_best_overlap", lambda *a, **k: calls.append(1) or E.numpy_entry(*a, **k))
    with np.errstate(all="ignore"):
        dev = eval_seg.main(["--imdb", "sds_eval_golden", "--output-dir", out])
        assert calls == [1]
        cpu = eval_seg.main(["--imdb", "sds_eval_golden", "--output-dir", out, "--cpu"])
    assert calls == [1]
    for res in (dev, cpu):
        assert np.array_equal(np.array(res[0.5]), ref["eval_ap_05"], equal_nan=True)
        assert np.array_equal(np.array(res[0.7]), ref["eval_ap_07"], equal_nan=True)


def test_config_file_switches_the_evaluation_on(tmp_path, monkeypatch):
    """test_net.py --cfg <file> with TEST: {USE_GPU_SDS_EVAL: True} evaluates on the device."""
    from mnc_config import cfg, cfg_from_file
    monkeypatch.setitem(cfg.TEST, "USE_GPU_SDS_EVAL", False)
    y = tmp_path / "sds_gpu.yml"
    y.write_text("TEST:\n  USE_GPU_SDS_EVAL: True\n")
    cfg_from_file(str(y))
    assert cfg.TEST.USE_GPU_SDS_EVAL is True
