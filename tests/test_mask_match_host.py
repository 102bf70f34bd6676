"""COCO-style matching and mask AP of packed instance masks, the host side (mnc_amd/coco_eval.py: match_numpy, accumulate,
summarize, CocoSegmEval(device=False); tools/eval_coco.py --cpu; the argument checks of mnc_mask_match that need no GPU).  The
hand-made cases of the matching rule with their expected tables written out, the closed form against the walk, one end-to-end
value worked out by hand.  Every comparison of tables is exact."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_match_inputs as MM  # noqa: E402  (sets up the reference-shaped import paths)
from mnc_amd import _lib, coco_eval, rle  # noqa: E402
from mnc_amd.coco_eval import CocoSegmEval, Match, match_closed_numpy, match_numpy  # noqa: E402
from mnc_amd.masks import _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

# name -> (rank [D], dt_match [A][T][D], dt_ignore [A][T][D], gt_match [A][T][G], gt_ignore [A][G], iou [D][G])
EXPECTED = {
    "threshold": ([0], [[[0], [-1]]], [[[0], [0]]], [[[0], [-1]]], [[0]], [[0.5]]),
    "identical_gts": ([0, 1], [[[1, 0]]], [[[0, 0]]], [[[1, 0]]], [[0, 0]], [[1.0, 1.0], [1.0, 1.0]]),
    "not_ignored_wins": ([0], [[[1]]], [[[0]]], [[[-1, 0]]], [[1, 0]], [[1.0, 0.6]]),
    "crowd": ([0, 1, 2], [[[0, 0, 0]]], [[[1, 1, 1]]], [[[2]]], [[1]], [[1.0], [0.5], [0.5]]),
    "ignore_once": ([0, 1], [[[0, -1]]], [[[1, 0]]], [[[0]]], [[1]], [[1.0], [1.0]]),
    "area": ([0, 1], [[[-1, -1]], [[-1, -1]]], [[[0, 0]], [[1, 0]]], [[[-1]], [[-1]]], [[0], [1]], [[0.0], [0.0]]),
    # ranks: 0.9, 0.7, then the three 0.5 by index; detections 2 and 3 are past max_det: unmatched and not ignored, whatever
    # their size; in the range [0, 5] the ground truths (10 pixels) are ignored, so are the detections matched to them
    "max_det": ([2, 0, 3, 4, 1], [[[0, 1, -1, -1, 4]], [[0, 1, -1, -1, 4]]], [[[0, 0, 0, 0, 0]], [[1, 1, 0, 0, 1]]],
                [[[0, 1, -1, -1, 4]], [[0, 1, -1, -1, 4]]], [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], np.eye(5).tolist()),
    "classes": ([0, 0], [[[0, -1]]], [[[0, 0]]], [[[0, -1]]], [[0, 0]], [[1.0, 0.0], [0.0, 1.0]]),
    "no_detections": ([], [[[]], [[]]], [[[]], [[]]], [[[-1, -1]], [[-1, -1]]], [[0, 1], [1, 1]], np.zeros((0, 2)).tolist()),
    "no_ground_truths": ([1, 0], [[[-1, -1]], [[-1, -1]]], [[[0, 0]], [[1, 0]]], [[[]], [[]]], [[], []], [[], []]),
    "nothing": ([], [[[]]], [[[]]], [[[]]], [[]], []),
}
DTYPES = (np.int32, np.int32, np.uint8, np.int32, np.uint8, np.float64)


def expected(name):
    c = MM.hand_cases()[name]
    D, G = len(c.dt), len(c.gt)
    A, T = len(c.kw["area_rngs"]), len(c.kw["iou_thrs"])
    shapes = ((D,), (A, T, D), (A, T, D), (A, T, G), (A, G), (D, G))
    return Match(*(np.array(v, t).reshape(s) for v, t, s in zip(EXPECTED[name], DTYPES, shapes)))


def same(got, want):
    for f, g, w in zip(Match._fields, got, want):
        if w is None:
            assert g is None, f
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f
    return True


@pytest.mark.parametrize("name", list(EXPECTED))
def test_hand_made_case_gives_the_tables_written_out(name):
    c = MM.hand_cases()[name]
    want = expected(name)
    assert same(match_numpy(c.dt, c.gt, return_iou=True, **c.kw), want)
    assert same(match_closed_numpy(c.dt, c.gt, return_iou=True, **c.kw), want)
    assert same(MT.mask_match_numpy(c.dt, c.gt, **c.kw), want._replace(iou=None))


def test_hand_made_cases_are_the_issue_s():
    assert list(MM.hand_cases()) == list(EXPECTED)
    crowd = MM.hand_cases()["crowd"]
    inter = np.array([100, 50, 50])
    assert np.array_equal(expected("crowd").iou[:, 0], inter / crowd.dt.areas) and crowd.gt.areas[0] == 1000   # inter / area_dt


@pytest.mark.parametrize("seed", MM.RANDOM_SEEDS)
def test_closed_form_equals_the_walk_on_random_sets(seed):
    c = MM.random_set(seed)
    want = match_numpy(c.dt, c.gt, return_iou=True, **c.kw)
    assert same(match_closed_numpy(c.dt, c.gt, return_iou=True, **c.kw), want)
    assert want.dt_match.shape == (4, 10, len(c.dt)) and len(set(c.dt.classes.tolist())) == 3
    matches, ignored, unmatched, taken = MM.degenerate(want, c.kw["iscrowd"])
    assert matches >= 20 and ignored >= 5 and unmatched >= 5 and taken > 1


def test_closed_form_equals_the_walk_across_chunks():
    c = MM.chunk_set(70, 130, 70)
    want = match_numpy(c.dt, c.gt, **c.kw)
    assert same(match_closed_numpy(c.dt, c.gt, **c.kw), want)
    # the two identical ground truths: the higher index first
    first, second = np.argsort(want.rank[:2])
    assert want.dt_match[0, 0, first] == 64 and want.dt_match[0, 0, second] in (63, -1)


def test_bad_parameters_raise():
    c = MM.hand_cases()["identical_gts"]
    for kw in ({"iou_thrs": []}, {"iou_thrs": [float("nan")]}, {"area_rngs": [[5, 1]]}, {"area_rngs": [[0, float("nan")]]},
               {"max_det": 0}, {"max_det": 2049}, {"iscrowd": [0, 2]}, {"ignore": [0, 3]}, {"iscrowd": [0]},
               {"iou_thrs": np.zeros(17)}, {"area_rngs": np.zeros((9, 2))}):
        with pytest.raises(ValueError):
            match_numpy(c.dt, c.gt, **dict(c.kw, **kw))


def _three_detections():
    """One image, one class, two disjoint ground truths; detections in score order: equals ground truth 1, touches nothing,
    equals ground truth 0."""
    g0, g1, none = [10, 10, 19, 19], [100, 40, 109, 49], [50, 0, 59, 4]
    return MM.solid([none, g1, g0], [1, 1, 1], [0.8, 0.9, 0.7]), MM.solid([g0, g1], [1, 1])


def test_end_to_end_value():
    dt, gt = _three_detections()
    ev = CocoSegmEval(device=False)
    m = ev.add("im0", dt, gt, [0, 0])
    assert m.rank.tolist() == [1, 0, 2] and m.dt_match[0, 0].tolist() == [-1, 1, 0]
    out = ev.summarize()
    assert list(out) == list(coco_eval.STAT_NAMES) and ev.stats.shape == (12,) and ev.stats.dtype == np.float64
    ap = (51 + 50 * 2.0 / 3.0) / 101
    assert abs(ap - 0.834983498349835) < 1e-15
    for k in ("AP", "AP50", "AP75", "APs"):                        # (the masks are 100 pixels: small)
        assert abs(out[k] - ap) < 1e-12, k
    assert out["AR1"] == 0.5 and out["AR10"] == 1.0 and out["AR100"] == 1.0 and out["ARs"] == 1.0
    assert out["APm"] == out["APl"] == out["ARm"] == out["ARl"] == -1.0           # no ground truth of that size
    assert np.array_equal(ev.stats, np.array(list(out.values())))
    acc = ev.eval
    assert acc["precision"].shape == (10, 101, 1, 4, 3) and acc["recall"].shape == (10, 1, 4, 3)
    lines = ev.lines()
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.835"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"


def test_accumulate_over_images_sorts_by_score_across_them():
    """Two images of the end-to-end kind: the false positive of one outscores a true positive of the other."""
    dt, gt = _three_detections()
    ev = CocoSegmEval(device=False)
    ev.add(2, dt, gt, [0, 0])
    ev.add(1, MM.solid([[10, 10, 19, 19]], [1], [0.85]), MM.solid([[10, 10, 19, 19]], [1]), [0])
    out = ev.summarize()
    # scores 0.9 tp, 0.85 tp, 0.8 fp, 0.7 tp over 3 ground truths: recall 1/3, 2/3, 2/3, 1; precision 1, 1, 3/4 (from the right), 3/4
    ap = (67 * 1.0 + 34 * 0.75) / 101
    assert abs(out["AP"] - ap) < 1e-12 and abs(out["AR1"] - 2.0 / 3.0) < 1e-12 and out["AR10"] == 1.0
    with pytest.raises(ValueError):
        ev.add(1, dt, gt, [0, 0])
    # a class without a not-ignored ground truth stays -1 and out of the means
    ev2 = CocoSegmEval(device=False)
    ev2.add(0, dt, gt, [0, 0])
    ev2.add(1, MM.solid([[0, 0, 3, 3]], [7], [0.5]), MM.solid([[0, 0, 3, 3]], [7]), [1])
    out2 = ev2.summarize()
    assert ev2.eval["classes"] == [1, 7] and (ev2.eval["precision"][:, :, 1] == -1).all()
    assert abs(out2["AP"] - 0.834983498349835) < 1e-12


def _files(tmp_path, polygon=False):
    """A ground-truth file and a results file over the random sets, written with the numpy codec -> (gt path, dt path, cases)."""
    cases = {"im%d" % s: MM.random_set(s, n_dt=30, n_gt=12) for s in MM.RANDOM_SEEDS[:2]}
    H, W = MM.H + 40, MM.W + 60                                    # (bounds may leave the frame: the file holds what lies inside)
    images, anns, results = [], [], []
    for name, c in cases.items():
        images.append({"id": name, "height": H, "width": W})
        for i, r in enumerate(rle.mask_rle_numpy(c.gt, H, W)):
            seg = r if i % 2 else {"size": r["size"], "counts": rle.string_to_counts(r["counts"]).tolist()}     # both RLE forms
            anns.append({"id": len(anns) + 1, "image_id": name, "category_id": int(c.gt.classes[i]), "segmentation": seg,
                         "iscrowd": int(c.kw["iscrowd"][i]), "area": float(c.kw["eval_area"][i]), "ignore": int(c.kw["ignore"][i])})
        for i, r in enumerate(rle.mask_rle_numpy(c.dt, H, W)):
            results.append({"image_id": name, "category_id": int(c.dt.classes[i]), "segmentation": r, "bbox": [0, 0, 0, 0],
                            "score": float(c.dt.scores[i])})
    if polygon:
        anns[3]["segmentation"] = [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]
    gt_path, dt_path = str(tmp_path / "gt.json"), str(tmp_path / "dt.json")
    with open(gt_path, "w") as f:
        json.dump({"images": images, "categories": [{"id": k} for k in (1, 2, 3)], "annotations": anns}, f)
    with open(dt_path, "w") as f:
        json.dump(results, f)
    return gt_path, dt_path, cases, (H, W)


def _tool(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "tools", "eval_coco.py")] + list(args), capture_output=True, text=True,
                          cwd=REPO)


def test_eval_coco_cpu_equals_the_evaluator_fed_directly(tmp_path):
    gt_path, dt_path, cases, (H, W) = _files(tmp_path)
    out_path = str(tmp_path / "stats.json")
    r = _tool("--gt", gt_path, "--dt", dt_path, "--cpu", "--out", out_path)
    assert r.returncode == 0, r.stderr[-2000:]
    ev = CocoSegmEval(device=False, classes=[1, 2, 3])
    for name, c in cases.items():
        # what the file holds: the part of every mask inside the image, in tight bounds
        dt = rle.masks_from_rle_numpy(rle.mask_rle_numpy(c.dt, H, W), c.dt.classes, c.dt.scores)
        gt = rle.masks_from_rle_numpy(rle.mask_rle_numpy(c.gt, H, W), c.gt.classes)
        ev.add(name, dt, gt, c.kw["iscrowd"], c.kw["ignore"], c.kw["eval_area"])
    want = ev.summarize()
    with open(out_path) as f:
        got = json.load(f)
    assert list(got["stats"]) == list(want) and [got["stats"][k] for k in want] == list(want.values())
    assert 0 < want["AP"] < 1 and want["AR1"] < want["AR100"]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(" Average")]
    assert lines == ev.lines() and got["lines"] == lines


def test_eval_coco_refuses_a_polygon(tmp_path):
    gt_path, dt_path, _, _ = _files(tmp_path, polygon=True)
    r = _tool("--gt", gt_path, "--dt", dt_path, "--cpu")
    assert r.returncode != 0 and "annotation 4" in r.stderr and "polygon" in r.stderr


def _call(dt, gt, kw, outputs=True, **over):
    """mnc_mask_match as it is, with single arguments replaced -> the return code (MncError's) or 0."""
    thrs = np.array(kw.get("iou_thrs", coco_eval.IOU_THRS), np.float64)
    rngs = np.array(kw.get("area_rngs", coco_eval.AREA_RNGS), np.float64).reshape(-1, 2)
    crowd = np.array(kw.get("iscrowd", np.zeros(len(gt))), np.uint8)
    ign = np.array(kw.get("ignore", np.zeros(len(gt))), np.uint8)
    area = np.array(gt.areas, np.float64)
    scores = np.array(over.get("scores", dt.scores), np.float32)
    D, G, A, T = over.get("nd", len(dt)), over.get("ng", len(gt)), over.get("A", len(rngs)), over.get("T", len(thrs))
    size = max(len(dt), 1) * max(len(gt), 1) * 16 * 8
    out = [np.zeros(size, t) for t in (np.int32, np.int32, np.uint8, np.int32, np.uint8)]
    ptrs = [_lib.ptr(o) for o in out]
    if over.get("null_output") is not None:
        ptrs[over["null_output"]] = None
    args = (_set_args(dt)[:5] + (D, _lib.ptr(dt.classes), _lib.ptr(scores)) + _set_args(gt)[:5] +
            (G, _lib.ptr(gt.classes), _lib.ptr(crowd), _lib.ptr(ign), _lib.ptr(area), _lib.ptr(thrs), T, _lib.ptr(rngs), A,
             over.get("max_det", kw.get("max_det", 100))) + tuple(ptrs) + (None, 0))
    try:
        return _lib.call("mnc_mask_match", *args), out
    except _lib.MncError as e:
        assert not any(o.any() for o in out)                      # refused before anything was written
        return e.code, out


def test_invalid_arguments_come_back_without_a_gpu():
    c = MM.hand_cases()["identical_gts"]
    INVALID = 1
    nan = float("nan")

    def rc(kw=None, **over):
        return _call(c.dt, c.gt, dict(c.kw, **(kw or {})), **over)[0]

    assert rc(nd=-1) == INVALID and rc(nd=2049) == INVALID and rc(ng=-1) == INVALID and rc(ng=2049) == INVALID
    assert rc(T=0) == INVALID and rc(T=17) == INVALID and rc(A=0) == INVALID and rc(A=9) == INVALID
    assert rc(max_det=0) == INVALID and rc(max_det=2049) == INVALID
    assert rc(scores=[0.5, nan]) == INVALID
    assert rc({"iou_thrs": [nan]}) == INVALID
    assert rc({"area_rngs": [[nan, 1.0]]}) == INVALID and rc({"area_rngs": [[0.0, nan]]}) == INVALID
    assert rc({"area_rngs": [[2.0, 1.0]]}) == INVALID                                   # lo > hi
    assert rc({"iscrowd": [0, 2]}) == INVALID and rc({"ignore": [255, 0]}) == INVALID
    for k in range(5):
        assert rc(null_output=k) == INVALID                                             # every table but the IoU is required
    # what mnc_mask_overlaps refuses of a set
    for field, value in (("bounds", [[0, 0, 2 ** 24, 0]]), ("offsets", [4]), ("offsets", [8])):     # coordinate, offset, rows past the bits
        bad = MM.solid([[0, 0, 0, 0]], [1], [0.5])
        bad._host[field] = np.array(value, bad._host[field].dtype)
        assert _call(bad, c.gt, c.kw)[0] == INVALID and _call(c.dt, bad, dict(c.kw, iscrowd=[0]))[0] == INVALID


@pytest.mark.parametrize("name", ["no_detections", "no_ground_truths", "nothing"])
def test_empty_sets_return_before_any_device_work(name):
    """D == 0 or G == 0: mnc_mask_match fills every table as the rule gives, on the host -- this passes without a GPU."""
    c = MM.hand_cases()[name]
    want = expected(name)
    code, out = _call(c.dt, c.gt, c.kw)
    assert code == 0
    for got, w in zip(out, want[:5]):
        assert np.array_equal(got[:w.size], w.reshape(-1)), name
    assert same(coco_eval.match(c.dt, c.gt, return_iou=True, **c.kw), want)
    assert same(c.dt.match(c.gt, **c.kw), want._replace(iou=None))
    # more detections than max_det, no ground truth: only the participating ones get the size rule
    dt = MM.solid([[0, 0, 9, 9]] * 3, [1, 1, 2], [0.5, 0.5, 0.1])
    kw = {"area_rngs": [[0, 50]], "iou_thrs": [0.5], "max_det": 1}
    got = coco_eval.match(dt, MM.solid([]), [], **kw)
    assert same(got, match_numpy(dt, MM.solid([]), [], **kw)) and got.dt_ignore.reshape(-1).tolist() == [1, 0, 1]


def test_header_declares_and_library_exports_the_entries():
    decls = _lib.parse_header()
    lib = _lib.load()
    for name, nargs in (("mnc_mask_match", 30), ("mnc_mask_match_dev", 26)):
        assert name in decls and len(decls[name][1]) == nargs and decls[name][0] is ctypes.c_int
        assert getattr(lib, name) is not None
    assert decls["mnc_mask_match"][2][-7:] == ["rank", "dt_match", "dt_ignore", "gt_match", "gt_ignore", "iou", "device_id"]
    assert MT.mask_match is not None and MT.mask_match_numpy is not None
