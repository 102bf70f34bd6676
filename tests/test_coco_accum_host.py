"""COCO's accumulate in one device call, the host side (mnc_amd/coco_eval.py: flatten_records, accumulate_flat_numpy, the argument
checks and the host-answered empty inputs of mnc_coco_accumulate, CocoSegmEval(device=False)): everything here passes without a
GPU.  Every comparison of tables is exact."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import coco_accum_inputs as CA  # noqa: E402  (sets up the import paths)
import mask_match_inputs as MM  # noqa: E402
from mnc_amd import _lib, coco_eval  # noqa: E402
from mnc_amd.coco_eval import CocoSegmEval  # noqa: E402

INVALID = 1


def _flat(name):
    c, _ = CA.oracle(name)
    return c, coco_eval.flatten_records(c.images, c.kw["classes"], c.kw["max_dets"])


@pytest.mark.parametrize("name", ["tiny", "empty_cells", "small_parameters"])
def test_flatten_records_equals_the_plain_loop(name):
    c, got = _flat(name)
    want = CA.flatten_loop(c.images, c.kw["classes"], c.kw["max_dets"])
    assert list(got) == list(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
        assert got[key].flags["C_CONTIGUOUS"], key
    assert (got["dt_class_idx"] == -1).any() == (name == "empty_cells")          # the class that is not evaluated
    assert got["dt_score"].view(np.uint32).tolist() == want["dt_score"].view(np.uint32).tolist()


def test_flatten_records_of_no_images_and_bad_records():
    got = coco_eval.flatten_records([], [1, 2], (1, 10), T=10, A=4)
    assert got["dt_flags"].shape == (4, 10, 0) and got["gt_ignore"].shape == (4, 0) and len(got["dt_class_idx"]) == 0
    c, _ = CA.oracle("tiny")
    with pytest.raises(ValueError):
        coco_eval.flatten_records(c.images, [2, 1], (1, 3))                        # not sorted
    bad = dict(c.images[0], dt_ignore=c.images[0]["dt_ignore"][:, :1])
    with pytest.raises(ValueError):
        coco_eval.flatten_records([bad], [1, 2], (1, 3))


@pytest.mark.parametrize("name", list(CA.CASES))
def test_closed_form_equals_accumulate(name):
    """The host statement of what the kernels compute (one stable sort, the least tp count per recall threshold) against the
    published loop -- on the very cases the GPU test runs, which also shows that the oracle of each takes seconds at most."""
    c, want = CA.oracle(name)
    kw = c.kw
    flat = coco_eval.flatten_records(c.images, kw["classes"], kw["max_dets"])
    precision, recall, npig = coco_eval.accumulate_flat_numpy(flat, len(kw["classes"]), list(kw["max_dets"]), want["rec_thrs"])
    assert precision.shape == want["precision"].shape and np.array_equal(precision, want["precision"])
    assert recall.shape == want["recall"].shape and np.array_equal(recall, want["recall"])
    assert ((npig == 0)[None, :, :, None] == (want["recall"] == -1)).all()


def test_cases_are_sized_from_the_kernel_s_constants():
    src = open(os.path.join(REPO, "mnc_amd", "csrc", "coco_accum.hip")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (kAccum\w+) = (\d+);", src)}
    assert consts["kAccumSortTile"] == coco_eval.ACCUM_SORT_TILE == consts["kAccumThreads"] * consts["kAccumSortItems"]
    assert consts["kAccumScanChunk"] == coco_eval.ACCUM_SCAN_CHUNK == consts["kAccumThreads"] * consts["kAccumScanItems"]
    assert (consts["kAccumMaxK"], consts["kAccumMaxM"], consts["kAccumMaxR"]) == (coco_eval.ACCUM_MAX_K, coco_eval.ACCUM_MAX_M,
                                                                                 coco_eval.ACCUM_MAX_R)
    assert (consts["kAccumMaxT"], consts["kAccumMaxA"], consts["kAccumMaxDet"]) == (coco_eval.MAX_T, coco_eval.MAX_A, coco_eval.MAX_N)
    assert "constexpr int kAccumMaxN = 1 << 24;" in src and coco_eval.ACCUM_MAX_N == 1 << 24
    # (b): a list of three chunks plus one, and classes of 0, 1 and exactly one chunk of detections
    c, _ = CA.oracle("chunks")
    flat = coco_eval.flatten_records(c.images, c.kw["classes"], c.kw["max_dets"])
    assert np.bincount(flat["dt_class_idx"], minlength=4).tolist() == [3 * CA.CHUNK + 1, 1, CA.CHUNK, 0]
    # (c): three tiles plus one key, 8 score levels with both zeros and both infinities, ties across every image
    c, _ = CA.oracle("tiles")
    flat = coco_eval.flatten_records(c.images, c.kw["classes"], c.kw["max_dets"])
    assert len(flat["dt_score"]) == 3 * CA.TILE + 1 and len(c.images) <= 12
    bits = set(flat["dt_score"].view(np.uint32).tolist())
    assert len(bits) == 8 and {0x00000000, 0x80000000, 0x7F800000, 0xFF800000} <= bits
    assert all(len(set(im["dt_scores"].view(np.uint32).tolist())) == 8 for im in c.images)
    # (d): the ranks reach every max_det and pass the largest
    c, want = CA.oracle("empty_cells")
    ranks = np.concatenate([im["rank"] for im in c.images])
    assert all((ranks == m).any() for m in c.kw["max_dets"]) and ranks.max() > max(c.kw["max_dets"])
    assert (want["precision"][:, :, 1] == 0).all() and (want["recall"][:, 1] == 0).all()          # ground truths, no detections
    assert (want["precision"][:, :, 2:] == -1).all() and (want["recall"][:, 2:] == -1).all()     # detections, npig == 0
    assert (want["precision"][:, :, 0] > 0).any()
    # (e)
    c, want = CA.oracle("small_parameters")
    assert want["precision"].shape == (1, 3, 2, 1, 1) and list(c.kw["rec_thrs"]) != sorted(c.kw["rec_thrs"])
    assert CA.oracle("limit_parameters")[1]["precision"].shape == (16, 101, 2, 8, 8)


def _call(flat, k, t, a, max_dets, rec_thrs, null=(), **over):
    """mnc_coco_accumulate as it is, with single arguments replaced -> (the return code, precision, recall, npig)."""
    f = dict(flat)
    f.update({key: np.ascontiguousarray(v, flat[key].dtype) for key, v in over.items() if key in flat})
    md, rt = np.asarray(max_dets, np.int32), np.asarray(rec_thrs, np.float64)
    N, Gn = over.get("N", len(f["dt_class_idx"])), over.get("Gn", len(f["gt_class_idx"]))
    M, R = over.get("M", len(md)), over.get("R", len(rt))
    precision, recall, npig = np.full(1 << 12, 7.0), np.full(1 << 10, 7.0), np.full(1 << 6, 7, np.int64)     # (the tiny case's)
    ptrs = {"precision": _lib.ptr(precision), "recall": _lib.ptr(recall), "npig": _lib.ptr(npig)}
    for key in null:
        ptrs[key] = None
    args = (_lib.ptr(f["dt_class_idx"]), _lib.ptr(f["dt_score"]), _lib.ptr(f["dt_rank"]), _lib.ptr(f["dt_flags"]), N,
            _lib.ptr(f["gt_class_idx"]), _lib.ptr(f["gt_ignore"]), Gn, over.get("K", k), over.get("T", t), over.get("A", a),
            _lib.ptr(md), M, _lib.ptr(rt), R, ptrs["precision"], ptrs["recall"], ptrs["npig"], 0)
    try:
        return _lib.call("mnc_coco_accumulate", *args), precision, recall, npig
    except _lib.MncError as e:
        assert (precision == 7.0).all() and (recall == 7.0).all() and (npig == 7).all()        # refused before anything was written
        return e.code, precision, recall, npig


def test_invalid_arguments_come_back_without_a_gpu():
    c, flat = _flat("tiny")
    K, T, A, md, rt = 2, 2, 1, [1, 3], [0.0, 0.5, 1.0]
    nan = float("nan")

    def rc(max_dets=md, rec_thrs=rt, null=(), **over):
        return _call(flat, K, T, A, max_dets, rec_thrs, null, **over)[0]

    def changed(key, index, value):
        v = flat[key].copy()
        v.reshape(-1)[index] = value
        return {key: v}

    assert rc(N=-1) == INVALID and rc(N=(1 << 24) + 1) == INVALID and rc(Gn=-1) == INVALID and rc(Gn=(1 << 24) + 1) == INVALID
    assert rc(K=0) == INVALID and rc(K=4097) == INVALID and rc(T=0) == INVALID and rc(T=17) == INVALID
    assert rc(A=0) == INVALID and rc(A=9) == INVALID and rc(M=0) == INVALID and rc(M=9) == INVALID
    assert rc(R=0) == INVALID and rc(R=1025) == INVALID
    assert rc(max_dets=[0, 3]) == INVALID and rc(max_dets=[1, 2049]) == INVALID
    assert rc(**changed("dt_class_idx", 3, -2)) == INVALID and rc(**changed("dt_class_idx", 0, K)) == INVALID
    assert rc(**changed("gt_class_idx", 1, -2)) == INVALID and rc(**changed("gt_class_idx", 0, K)) == INVALID
    assert rc(**changed("dt_rank", 2, -1)) == INVALID
    assert rc(**changed("dt_score", 5, nan)) == INVALID and rc(rec_thrs=[0.0, nan, 1.0]) == INVALID
    assert rc(**changed("dt_flags", 7, 4)) == INVALID and rc(**changed("gt_ignore", 2, 2)) == INVALID
    assert rc(null=("precision",)) == INVALID and rc(null=("recall",)) == INVALID
    # the Python surface refuses the same before the call (ValueError), whether or not there is a device
    for kw in ({"max_dets": (0, 3)}, {"max_dets": (1, 2049)}, {"rec_thrs": [nan]}, {"rec_thrs": np.zeros(1025)},
               {"max_dets": tuple(range(1, 10))}, {"iou_thrs": np.linspace(0, 1, 17)}, {"area_rngs": np.zeros((9, 2))}):
        with pytest.raises(ValueError):
            coco_eval.accumulate_device(c.images, **dict(c.kw, **kw))
    bad = dict(c.images[1], dt_scores=np.full(len(c.images[1]["dt_scores"]), nan, np.float32))
    with pytest.raises(ValueError):
        coco_eval.accumulate_device([bad], **c.kw)
    with pytest.raises(ValueError):
        coco_eval.accumulate_device(c.images, **dict(c.kw, classes=range(4097)))


def test_empty_inputs_are_answered_on_the_host():
    """N == 0 and Gn == 0: mnc_coco_accumulate fills the tables as the rule gives, before any device work."""
    c, _ = CA.oracle("tiny")
    kw = c.kw
    no_dt = [dict(im, dt_classes=im["dt_classes"][:0], dt_scores=im["dt_scores"][:0], rank=im["rank"][:0],
                  dt_match=im["dt_match"][:, :, :0], dt_ignore=im["dt_ignore"][:, :, :0]) for im in c.images]
    no_dt[0]["gt_ignore"] = np.where(no_dt[0]["gt_classes"] == 2, 1, no_dt[0]["gt_ignore"]).astype(np.uint8)
    for im in no_dt[1:]:
        im["gt_classes"] = np.where(im["gt_classes"] == 2, 1, im["gt_classes"]).astype(np.int32)     # class 2: npig == 0
    no_gt = [dict(im, gt_classes=im["gt_classes"][:0], gt_ignore=im["gt_ignore"][:, :0]) for im in c.images]
    for images in (no_dt, no_gt, []):
        want = coco_eval.accumulate(images, **kw)
        got = coco_eval.accumulate_device(images, **kw)
        assert list(got) == list(want) or sorted(got) == sorted(want)
        assert np.array_equal(got["precision"], want["precision"]) and np.array_equal(got["recall"], want["recall"])
        assert got["classes"] == want["classes"] and got["max_dets"] == want["max_dets"]
    want = coco_eval.accumulate(no_dt, **kw)
    assert (want["precision"][:, :, 0] == 0).all() and (want["precision"][:, :, 1] == -1).all()
    flat = coco_eval.flatten_records(no_dt, kw["classes"], kw["max_dets"])
    code, _, _, npig = _call(flat, 2, 2, 1, kw["max_dets"], kw["rec_thrs"])
    assert code == 0 and npig[1] == 0 and npig[0] == sum(int(((im["gt_classes"] == 1) & (im["gt_ignore"][0] == 0)).sum()) for im in no_dt)
    # no class at all: accumulate's empty tables
    got = coco_eval.accumulate_device([], classes=[])
    assert got["precision"].shape == (10, 101, 0, 4, 3) and got["recall"].shape == (10, 0, 4, 3)


def test_header_declares_and_library_exports_the_entries():
    decls = _lib.parse_header()
    lib = _lib.load()
    for name, nargs in (("mnc_coco_accumulate", 19), ("mnc_coco_accum_timing", 2)):
        assert name in decls and len(decls[name][1]) == nargs and decls[name][0] is ctypes.c_int
        assert getattr(lib, name) is not None
    assert decls["mnc_coco_accumulate"][2][-4:] == ["precision", "recall", "npig", "device_id"]
    assert decls["mnc_coco_accum_timing"][2] == ["on", "last_ms"]
    last = ctypes.c_double(0.0)
    _lib.call("mnc_coco_accum_timing", 0, ctypes.addressof(last))
    assert last.value == -1.0                                                       # nothing was timed


def test_hand_worked_values_still_come_out_of_the_host_evaluator():
    """The two values of tests/test_mask_match_host.py, through CocoSegmEval(device=False): accumulate_on_device follows `device`,
    so nothing here touches a GPU."""
    g0, g1, none = [10, 10, 19, 19], [100, 40, 109, 49], [50, 0, 59, 4]
    dt, gt = MM.solid([none, g1, g0], [1, 1, 1], [0.8, 0.9, 0.7]), MM.solid([g0, g1], [1, 1])
    ev = CocoSegmEval(device=False)
    assert ev.accumulate_on_device is False and CocoSegmEval(device=False, accumulate_on_device=True).accumulate_on_device is True
    assert CocoSegmEval(device=True).accumulate_on_device is True and CocoSegmEval(accumulate_on_device=False).accumulate_on_device is False
    ev.add("im0", dt, gt, [0, 0])
    assert abs(ev.summarize()["AP"] - 0.834983498349835) < 1e-12
    ev = CocoSegmEval(device=False)
    ev.add(2, dt, gt, [0, 0])
    ev.add(1, MM.solid([[10, 10, 19, 19]], [1], [0.85]), MM.solid([[10, 10, 19, 19]], [1]), [0])
    assert abs(ev.summarize()["AP"] - (67 + 34 * 0.75) / 101) < 1e-12
    # the same tables from the flat arrays by the closed form
    images = [ev._images[i] for i in sorted(ev._images)]
    flat = coco_eval.flatten_records(images, [1], coco_eval.MAX_DETS)
    precision, recall, _ = coco_eval.accumulate_flat_numpy(flat, 1, list(coco_eval.MAX_DETS), coco_eval.REC_THRS)
    assert np.array_equal(precision, ev.eval["precision"]) and np.array_equal(recall, ev.eval["recall"])
