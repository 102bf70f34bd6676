"""COCO's accumulate in one device call (csrc/coco_accum.hip: mnc_coco_accumulate; mnc_amd.coco_eval.accumulate_device and
CocoSegmEval over it) against the published loop on the host (mnc_amd.coco_eval.accumulate) on the same records.  Every
comparison is np.array_equal on precision and recall: equality to the bit is the claim, there is no tolerance.  The cases are
those of tests/coco_accum_inputs.py, sized from the kernel's own constants; tests/test_coco_accum_host.py shows without a GPU that
they are what they say."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import coco_accum_inputs as CA  # noqa: E402  (sets up the import paths)
import mask_match_inputs as MM  # noqa: E402
from mnc_amd import coco_eval  # noqa: E402
from mnc_amd.coco_eval import CocoSegmEval  # noqa: E402

pytestmark = pytest.mark.gpu


def same_tables(got, want):
    assert got["precision"].shape == want["precision"].shape and got["recall"].shape == want["recall"].shape
    assert got["precision"].dtype == want["precision"].dtype == np.float64 and got["recall"].dtype == np.float64
    assert np.array_equal(got["recall"], want["recall"])
    assert np.array_equal(got["precision"], want["precision"])
    assert got["classes"] == want["classes"] and got["max_dets"] == want["max_dets"]
    for key in ("iou_thrs", "area_rngs", "rec_thrs"):
        assert np.array_equal(got[key], want[key]), key
    return True


@pytest.mark.parametrize("name", list(CA.CASES))
def test_device_tables_equal_the_host_loop_s(name):
    """(a) tiny, (b) chunks, (c) tiles, (d) empty_cells, (e) small_parameters and limit_parameters."""
    c, want = CA.oracle(name)
    assert same_tables(coco_eval.accumulate_device(c.images, **c.kw), want)


def test_tiny_case_by_eye():
    """(a) once more with the numbers in sight: 3 images, 2 classes, T = 2, one area range, max_dets 1 and 3."""
    c, want = CA.oracle("tiny")
    got = coco_eval.accumulate_device(c.images, **c.kw)
    assert got["precision"].shape == (2, 5, 2, 1, 2) and got["recall"].shape == (2, 2, 1, 2)
    assert got["recall"].tolist() == want["recall"].tolist() and got["precision"].tolist() == want["precision"].tolist()
    assert (got["recall"] >= 0).all() and got["recall"].max() > 0


def test_ranks_at_and_above_every_max_det_inside_the_kernel():
    """(d) accumulate_device leaves out the detections no list holds; here they all go in (flattened with the limit 2048) and the
    kernel's own comparison with each max_det has to drop them.  npig comes back too."""
    c, want = CA.oracle("empty_cells")
    flat = coco_eval.flatten_records(c.images, c.kw["classes"], (2048,))
    assert (flat["dt_rank"] >= max(c.kw["max_dets"])).any()
    precision, recall, npig = coco_eval.accumulate_flat(flat, len(c.kw["classes"]), c.kw["max_dets"], want["rec_thrs"])
    assert np.array_equal(precision, want["precision"]) and np.array_equal(recall, want["recall"])
    assert ((npig == 0)[None, :, :, None] == (want["recall"] == -1)).all() and npig[0].min() > 0 and (npig[2:] == 0).all()


def test_unsorted_and_repeated_classes_come_back_in_the_caller_s_order():
    c, _ = CA.oracle("empty_cells")
    kw = dict(c.kw, classes=[7, 1, 5, 1])
    assert same_tables(coco_eval.accumulate_device(c.images, **kw), coco_eval.accumulate(c.images, **kw))


def test_same_input_twice_gives_identical_bytes():
    """(f) on the case whose tie groups cross every tile: no result depends on the order in which anything arrived."""
    c, want = CA.oracle("tiles")
    first = coco_eval.accumulate_device(c.images, **c.kw)
    second = coco_eval.accumulate_device(c.images, **c.kw)
    assert first["precision"].tobytes() == second["precision"].tobytes() and first["recall"].tobytes() == second["recall"].tobytes()
    assert first["precision"].tobytes() == want["precision"].tobytes()


def test_evaluator_on_masks_gives_the_host_evaluator_s_stats():
    """(g) CocoSegmEval(device=True) -- matching and accumulation on the GPU -- on the masks of mask_match_inputs.random_set."""
    dev, host, mixed = CocoSegmEval(device=True), CocoSegmEval(device=False), CocoSegmEval(device=False, accumulate_on_device=True)
    assert dev.accumulate_on_device and not host.accumulate_on_device
    for seed in MM.RANDOM_SEEDS:
        s = MM.random_set(seed)
        for ev in (dev, host, mixed):
            ev.add(seed, s.dt, s.gt, s.kw["iscrowd"], s.kw["ignore"], s.kw["eval_area"])
    want = host.summarize()
    for ev in (dev, mixed):
        got = ev.summarize()
        assert list(got) == list(want) and list(got.values()) == list(want.values())
        assert np.array_equal(ev.stats, host.stats) and same_tables(ev.eval, host.eval)
    assert 0 < want["AP"] < 1
