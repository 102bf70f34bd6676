"""COCO-style matching of packed instance masks on the GPU (csrc/mask_match.hip: mnc_mask_match, mnc_mask_match_dev and the Python
surfaces over them) against the numpy statement (mnc_amd.coco_eval.match_numpy, which tests/test_mask_match_host.py pins to
tables written out by hand).  Every comparison of tables is exact.  The sets are those of tests/mask_match_inputs.py: the
hand-made cases, classes whose ground truths span one, two and three chunks of 64 lanes (65, 70, 129; a tie across the chunk
boundary at indices 63 / 64) with 65 and 130 detections, and seeded random sets with crowd and ignore flags."""
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_match_inputs as MM  # noqa: E402
import render_inputs as RI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd.coco_eval import CocoSegmEval, Match, match, match_numpy  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, InstanceBlock, records_from_lists  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

S = RI.S
CHUNKS = [(65, 65), (70, 130), (129, 130)]                # (ground truths, detections) of the class
_WANT = {}


def _want(key, make):
    """The case and its numpy tables, computed once."""
    if key not in _WANT:
        c = make()
        _WANT[key] = (c, match_numpy(c.dt, c.gt, return_iou=True, **c.kw))
    return _WANT[key]


def _same(got, want):
    for f, g, w in zip(Match._fields, got, want):
        if w is None:
            assert g is None, f
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f
    return True


@pytest.mark.parametrize("name", list(MM.hand_cases()))
def test_hand_made_cases_equal_the_numpy_statement(name):
    c, want = _want(name, lambda: MM.hand_cases()[name])
    assert _same(match(c.dt, c.gt, return_iou=True, **c.kw), want)
    assert _same(c.dt.match(c.gt, **c.kw), want._replace(iou=None))
    assert _same(MT.mask_match(c.dt, c.gt, **c.kw), want._replace(iou=None))


@pytest.mark.parametrize("n_gt,n_dt", CHUNKS)
def test_more_than_one_chunk_of_ground_truths(n_gt, n_dt):
    c, want = _want((n_gt, n_dt), lambda: MM.chunk_set(n_gt, n_dt, n_gt))
    assert (c.gt.classes == 1).sum() == n_gt and (c.dt.classes == 1).sum() == n_dt
    assert np.array_equal(c.gt.dense(63), c.gt.dense(64)) and np.array_equal(c.gt.bounds[63], c.gt.bounds[64])
    first = int(np.argsort(want.rank[:2])[0])
    assert want.dt_match[0, 0, first] == 64                                    # the tie goes to the later chunk
    assert (want.dt_match[0, 0] >= 64).sum() > 0 and (want.dt_match[0, 0] >= 0).sum() >= 20
    assert _same(match(c.dt, c.gt, return_iou=True, **c.kw), want)


@pytest.mark.parametrize("seed", MM.RANDOM_SEEDS)
def test_random_sets_equal_the_numpy_statement(seed):
    c, want = _want(seed, lambda: MM.random_set(seed))
    assert want.dt_match.shape == (4, 10, len(c.dt)) and sorted(set(c.dt.classes.tolist())) == [1, 2, 3]
    matches, ignored, unmatched, taken = MM.degenerate(want, c.kw["iscrowd"])
    assert matches >= 20 and ignored >= 5 and unmatched >= 5 and taken > 1
    flagged = (np.asarray(c.kw["iscrowd"]) | np.asarray(c.kw["ignore"])).mean()
    assert 0.1 < flagged < 0.35
    got = match(c.dt, c.gt, return_iou=True, **c.kw)
    assert _same(got, want)
    assert _same(match(c.dt, c.gt, **c.kw), want._replace(iou=None))           # without the IoU output


def test_dirty_padding_changes_nothing():
    seed = MM.RANDOM_SEEDS[0]
    c, want = _want(seed, lambda: MM.random_set(seed))
    d = MM.random_set(seed, dirty=True)
    assert not np.array_equal(d.dt.bits, c.dt.bits) and not np.array_equal(d.gt.bits, c.gt.bits)
    assert np.array_equal(d.dt.areas, c.dt.areas) and np.array_equal(d.gt.areas, c.gt.areas)
    for dt, gt in ((d.dt, d.gt), (d.dt, c.gt), (c.dt, d.gt)):
        assert _same(match(dt, gt, return_iou=True, **c.kw), want)


def test_other_parameters():
    """One threshold and range, sixteen thresholds and eight ranges, thresholds at and past 1, max_det below the class's count."""
    seed = MM.RANDOM_SEEDS[1]
    c = MM.random_set(seed, n_dt=40, n_gt=20)
    for kw in ({"iou_thrs": [0.3], "area_rngs": [[0, 1e10]]},
               {"iou_thrs": np.linspace(0.0, 1.5, 16), "area_rngs": [[0, 100 * (k + 1)] for k in range(8)], "max_det": 5},
               {"iou_thrs": [1.0, 0.999], "area_rngs": [[50, 50], [0, 0]], "max_det": 1}):
        kw = dict(c.kw, **kw)
        assert _same(match(c.dt, c.gt, return_iou=True, **kw), match_numpy(c.dt, c.gt, return_iou=True, **kw))


def _block(rec, counts, cap):
    """A device instance block holding `rec`, as the voting leaves it -> (InstanceBlock, its context)."""
    from mnc_amd.engine import _Ctx
    ctx = _Ctx(0)
    blk = InstanceBlock(types.SimpleNamespace(_ctx=ctx), 21, S, 100, 300)
    assert blk.rows_cap >= cap
    head = np.zeros(HEAD_BYTES // 4, np.int32)
    head[:len(counts)] = counts
    raw = np.concatenate((head.view(np.uint8), np.ascontiguousarray(rec).reshape(-1).view(np.uint8)))
    _lib.call("mnc_h2d", ctx.h, blk.ptr, _lib.ptr(raw), raw.nbytes)
    return blk, ctx


def test_device_entry_equals_the_host_entry():
    rng = np.random.default_rng(71)
    h, w = 70, 200
    list_mask, list_box = RI.class_lists(rng, w, h, 0.5)
    cap = 200
    rec, total = records_from_lists(list_mask, list_box, cap, S)
    assert 3 < total < cap
    rec[1, 4] = rec[0, 4]                                                      # a score tie
    counts = [total] + [len(b) for b in list_box]
    blk, ctx = _block(rec, counts, cap)
    try:
        view = blk.view()
        pm = view.masks(h, w, score_thresh=0.0)
        assert "bits" not in pm._host and pm._device() is not None            # device-resident
        host = view.masks(h, w, score_thresh=0.0).fetch()                     # the same image once more, copied
        flat = PackedMasks(**host.arrays())                                    # host arrays alone: the host entry
        n = len(flat)
        # ground truths: every other instance itself, one of them a crowd, one ignored, and the edge set's masks
        idx = np.arange(0, n, 2)
        own = flat.take(idx)
        other = MM.MI.edge_sets()[1]
        gt = MM.MI.pack(own.bounds.tolist() + other.bounds.tolist(), [own.dense(i) for i in range(len(own))] +
                        [other.dense(j) for j in range(len(other))], own.classes.tolist() + [int(flat.classes[0])] * len(other))
        crowd, ignore = np.zeros(len(gt), np.uint8), np.zeros(len(gt), np.uint8)
        crowd[1], ignore[2], crowd[len(own) + 10] = 1, 1, 1
        kw = {"iscrowd": crowd, "ignore": ignore, "area_rngs": [[0, 1e10], [0, 300], [300, 1e10]]}
        with pytest.raises(RuntimeError):
            pm.match(gt, **kw)                                                 # the second masks() made the first result stale
        pm = view.masks(h, w, score_thresh=0.0)
        want = match(flat, gt, return_iou=True, **kw)
        assert _same(want, match_numpy(flat, gt, return_iou=True, **kw))
        assert (want.dt_match[0, 0] >= 0).sum() >= len(idx) // 2 and want.dt_ignore.sum() >= 2
        got = pm.match(gt, return_iou=True, **kw)
        assert "bits" not in pm._host and _same(got, want)
        assert _same(pm.match(gt, **kw), want._replace(iou=None))
        none = MM.solid([])
        assert _same(pm.match(none, **dict(kw, iscrowd=[], ignore=[])), match_numpy(flat, none, [], area_rngs=kw["area_rngs"]))
        # the masks the _dev entry reads are as they were; a fetched result that is still current goes on using the device
        assert all(np.array_equal(getattr(pm.fetch(), f), getattr(host, f)) for f in PackedMasks.FIELDS)
        assert _same(host.match(gt, **kw), want._replace(iou=None))
    finally:
        blk.release()
        ctx.close()


def test_evaluator_on_the_device_equals_the_host_s():
    dev, cpu = CocoSegmEval(device=True), CocoSegmEval(device=False)
    sets = [MM.random_set(s, n_dt=40, n_gt=16) for s in MM.RANDOM_SEEDS] + [MM.chunk_set(65, 65, 65)]
    for i, c in enumerate(sets):
        for ev in (dev, cpu):
            ev.add(i, c.dt, c.gt, c.kw["iscrowd"], c.kw["ignore"], c.kw.get("eval_area"))
    dev.summarize()
    cpu.summarize()
    assert dev.stats.dtype == np.float64 and dev.stats.shape == (12,) and np.array_equal(dev.stats, cpu.stats)
    assert np.array_equal(dev.eval["precision"], cpu.eval["precision"]) and np.array_equal(dev.eval["recall"], cpu.eval["recall"])
    assert 0 < cpu.stats[0] < 1 and cpu.stats[6] < cpu.stats[8]
