"""Mask IoU between packed instance masks and the mask NMS on the GPU (csrc/mask_overlaps.hip: mnc_mask_overlaps,
mnc_mask_overlaps_dev, mnc_mask_nms, mnc_mask_nms_dev and the Python surfaces over them) against the numpy statements
(mask_overlaps_numpy, mask_nms_numpy, which tests/test_mask_overlaps_host.py pins to the reference's mask_overlap and to a painted
canvas).  Every comparison is exact.  The sets are small -- a 70 x 200 frame, at most about 40 instances a set -- and placed
where the kernel can go wrong: widths 1, 63, 64, 65, 128, 129, every residue of the horizontal offset between two bounds in
{0, 1, 31, 63} with both signs, bounds inside one another, sharing one row / column / pixel, adjacent, negative and past the frame,
all-zero and identical masks, an instance without rows, dirty padding."""
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_overlap_inputs as MI  # noqa: E402
import render_inputs as RI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, InstanceBlock, records_from_lists  # noqa: E402
from mnc_amd.masks import PackedMasks, mask_nms, mask_overlaps  # noqa: E402
from transform import mask_transform as MT  # noqa: E402
from transform.mask_transform import mask_nms_numpy, mask_overlaps_numpy  # noqa: E402

pytestmark = pytest.mark.gpu

S = RI.S
THRESHOLDS = [0.0, 0.3, 1.0]


@pytest.fixture(scope="module")
def edge():
    a, b = MI.edge_sets()
    return a, b, mask_overlaps_numpy(a, b)


def _equal(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    return True


def test_offsets_cover_every_residue_and_sign():
    ba, bb = MI.edge_boxes()
    d = {(a[0] - b[0]) for a in ba[:6] for b in bb[:27]}
    assert {x % 64 for x in d} >= {0, 1, 31, 63} and min(d) < 0 < max(d)
    assert sorted({a[2] - a[0] + 1 for a in ba[:6]}) == MI.WIDTHS


def test_host_entry_equals_the_numpy_statement(edge):
    a, b, want = edge
    got = mask_overlaps(a, b)
    assert _equal(got, want)
    assert _equal(MT.mask_overlaps(b, a), (want[0].T.copy(), want[1].T.copy()))            # the roles exchanged
    assert (want[0] > 0).sum() > 100 and (want[1] == 1.0).sum() >= 3 and (want[0] == 0).sum() > 100


def test_b_none_equals_a_twice(edge):
    a = edge[0]
    want = mask_overlaps_numpy(a)
    assert _equal(mask_overlaps(a), want) and _equal(mask_overlaps(a, a), want) and _equal(mask_overlaps(a, a.take(range(len(a)))), want)
    assert _equal(a.overlaps(), want)


def test_dirty_padding_is_not_counted(edge):
    a, b, want = edge
    da, db = MI.edge_sets(dirty=True)
    assert not np.array_equal(da.bits, a.bits) and np.array_equal(da.areas, a.areas)
    assert _equal(mask_overlaps(da, db), want) and _equal(mask_overlaps(da, b), want) and _equal(mask_overlaps(a, db), want)
    assert _equal(mask_overlaps(da), mask_overlaps_numpy(a))


def test_one_output_alone_and_empty_sets(edge):
    a, b, want = edge
    inter = np.zeros(want[0].shape, np.int64)
    iou = np.zeros(want[1].shape, np.float64)
    from mnc_amd.masks import _set_args
    _lib.call("mnc_mask_overlaps", *(_set_args(a) + _set_args(b) + (_lib.ptr(inter), None, 0)))
    _lib.call("mnc_mask_overlaps", *(_set_args(a) + _set_args(b) + (None, _lib.ptr(iou), 0)))
    assert _equal((inter, iou), want)
    none = MI.pack([], [])
    for x, y in ((none, b), (a, none), (none, none)):
        got = mask_overlaps(x, y)
        assert got[0].shape == got[1].shape == (len(x), len(y)) and got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert mask_overlaps(none)[0].shape == (0, 0) and mask_nms(none, 0.5).shape == (0,)


def test_many_pairs_and_a_large_instance():
    rng = np.random.default_rng(61)
    n = 90
    x = np.sort(rng.integers(-20, 620, (n, 2)), 1)
    y = np.sort(rng.integers(-20, 420, (n, 2)), 1)
    bounds = [[int(x[i, 0]), int(y[i, 0]), int(x[i, 1]), int(y[i, 1])] for i in range(n)]
    bounds[0] = [-20, -20, 619, 419]
    pm = MI.pack(bounds, [MI._random_dense(rng, b) for b in bounds], rng.integers(1, 21, n), rng.uniform(0, 1, n))
    want = mask_overlaps_numpy(pm)
    assert _equal(mask_overlaps(pm), want)
    assert want[0].max() > 2 ** 15


_NMS_SETS = {}


def _nms_set(name):
    if not _NMS_SETS:
        _NMS_SETS.update(MI.nms_cases())
        _NMS_SETS["crowded"] = MI.crowded_set()
        _NMS_SETS["edge"] = MI.edge_sets()[0]
    return _NMS_SETS[name]


_NMS_WANT = {}


def _nms_want(name, thresh, class_aware):
    key = (name, thresh, class_aware)
    if key not in _NMS_WANT:
        _NMS_WANT[key] = mask_nms_numpy(_nms_set(name), thresh, class_aware)
    return _NMS_WANT[key]


@pytest.mark.parametrize("class_aware", [False, True])
@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("name", ["three_identical", "tie", "half", "classes", "crowded", "edge"])
def test_mask_nms_equals_the_numpy_statement(name, thresh, class_aware):
    pm = _nms_set(name)
    want = _nms_want(name, thresh, class_aware)
    got = mask_nms(pm, thresh, class_aware)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(pm.nms(thresh, class_aware), want) and np.array_equal(MT.mask_nms(pm, thresh, class_aware), want)
    kept = pm.take(got)
    assert len(kept) == len(want) and np.array_equal(kept.scores, pm.scores[want])


def test_mask_nms_threshold_edge_and_counts():
    half = _nms_set("half")
    below = float(np.nextafter(0.5, 0.0))
    assert mask_nms(half, 0.5).tolist() == [0, 1] and mask_nms(half, below).tolist() == [0]
    crowded = _nms_set("crowded")
    blind, aware = _nms_want("crowded", 0.3, False), _nms_want("crowded", 0.3, True)
    assert 1 < len(blind) < len(aware) < len(crowded)                          # the case does suppress, and classes matter
    assert len(_nms_want("crowded", 1.0, False)) == len(crowded)


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


def _same(got, want):
    return all(np.array_equal(getattr(got, f), getattr(want, f)) for f in PackedMasks.FIELDS)


@pytest.mark.parametrize("score_thresh", [0.0, 0.5])
def test_device_entries_equal_the_host_entries(score_thresh, edge):
    rng = np.random.default_rng(71)
    h, w = 70, 200
    list_mask, list_box = RI.class_lists(rng, w, h, 0.5)
    cap = 200
    rec, total = records_from_lists(list_mask, list_box, cap, S)
    assert 3 < total < cap
    above = np.where(rec[:total, 4] >= 0.5)[0]
    rec[above[1], 0], rec[above[1], 2] = 60.0, 30.0                            # x2 < x1: an instance without rows
    rec[above[2], 4] = rec[above[0], 4]                                        # a score tie
    counts = [total] + [len(b) for b in list_box]
    blk, ctx = _block(rec, counts, cap)
    try:
        view = blk.view()
        pm = view.masks(h, w, score_thresh=score_thresh)
        assert "bits" not in pm._host and pm._device() is not None            # device-resident
        host = view.masks(h, w, score_thresh=score_thresh).fetch()            # the same image once more, copied
        assert host is not pm
        with pytest.raises(RuntimeError):
            pm.overlaps()                                                      # ... which made the first result stale
        with pytest.raises(RuntimeError):
            pm.nms(0.5)
        pm = view.masks(h, w, score_thresh=score_thresh)
        n = len(host)
        assert 3 < n <= total and min(host.size(i)[1] for i in range(n)) == 0
        flat = PackedMasks(**host.arrays())                                    # host arrays alone: the host entries
        want_self = mask_overlaps(flat)
        assert _equal(want_self, mask_overlaps_numpy(flat))
        got_self = pm.overlaps()
        assert "bits" not in pm._host and _equal(got_self, want_self)
        assert want_self[0].shape == (n, n) and (want_self[0] > 0).sum() > n
        b = edge[1]
        want_b = mask_overlaps(flat, b)
        assert _equal(pm.overlaps(b), want_b) and (want_b[0] > 0).sum() > 10
        assert _equal(pm.overlaps(MI.pack([], [])), (np.zeros((n, 0), np.int64), np.zeros((n, 0), np.float64)))
        for thresh in THRESHOLDS:
            for class_aware in (False, True):
                want = mask_nms_numpy(flat, thresh, class_aware)
                assert np.array_equal(mask_nms(flat, thresh, class_aware), want)
                got = pm.nms(thresh, class_aware)
                assert got.dtype == np.int32 and np.array_equal(got, want), (thresh, class_aware)
        assert "bits" not in pm._host
        # the masks the _dev entries read are as they were
        assert _same(pm.fetch(), host) and _same(view.masks(h, w, score_thresh=score_thresh), host)
        # a fetched result that is still current goes on using the device; one that is stale, its host arrays
        assert _equal(host.overlaps(), want_self) and np.array_equal(host.nms(0.3), mask_nms_numpy(flat, 0.3))
    finally:
        blk.release()
        ctx.close()
