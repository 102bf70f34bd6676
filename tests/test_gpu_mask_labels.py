"""Label maps in and out of packed masks on the GPU (csrc/mask_labels.hip: mnc_label_table, mnc_label_masks, mnc_mask_to_labels and the
Python surfaces over them) against the numpy statements (mnc_amd.labels.from_labels_numpy and to_labels_numpy, which
tests/test_mask_labels_host.py pins to scipy, np.bincount, parse_inst and the painting loop).  Every comparison is exact, field by
field, dtype and shape included.  The maps and sets are those of tests/mask_labels_inputs.py: the smallest at which a kernel can go
wrong."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_algebra_inputs as AI  # noqa: E402
import mask_labels_inputs as LI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import labels as LB  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY = np.uint64(0x5555555555555555)
CANARY32 = np.int32(0x55555555)


def same_result(got, want):
    (gp, gi), (wp, wi) = got, want
    assert gi.dtype == wi.dtype == np.int32 and gi.shape == wi.shape and np.array_equal(gi, wi)
    return AI.same_masks(gp, wp)


def same_map(got, want):
    assert got.dtype == want.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    return True


# ---- from_labels ----

@pytest.mark.parametrize("name", sorted(LI.MAPS))
def test_from_labels_equals_the_statement(name):
    """Widths 1, 63, 64, 65, 130 and heights 1, 2, 65; boxes that start at columns 0, 1, 63, 64, 65; runs of length one, a run that
    fills a 130-wide row, single pixels; ids 31 / 32 / 33, 32767 / 32768 / 40000 and 2^24 - 1; exactly 2048 labels; a window of the
    engineered superpixel image; the map of the 300 blobs."""
    label = LI.get(name)
    got = PackedMasks.from_labels(label)
    assert same_result(got, LI.from_ref(name)) and AI.canonical(got[0])
    if name == "labels_2048":
        assert len(got[0]) == 2048 and got[1][-1] == 2048 and tuple(got[0].bounds[-1]) == (62, 63, 63, 63) and got[0].areas[-1] == 2
    if name == "top_id":
        assert got[1][-1] == LI.TOP_ID


def test_other_dtypes_and_the_host_array_form():
    label = LI.get("box_edges")
    for dtype in (np.uint8, np.uint16, np.int64):
        assert same_result(LB.from_labels(label.astype(dtype)), LI.from_ref("box_edges"))
    assert same_result(MT.masks_from_labels(label), LI.from_ref("box_edges"))
    assert same_map(MT.mask_labels(LI.from_ref("box_edges")[0], 12, 200), MT.mask_labels_numpy(LI.from_ref("box_edges")[0], 12, 200))


def test_maps_with_no_instance_and_the_background_forms():
    zeros = np.zeros((3, 70), np.int32)
    pm, ids = PackedMasks.from_labels(zeros)
    assert len(pm) == 0 and ids.shape == (0,) and ids.dtype == np.int32 and pm.bits.size == 0
    assert same_result((pm, ids), LB.from_labels_numpy(zeros))
    label = LI.get("full_row")
    assert same_result(PackedMasks.from_labels(label, background=None), LB.from_labels_numpy(label, background=None))
    assert same_result(PackedMasks.from_labels(zeros, background=None), LB.from_labels_numpy(zeros, background=None))
    voc = label.copy()
    voc[0, :5] = 255
    voc[3, 129] = 255
    got = PackedMasks.from_labels(voc, background=(0, 255))
    assert 255 not in got[1] and same_result(got, LB.from_labels_numpy(voc, background=(0, 255)))
    assert same_result(PackedMasks.from_labels(label, background=(0, 255, 9999, 2 ** 24 - 1)), LI.from_ref("full_row"))
    only = np.full((2, 65), 255, np.int32)
    assert len(PackedMasks.from_labels(only, background=(0, 255))[0]) == 0


def test_more_than_2048_labels_are_refused_with_their_count():
    for name, count in (("labels_2049", 2049), ("superpixels", LI.SUPERPIXEL_LABELS)):
        label = LI.get(name)
        with pytest.raises(ValueError, match="%d instances" % count):
            PackedMasks.from_labels(label)
        cap = 2048
        ids, bounds, areas = np.full(cap, CANARY32), np.full((cap, 4), CANARY32), np.full(cap, 0x5555555555555555, np.int64)
        lo, hi = np.full(cap, CANARY32), np.full(cap, CANARY32)
        n, need, skip = ctypes.c_int(-1), ctypes.c_size_t(77), np.zeros(1, np.int32)
        with pytest.raises(_lib.MncError) as e:
            _lib.call("mnc_label_table", _lib.ptr(label), None, label.shape[0], label.shape[1], _lib.ptr(skip), 1, cap,
                      ctypes.addressof(n), _lib.ptr(ids), _lib.ptr(bounds), _lib.ptr(areas), _lib.ptr(lo), _lib.ptr(hi),
                      ctypes.addressof(need), 0)
        assert e.value.code == INVALID and n.value == count and need.value == 77
        for a in (ids, bounds, lo, hi):
            assert (a == CANARY32).all()
        assert (areas == 0x5555555555555555).all()
    # a smaller cap refuses a map that 2048 would take, the same way
    label = LI.get("box_edges")
    with pytest.raises(ValueError, match="7 instances"):
        LB.label_table(np.ascontiguousarray(label), None, (0,), cap=6)
    assert LB.label_table(np.ascontiguousarray(label), None, (0,), cap=7)[0] == 7


def test_classes():
    inst, cls = LI.class_maps()
    assert same_result(PackedMasks.from_labels(inst, cls), LB.from_labels_numpy(inst, cls))
    assert same_result(PackedMasks.from_labels(inst, cls=cls.astype(np.uint8)), LB.from_labels_numpy(inst, cls))
    inst, mixed, first = LI.mixed_class_maps()
    with pytest.raises(ValueError, match="instance %d has" % first):
        PackedMasks.from_labels(inst, mixed)
    ids = LB.from_labels_numpy(inst)[1]
    table = {int(i): int(i) * 3 - 50 for i in ids}
    assert same_result(PackedMasks.from_labels(inst, classes=table), LB.from_labels_numpy(inst, classes=table))
    del table[int(ids[0])]
    with pytest.raises(ValueError, match="no entry for id %d" % ids[0]):
        PackedMasks.from_labels(inst, classes=table)
    from utils.voc_eval import parse_inst_maps
    inst, cls = LI.class_maps()
    for g, w in zip(parse_inst_maps(inst, cls, on_device=True), parse_inst_maps(inst, cls)):
        assert all(np.array_equal(g[k], w[k]) and np.asarray(g[k]).dtype == np.asarray(w[k]).dtype for k in w)


def test_values_outside_the_range_are_refused():
    bad = np.zeros((2, 3), np.int64)
    for v in (2 ** 24, -1, 2 ** 32 + 5):
        bad[1, 2] = v
        with pytest.raises(ValueError):
            PackedMasks.from_labels(bad)
    bad32 = np.zeros((2, 3), np.int32)
    bad32[1, 2] = 2 ** 24
    with pytest.raises(ValueError, match=r"label\[1\]\[2\]"):
        PackedMasks.from_labels(bad32)


# ---- the raw entries ----

def _table(label):
    return LB.label_table(np.ascontiguousarray(label, np.int32), None, (0,))


def _masks_call(label, ids, bounds, bits, cap, used):
    return _lib.call("mnc_label_masks", _lib.ptr(label), label.shape[0], label.shape[1], _lib.ptr(ids), _lib.ptr(bounds), len(ids),
                     _lib.ptr(bits), cap, ctypes.addressof(used), 0)


def test_label_masks_room_canaries_and_null_pointers():
    label = np.ascontiguousarray(LI.get("box_edges"))
    n, ids, bounds, areas, lo, hi, need = _table(label)
    want = LI.from_ref("box_edges")[0]
    assert n == len(want) and need == want.bits.nbytes and np.array_equal(areas, want.areas) and not lo.any() and not hi.any()
    bits = np.full(need // 8 + 16, CANARY, np.uint64)
    used = ctypes.c_size_t(5)
    with pytest.raises(_lib.MncError) as e:
        _masks_call(label, ids, bounds, bits, need - 8, used)
    assert e.value.code == INVALID and "bits_cap" in str(e.value) and (bits == CANARY).all()
    _masks_call(label, ids, bounds, bits, need, used)
    assert used.value == need and np.array_equal(bits[:need // 8], want.bits) and (bits[need // 8:] == CANARY).all()
    for args in ((None, ids, bounds, bits), (label, None, bounds, bits), (label, ids, None, bits), (label, ids, bounds, None)):
        with pytest.raises(_lib.MncError) as e:
            _lib.call("mnc_label_masks", _lib.ptr(args[0]), 12, 200, _lib.ptr(args[1]), _lib.ptr(args[2]), n, _lib.ptr(args[3]), need,
                      ctypes.addressof(used), 0)
        assert e.value.code == INVALID
    with pytest.raises(_lib.MncError):
        _lib.call("mnc_label_masks", _lib.ptr(label), 12, 200, _lib.ptr(ids), _lib.ptr(bounds), n, _lib.ptr(bits), need, None, 0)
    out = np.zeros(4, np.int32)
    z = ctypes.c_int(0)
    for args in ((None, ctypes.addressof(z), ctypes.addressof(used)), (_lib.ptr(label), None, ctypes.addressof(used)),
                 (_lib.ptr(label), ctypes.addressof(z), None)):
        with pytest.raises(_lib.MncError) as e:
            _lib.call("mnc_label_table", args[0], None, 12, 200, None, 0, 4, args[1], _lib.ptr(out), _lib.ptr(out), _lib.ptr(out),
                      _lib.ptr(out), _lib.ptr(out), args[2], 0)
        assert e.value.code == INVALID
    with pytest.raises(_lib.MncError):
        _lib.call("mnc_mask_to_labels", *(_set_args(want, areas=False) + (_lib.ptr(want.scores), None, None, 0, 12, 200, None, 0)))
    # a table that does not belong to the map: ids out of order, a box that leaves the image
    for bad_ids, bad_bounds in ((ids[::-1].copy(), bounds), (ids, np.concatenate((bounds[:-1], [[0, 0, 200, 3]])).astype(np.int32))):
        with pytest.raises(_lib.MncError) as e:
            _masks_call(label, bad_ids, bad_bounds, bits, bits.nbytes, used)
        assert e.value.code == INVALID
    # ids that the map does not hold, and boxes smaller than the instances: nothing outside the rows is written
    small = bounds.copy()
    small[:, 2] = np.minimum(small[:, 0] + 2, bounds[:, 2])
    odd = ids.copy() + 100
    for t_ids, t_bounds in ((odd, bounds), (ids, small)):
        bits[:] = CANARY
        _masks_call(label, t_ids, t_bounds, bits, bits.nbytes, used)
        assert (bits[used.value // 8:] == CANARY).all()
        got = PackedMasks(t_bounds, np.cumsum([0] + [8 * (int(b[3]) - int(b[1]) + 1) * ((int(b[2]) - int(b[0])) // 64 + 1)
                                                     for b in t_bounds])[:-1], np.zeros(n), None, None, bits[:used.value // 8])
        for k in range(n):
            x1, y1, x2, y2 = (int(v) for v in t_bounds[k])
            assert np.array_equal(got.dense(k), label[y1:y2 + 1, x1:x2 + 1] == t_ids[k])


# ---- to_labels ----

@pytest.mark.parametrize("name", sorted(LI.sets()))
def test_to_labels_equals_the_statement(name):
    """Equal scores, the nested stacks in both orders, 1025 small instances (17 rounds of 64), no instance, dirty padding bits,
    negative bounds; default and explicit order, default values, classes, negative values and 2^31 - 1, a non-zero background."""
    pm, H, W = LI.sets()[name]
    n = len(pm)
    rng = np.random.default_rng(11)
    assert same_map(pm.to_labels(H, W), LI.to_ref(name, pm, H, W))
    assert same_map(pm.to_labels(H, W, values=pm.classes, background=-7), LI.to_ref(name, pm, H, W, pm.classes, None, -7))
    values = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    if n:
        values[0], values[-1] = 2 ** 31 - 1, -2 ** 31
    order = rng.permutation(n).astype(np.int32)
    assert same_map(pm.to_labels(H, W, values, order, 2 ** 31 - 1), LI.to_ref(name, pm, H, W, values, order, 2 ** 31 - 1))
    assert same_map(pm.to_labels(H, W, order=np.arange(n)[::-1]), LI.to_ref(name, pm, H, W, None, np.arange(n)[::-1]))


@pytest.mark.parametrize("size", [(37, 5), (3, 65), (1, 1), (70, 64)])
def test_to_labels_of_narrow_and_odd_images(size):
    H, W = size
    for name in ("word_dirty", "negative", "equal"):
        pm = LI.sets()[name][0]
        assert same_map(pm.to_labels(H, W, background=4), LI.to_ref(name, pm, H, W, None, None, 4))


def test_to_labels_writes_nothing_past_the_map_and_checks_its_arguments():
    pm, H, W = LI.sets()["equal"]
    out = np.full((H + 1, W), CANARY32, np.int32)
    _lib.call("mnc_mask_to_labels", *(_set_args(pm, areas=False) + (_lib.ptr(pm.scores), None, None, 0, H, W, _lib.ptr(out), 0)))
    assert np.array_equal(out[:H], LI.to_ref("equal", pm, H, W)) and (out[H] == CANARY32).all()
    empty = AI.get("empty")
    out[:] = CANARY32
    _lib.call("mnc_mask_to_labels", *(_set_args(empty, areas=False) + (None, None, None, -9, H, W, _lib.ptr(out), 0)))
    assert (out[:H] == -9).all() and (out[H] == CANARY32).all()
    for kw in ({"order": [0, 0, 1, 2, 3, 4, 5, 6]}, {"order": [0, 1, 2]}, {"values": [1, 2, 3]}, {"background": 2 ** 31}):
        with pytest.raises((ValueError, _lib.MncError)):
            pm.to_labels(H, W, **kw)
    with pytest.raises(ValueError):
        pm.to_labels(0, W)
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_mask_to_labels", *(_set_args(pm, areas=False) + (None, None, None, 0, H, W, _lib.ptr(out), 0)))
    assert e.value.code == INVALID


# ---- round trips and run to run ----

def test_round_trips_on_the_device():
    pm = AI.get("blobs")
    H, W = LI.BLOBS_SIZE
    seg = pm.to_labels(H, W)
    assert same_map(seg, LI.get("blobs"))
    got, ids = PackedMasks.from_labels(seg, classes={i + 1: int(c) for i, c in enumerate(pm.classes)})
    cut = pm.layered().crop(0, 0, W - 1, H - 1)                  # the existing kernels on the other side
    kept = np.nonzero(cut.areas > 0)[0]
    want = cut.take(kept)
    assert len(kept) == LI.SURVIVORS["blobs"] and np.array_equal(ids, kept + 1)
    for f in ("bounds", "offsets", "areas", "classes", "bits"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
    assert np.array_equal(np.bincount(seg.reshape(-1), minlength=len(pm) + 1)[1:], cut.areas)
    # and back: the map of the instances of a map is the map
    back = got.to_labels(H, W, values=ids, order=np.arange(len(got)))
    assert same_map(back, seg)


def test_run_to_run():
    label = np.ascontiguousarray(LI.get("blobs"))
    a, b = _table(label), _table(label)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
    n, ids, bounds, _, _, _, need = a
    assert LB.label_masks(label, ids, bounds, need).tobytes() == LB.label_masks(label, ids, bounds, need).tobytes()
    pm = AI.get("blobs")
    assert pm.to_labels(*LI.BLOBS_SIZE).tobytes() == pm.to_labels(*LI.BLOBS_SIZE).tobytes()


def test_timing_hook():
    label = np.ascontiguousarray(LI.get("blobs"))
    LB.timing(True)
    _table(label)
    assert LB.timing(False) > 0.0
    pm = AI.get("equal")
    LB.timing(True)
    pm.to_labels(AI.IMAGE_H, AI.IMAGE_W)
    assert LB.timing(False) > 0.0
