"""The squared Euclidean distance transform, the inscribed disc and the morphology by a disc of packed instance masks on the GPU
(csrc/mask_distance.hip: mnc_mask_distance, mnc_mask_inscribed, mnc_mask_morph and the Python surfaces over them) against the numpy
statements (mnc_amd.distance.distance_numpy, inscribed_numpy, morph_numpy, which tests/test_mask_distance_host.py pins to scipy, to
a brute force and to closed forms).  Every comparison is exact, field by field, dtype and shape included.  The sets are those of
tests/mask_distance_inputs.py; that the word-boundary set can fail (a quarter of its instances keep a pixel after the erosion, a
quarter change under the opening) is asserted of the numpy statement in the host test."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import mask_distance_inputs as DI  # noqa: E402
import render_inputs as RI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import distance as DT  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, InstanceBlock, records_from_lists  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY = np.uint64(0x5555555555555555)


def _maps(name):
    got = DT.distance(DI.get(name))
    assert DI.same_arrays(got, DI.reference(name, "distance"))
    return got


def _discs(name):
    got = DT.inscribed(DI.get(name))
    assert DI.same_arrays(got, DI.reference(name, "inscribed"))
    return got


def _morph(name, op, r2, H=None, W=None):
    got = DT.morph(DI.get(name), op, r2=r2, H=H, W=W)
    assert DI.same_masks(got, DI.reference(name, op, r2, H, W))
    return got


# ---- the word-boundary set ----

def test_word_boundary_distance_and_inscribed():
    pm = DI.get("word")
    assert set(DI.WIDTHS) == set((pm.bounds[:, 2] - pm.bounds[:, 0] + 1).tolist()) and (pm.bounds[:, 0] < 0).any()
    assert set(DI.HEIGHTS) == set((pm.bounds[:, 3] - pm.bounds[:, 1] + 1).tolist())
    _maps("word")
    _discs("word")


@pytest.mark.parametrize("r2", DI.R2S)
@pytest.mark.parametrize("op", DI.OPS)
def test_word_boundary_morphology(op, r2):
    _morph("word", op, r2)


# ---- a whole word's reach ----

@pytest.mark.parametrize("r2", DI.WORD_R2S)
@pytest.mark.parametrize("op", DI.OPS)
def test_discs_of_a_whole_words_reach(op, r2):
    pm = DI.get("reach")
    assert ((pm.bounds[:, 2] - pm.bounds[:, 0] + 1) > 128).all()
    got = _morph("reach", op, r2)
    if op == "dilate":
        assert got.areas[4] > 2 * 3 * 100                         # the two dots became discs


def test_a_disc_larger_than_the_masks():
    pm, r2 = DI.get("reach").take([0, 4]), 210 * 210             # 129 and 200 columns wide
    for op in ("erode", "open"):
        got = DT.morph(pm, op, r2=r2)
        assert DI.same_masks(got, DT.morph_numpy(pm, op, r2))
        assert (got.areas == 0).all() and not got.bits.any() and np.array_equal(got.bounds, pm.bounds)
    want = DT.morph_numpy(pm, "close", r2)
    got = DT.morph(pm, "close", r2=r2)
    assert DI.same_masks(got, want) and got.bits.tobytes() == want.bits.tobytes() and want.areas[0] > pm.areas[0]


# ---- the far zero ----

def test_far_zero_rectangles_equal_the_closed_form():
    pm = DI.get("far")
    got = _maps("far")
    for i, (h, w) in enumerate(((260, 600), (600, 260))):
        assert pm.size(i) == (h, w)
        yy, xx = np.mgrid[0:h, 0:w]
        want = np.minimum(np.minimum(xx + 1, w - xx), np.minimum(yy + 1, h - yy)) ** 2
        assert np.array_equal(got.map(i), want.astype(np.uint32)) and got.map(i).max() == 130 * 130
    xy, r2 = _discs("far")
    # the ties: the first pixel at depth 130 in raster order is (129, 129) of either rectangle
    assert r2.tolist() == [130 * 130, 130 * 130]
    assert (xy - pm.bounds[:, :2]).tolist() == [[129, 129], [129, 129]]
    for op, r in (("erode", 129 * 129), ("erode", 130 * 130), ("close", 100 * 100)):
        _morph("far", op, r)


# ---- tall narrow masks ----

def test_tall_narrow_masks():
    _maps("tall")
    xy, r2 = _discs("tall")
    assert r2[[0, 2, 4]].tolist() == [1, 1, 4]
    for op in DI.OPS:
        for r in (1, 2, 9):
            _morph("tall", op, r)


# ---- bounds ----

def test_bounds_that_leave_an_image_and_instances_without_rows():
    pm = DI.get("bounds")
    H, W = DI.BOUNDS_H, DI.BOUNDS_W
    _maps("bounds")
    xy, r2 = _discs("bounds")
    assert xy[[6, 7, 10]].tolist() == [[-1, -1]] * 3 and r2[[6, 7, 10]].tolist() == [0, 0, 0]
    for op in DI.OPS:
        got = _morph("bounds", op, 25)
        if op != "dilate":
            assert np.array_equal(got.bounds, pm.bounds)
    got = _morph("bounds", "dilate", 25, H, W)
    assert got.bounds[[6, 9, 10]].tolist() == [[0, 0, -1, -1]] * 3                    # no rows, nothing left, no rows
    assert got.bounds[8].tolist() == [0, 5, 2, 35] and got.bounds[0].tolist() == [0, 0, 85, 45]
    assert got.bounds[5].tolist() == [0, 0, W - 1, H - 1] and got.areas[8] > 0
    free = _morph("bounds", "dilate", 25)
    assert free.bounds[8].tolist() == [-85, 5, 2, 35] and free.bounds[6].tolist() == pm.bounds[6].tolist()


@pytest.mark.parametrize("name", ["many65", "many130", "empty"])
def test_more_than_one_wave_of_instances_and_none(name):
    assert len(DI.get(name)) == {"many65": 65, "many130": 130, "empty": 0}[name]
    _maps(name)
    _discs(name)
    for op in DI.OPS:
        _morph(name, op, 5)
    _morph(name, "dilate", 5, 40, 300)


def test_dirty_padding_bits_change_nothing():
    dirty, clean = DI.word_set(dirty=True), DI.get("word")
    assert not np.array_equal(dirty.bits, clean.bits)
    assert DI.same_arrays(DT.distance(dirty), DI.reference("word", "distance"))
    assert DI.same_arrays(DT.inscribed(dirty), DI.reference("word", "inscribed"))
    for op in DI.OPS:
        assert DI.same_masks(DT.morph(dirty, op, r2=5), DI.reference("word", op, 5, None, None))
    clean_bounds = DI.bounds_set(dirty=False)
    assert DI.same_masks(DT.morph(clean_bounds, "close", r2=25), DI.reference("bounds", "close", 25, None, None))


# ---- real size ----

def test_real_size_every_surface_and_repeatability():
    pm = DI.get("real")
    assert len(pm) == 10 and (pm.bounds[:, 0] < 0).any()
    maps = _maps("real")
    assert DI.same_arrays(pm.distance(), maps) and DI.same_arrays(MT.mask_distance(pm), maps)
    assert maps.sq.tobytes() == DT.distance(pm).sq.tobytes()
    discs = _discs("real")
    assert DI.same_arrays(pm.inscribed(), discs) and DI.same_arrays(MT.mask_inscribed(pm), discs)
    for i in range(len(pm)):                                       # the deepest pixel lies in the mask, at that depth
        if discs[1][i]:
            dx, dy = (discs[0][i] - pm.bounds[i, :2]).tolist()
            assert pm.dense(i)[dy, dx] and maps.map(i)[dy, dx] == discs[1][i] == maps.map(i).max()
    r2 = DT.radius_sq(2)
    for op, method, wrapper in (("erode", pm.erode, MT.mask_erode), ("open", pm.open, MT.mask_open), ("close", pm.close, MT.mask_close)):
        got = _morph("real", op, r2)
        assert DI.same_masks(method(2), got) and DI.same_masks(method(r2=r2), got) and DI.same_masks(wrapper(pm, 2), got)
        again = DT.morph(pm, op, r2=r2)
        assert all(getattr(again, f).tobytes() == getattr(got, f).tobytes() for f in PackedMasks.FIELDS)
    r2 = DT.radius_sq(23)
    got = _morph("real", "dilate", r2, 600, 1000)
    assert DI.same_masks(pm.dilate(23, H=600, W=1000), got) and DI.same_masks(MT.mask_dilate(pm, r2=r2, H=600, W=1000), got)
    assert DI.same_masks(pm.dilate(r2=r2), _morph("real", "dilate", r2))
    changed = DI.reference("real", "open", 4, None, None)
    assert (changed.areas != pm.areas).any()


# ---- buffers ----

def test_room_to_spare_keeps_its_canary_and_too_little_room_writes_nothing():
    pm = DI.get("bounds")
    want = DI.reference("bounds", "dilate", 25, DI.BOUNDS_H, DI.BOUNDS_W)
    need = want.bits.nbytes
    roomy = np.full(need // 8 + 4, CANARY, np.uint64)
    bounds, offsets, areas, size = DT.morph_call(pm, 1, 25, DI.BOUNDS_H, DI.BOUNDS_W, roomy)
    assert size == need and np.array_equal(roomy[:need // 8], want.bits) and (roomy[need // 8:] == CANARY).all()
    assert np.array_equal(areas, want.areas) and np.array_equal(bounds, want.bounds) and np.array_equal(offsets, want.offsets)
    # sizes only: nothing is launched, the table and the size come back
    bounds, offsets, areas, size = DT.morph_call(pm, 1, 25, DI.BOUNDS_H, DI.BOUNDS_W, None)
    assert size == need and np.array_equal(bounds, want.bounds) and np.array_equal(offsets, want.offsets) and not areas.any()
    # too little room: the sizes, and nothing else
    small = np.full(need // 8 - 1, CANARY, np.uint64)
    n = len(pm)
    ob, oo, oa = np.zeros((n, 4), np.int32), np.zeros(n, np.int64), np.full(n, -7, np.int64)
    size = ctypes.c_size_t(0)
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_mask_morph", *(_set_args(pm, areas=False) + (
            1, 25, DI.BOUNDS_H, DI.BOUNDS_W, _lib.ptr(ob), _lib.ptr(oo), _lib.ptr(oa), _lib.ptr(small), small.nbytes,
            ctypes.addressof(size), 0)))
    assert e.value.code == INVALID and size.value == need and (small == CANARY).all() and (oa == -7).all()
    assert np.array_equal(ob, want.bounds) and np.array_equal(oo, want.offsets)


def test_distance_buffers():
    pm = DI.get("bounds")
    want = DI.reference("bounds", "distance")
    total = int(want.dist_ptr[-1])
    dist_ptr, size = DT.distance_call(pm, None)
    assert size == total and np.array_equal(dist_ptr, want.dist_ptr)
    roomy = np.full(total + 5, 0x55555555, np.uint32)
    dist_ptr, size = DT.distance_call(pm, roomy)
    assert size == total and np.array_equal(roomy[:total], want.sq) and (roomy[total:] == 0x55555555).all()
    small = np.full(total - 1, 0x55555555, np.uint32)
    with pytest.raises(_lib.MncError) as e:
        DT.distance_call(pm, small)
    assert e.value.code == INVALID and (small == 0x55555555).all()


# ---- invalid arguments ----

def _refused(pm, op, r2, H, W, n=None):
    n = len(pm) if n is None else n
    ob, oo, oa = np.full((max(n, 1), 4), 77, np.int32), np.full(max(n, 1), 77, np.int64), np.full(max(n, 1), 77, np.int64)
    bits, size = np.full(64, CANARY, np.uint64), ctypes.c_size_t(12345)
    args = _set_args(pm, areas=False)[:4] + (n,)
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_mask_morph", *(args + (op, r2, H, W, _lib.ptr(ob), _lib.ptr(oo), _lib.ptr(oa), _lib.ptr(bits), bits.nbytes,
                                              ctypes.addressof(size), 0)))
    assert e.value.code == INVALID
    assert (ob == 77).all() and (oo == 77).all() and (oa == 77).all() and (bits == CANARY).all() and size.value == 12345
    return True


def test_invalid_arguments_are_refused_and_nothing_is_written():
    pm = DI.get("many65").take([0, 1, 2])
    assert _refused(pm, 4, 1, 0, 0) and _refused(pm, -1, 1, 0, 0)                      # a bad op
    assert _refused(pm, 0, -1, 0, 0) and _refused(pm, 0, 1024 * 1024 + 1, 0, 0)         # r2
    assert _refused(pm, 1, 4, 50, 0) and _refused(pm, 1, 4, 0, 50) and _refused(pm, 1, 4, 32769, 50)   # H without W
    big = np.zeros((2049, 4), np.int32)
    big[:, 2:] = -1
    none = PackedMasks(big, np.zeros(2049, np.int64), np.zeros(2049, np.int64), None, None, np.zeros(0, np.uint64))
    assert _refused(none, 0, 1, 0, 0)                                                  # n = 2049
    edge = DI.MI.pack([[2 ** 24 - 12, 0, 2 ** 24 - 3, 4]], [np.ones((5, 10), bool)])
    assert DI.same_masks(DT.morph(edge, "dilate", r2=4), DT.morph_numpy(edge, "dilate", 4))     # 2^24 - 1 is still a coordinate
    assert _refused(edge, 1, 9, 0, 0) and _refused(edge, 3, 9, 0, 0)                   # grown to 2^24
    assert DI.same_masks(DT.morph(edge, "erode", r2=9), DT.morph_numpy(edge, "erode", 9))
    for bad in ({"op": "shrink", "r2": 1}, {"op": "erode"}, {"op": "erode", "r2": 1, "radius": 1.0}, {"op": "dilate", "r2": 1, "H": 5}):
        with pytest.raises(ValueError):
            DT.morph(pm, **bad)


# ---- a device-resident result ----

def _block(rec, counts, cap):
    from mnc_amd.engine import _Ctx
    ctx = _Ctx(0)
    blk = InstanceBlock(types.SimpleNamespace(_ctx=ctx), 21, RI.S, 100, 300)
    assert blk.rows_cap >= cap
    head = np.zeros(HEAD_BYTES // 4, np.int32)
    head[:len(counts)] = counts
    raw = np.concatenate((head.view(np.uint8), np.ascontiguousarray(rec).reshape(-1).view(np.uint8)))
    _lib.call("mnc_h2d", ctx.h, blk.ptr, _lib.ptr(raw), raw.nbytes)
    return blk, ctx


def test_device_resident_result_gives_what_its_host_copy_gives():
    rng = np.random.default_rng(72)
    h, w = 70, 200
    list_mask, list_box = RI.class_lists(rng, w, h, 0.5)
    cap = 200
    rec, total = records_from_lists(list_mask, list_box, cap, RI.S)
    blk, ctx = _block(rec, [total] + [len(b) for b in list_box], cap)
    try:
        view = blk.view()
        flat = PackedMasks(**view.masks(h, w, score_thresh=0.0).fetch().arrays())
        assert len(flat) > 3
        pm = view.masks(h, w, score_thresh=0.0)
        assert "bits" not in pm._host and pm._device() is not None
        assert DI.same_masks(pm.open(r2=5), DT.morph_numpy(flat, "open", 5))
        assert DI.same_masks(pm.dilate(r2=5, H=h, W=w), DT.morph_numpy(flat, "dilate", 5, h, w))
        assert DI.same_arrays(pm.distance(), DT.distance_numpy(flat)) and DI.same_arrays(pm.inscribed(), DT.inscribed_numpy(flat))
    finally:
        blk.release()
        ctx.close()


# ---- the demo ----

def test_demo_smooth_radius_writes_close_of_open(tmp_path):
    import glob
    import io
    import json
    from contextlib import redirect_stdout

    import demo
    from mnc_amd import models
    jpg = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "demo", "*.jpg")))[0]
    proto = models.write_mnc_5stage_test_prototxt(width_div=8)
    name = os.path.splitext(os.path.basename(jpg))[0]
    im = demo._read_image_bgr(jpg)
    got, saved = {}, {}
    for key, flags in (("plain", []), ("smooth", ["--smooth-radius", "2"]), ("smooth_cpu", ["--smooth-radius", "2", "--cpu"])):
        out = str(tmp_path / (key + ".json"))
        os.makedirs(str(tmp_path / key))
        with redirect_stdout(io.StringIO()):
            demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-coco", out, "--save-masks", str(tmp_path / key),
                       "--vis-thresh", "0.0"] + flags)
        with open(out) as f:
            got[key] = json.load(f)
        saved[key] = PackedMasks.load(str(tmp_path / key / (name + "_masks.npz")))
    pm = saved["plain"]
    assert len(pm) > 0
    want = DT.morph_numpy(DT.morph_numpy(pm, "open", 4), "close", 4)
    assert DI.same_masks(saved["smooth"], want) and DI.same_masks(saved["smooth_cpu"], want)     # --cpu: the numpy statements
    assert (want.areas != pm.areas).any() and got["smooth_cpu"] == got["smooth"]
    assert got["smooth"] == json.loads(json.dumps(demo._coco_results(name, im.shape, want, cpu=True)))
