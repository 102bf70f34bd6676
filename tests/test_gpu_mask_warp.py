"""The geometric transforms of packed instance masks on the GPU (csrc/mask_warp.hip: mnc_mask_isometry, mnc_mask_warp and the Python
surfaces over them) against the numpy statements (mnc_amd.warp.isometry_numpy and warp_numpy, which tests/test_mask_warp_host.py
pins to numpy's flips and rotations, np.kron, a brute force in Python integers and closed forms).  Every comparison is exact, field
by field, dtype and shape included.  The sets, maps and windows are those of tests/mask_warp_inputs.py."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import mask_warp_inputs as WI  # noqa: E402
import render_inputs as RI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import algebra as AL  # noqa: E402
from mnc_amd import warp as WP  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, InstanceBlock, records_from_lists  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY = np.uint64(0x5555555555555555)
BIG = (-2000, -2000, 2000, 2000)


# ---- word and block boundaries ----

@pytest.mark.parametrize("code", WI.CODES)
def test_isometries_at_word_and_block_boundaries(code):
    pm = WI.get("word")
    assert sorted(set(pm.size(i) for i in range(len(pm))))[0] == (1, 1) and (130, 1) in [pm.size(i) for i in range(len(pm))]
    for tx, ty in ((0, 0), WI.SHIFTS[code]):
        got = WP.isometry(pm, code, tx, ty)
        assert WI.same_masks(got, WI.isometry_ref("word", code, tx, ty)) and WI.canonical(got) and got.areas.any()
    got = WP.isometry(WI.get("negative"), code, *WI.SHIFTS[code])
    assert WI.same_masks(got, WI.isometry_ref("negative", code, *WI.SHIFTS[code]))


@pytest.mark.parametrize("code", WI.CODES)
def test_loose_bounds_and_set_padding_bits_change_nothing(code):
    clean, dirty = WI.get("word"), WI.get("word_dirty")
    assert not np.array_equal(clean.bits, dirty.bits) and np.array_equal(clean.bounds, dirty.bounds)
    tight = AL.combine_numpy(clean, None, "copy")
    assert (tight.bounds != clean.bounds).any(axis=1).sum() > 10             # bounds with empty border rows and columns
    want = WI.isometry_ref("word", code, 3, -7)
    assert WI.same_masks(WP.isometry(dirty, code, 3, -7), want)
    assert WI.same_masks(WP.isometry(tight, code, 3, -7), want)
    coef, den = WP.isometry_map(code, 3, -7)
    assert WI.same_masks(WP.warp(dirty, coef, den, BIG), want)               # the other kernel


# ---- more instances than a scan tile ----

def test_1025_instances_cross_the_size_kernels_blocks_and_the_scans_tile():
    pm = WI.get("edge")
    assert len(pm) == 1025 and sum(h * w == 0 for h, w in (pm.size(i) for i in range(len(pm)))) == 146
    for code, tx, ty in ((2, 19, -3), (1, -40, 7)):                          # rows stay rows; rows become columns of up to 65 rows
        got = WP.isometry(pm, code, tx, ty)
        assert WI.same_masks(got, WI.isometry_ref("edge", code, tx, ty)) and WI.canonical(got)
        assert got.areas.sum() == pm.areas.sum() and got.areas[1024] > 0 and got.offsets[1024] > got.offsets[1023] > 0


# ---- the empty cases ----

def test_empty_cases():
    e = WI.get("empty")
    for code in WI.CODES:
        assert WI.same_masks(WP.isometry(e, code, 1, 2), WP.isometry_numpy(e, code, 1, 2)) and len(WP.isometry(e, code)) == 0
    assert WI.same_masks(WP.warp(e, (1, 0, 0, 0, 1, 0), 1, BIG), WP.warp_numpy(e, (1, 0, 0, 0, 1, 0), 1, BIG))
    pm = WI.get("image0")
    rowless = pm.take([6, 6])
    assert tuple(rowless.bounds[0]) == (0, 0, -1, -1)
    for code in (2, 5):
        assert WI.same_masks(WP.isometry(rowless, code, 4, 4), WP.isometry_numpy(rowless, code, 4, 4))
    got = WP.isometry(pm, 5, 0, 69)
    assert tuple(got.bounds[6]) == (0, 0, -1, -1) and tuple(got.bounds[7]) == (0, 0, -1, -1) and got.areas[5] == pm.areas[5]
    name, coef, den = WI.maps()["rotation16"]
    far = WP.warp(pm, coef, den, WI.FAR_WINDOW)                              # answered on the host
    assert WI.same_masks(far, WP.warp_numpy(pm, coef, den, WI.FAR_WINDOW)) and far.bits.size == 0 and not far.areas.any()
    rc, bound, used, *_ = _warp_call(pm, coef, den, WI.FAR_WINDOW, np.full(4, CANARY, np.uint64))
    assert rc == 0 and bound == 0 and used == 0


# ---- the gather ----

@pytest.mark.parametrize("name,H,W", [("image0",) + WI.IMAGES[0], ("image1",) + WI.IMAGES[1]])
def test_resizes(name, H, W):
    pm = WI.get(name)
    for H2, W2 in WI.RESIZES[(H, W)]:
        coef, den = WP.resize_map(H, W, H2, W2)
        window = (0, 0, W2 - 1, H2 - 1)
        got = WP.warp(pm, coef, den, window)
        assert WI.same_masks(got, WI.warp_ref(name, coef, den, window)), (H2, W2)
        assert WI.same_masks(pm.resize(H, W, H2, W2), got) and got.areas.any()


@pytest.mark.parametrize("key", sorted(WI.maps()))
@pytest.mark.parametrize("window", WI.WINDOWS)
def test_gathers_in_windows_that_cut_at_and_inside_a_word(key, window):
    name, coef, den = WI.maps()[key]
    got = WP.warp(WI.get(name), coef, den, window)
    assert WI.same_masks(got, WI.warp_ref(name, coef, den, window))
    live = got.areas > 0
    assert (got.bounds[live, 0] >= window[0]).all() and (got.bounds[live, 2] <= window[2]).all()
    if window == WI.WINDOWS[0]:
        assert got.areas.sum() > 500 and WI.canonical(got)


@pytest.mark.parametrize("code", WI.CODES)
def test_the_gather_through_an_isometry_map_is_the_isometry_kernel(code):
    for name in ("word", "negative"):
        pm = WI.get(name)
        tx, ty = WI.SHIFTS[code]
        assert WI.same_masks(WP.warp(pm, *WP.isometry_map(code, tx, ty), window=BIG), WP.isometry(pm, code, tx, ty)), name


def test_denominators_and_numerators_at_their_limits():
    pm = WI.get("negative")
    want = AL.combine_numpy(pm, None, "copy")
    for den in (1 << 32, (1 << 32) - 5, 3):                                  # a shift, and divisions with numerators near 2^56
        assert WI.same_masks(WP.warp(pm, (den, 0, 0, 0, den, 0), den, BIG), want), den
    # floors of negative quotients that den does not divide: down by 3, up by 3, and a mixed map over 9
    for coef, den in (((3, 0, 1, 0, 3, 2), 1), ((1, 0, 0, 0, 1, 0), 3), ((5, 0, -3, 0, -7, 11), 9)):
        got = WP.warp(pm, coef, den, (-120, -80, 40, 30))
        assert WI.same_masks(got, WP.warp_numpy(pm, coef, den, (-120, -80, 40, 30))) and got.areas.any(), (coef, den)
    # numerators near 2^55: sx = -x + far - 256, sy = y + 128 - far, seen through a window at far = 2^23
    far = 1 << 23
    window = (far - 100, far - 300, far + 400, far + 100)
    for den in (1 << 32, (1 << 32) - 5):
        coef = (-den, 0, den * (far - 256), 0, den, den * (128 - far))
        got = WP.warp(pm, coef, den, window)
        assert WI.same_masks(got, WP.warp_numpy(pm, coef, den, window)) and got.areas.any(), den
    # an offset at 2^60 takes every source out of reach: nothing, and nothing wraps around
    got = WP.warp(pm, (7, 0, -(1 << 60), 0, 7, 1 << 60), 5, BIG)
    assert not got.areas.any() and got.bits.size == 0


# ---- the C ABI ----

def _call(entry, pm, middle, bits, cap=None, n_out=None):
    """An n18 entry as it is -> (status, bound, used, bounds, offsets, areas)."""
    n = len(pm) if n_out is None else n_out
    bounds, offsets, areas = np.full((n, 4), 77, np.int32), np.full(n, 77, np.int64), np.full(n, 77, np.int64)
    bound, used = ctypes.c_size_t(12345), ctypes.c_size_t(54321)
    rc = getattr(_lib.load(), entry)(*(_set_args(pm, areas=False) + middle + (
        _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits),
        (bits.nbytes if bits is not None else 0) if cap is None else cap, ctypes.addressof(bound), ctypes.addressof(used), 0)))
    return rc, bound.value, used.value, bounds, offsets, areas


def _warp_call(pm, coef, den, window, bits, cap=None):
    c, win = np.array(coef, np.int64), np.array(window, np.int32)
    return _call("mnc_mask_warp", pm, (_lib.ptr(c), int(den), _lib.ptr(win)), bits, cap)


def _isometry_call(pm, code, tx, ty, bits, cap=None):
    return _call("mnc_mask_isometry", pm, (int(code), int(tx), int(ty)), bits, cap)


def test_the_size_call_launches_nothing_and_returns_the_statements_bound():
    pm = WI.get("word")
    rows = [i for i in range(len(pm)) if AL._rows(pm, i)]
    WP.timing(True)
    try:
        for code in (2, 5):
            rc, bound, used, bounds, offsets, areas = _isometry_call(pm, code, 9, -9, None)
            assert rc == 0 and used == 54321 and (bounds == 77).all() and (offsets == 77).all() and (areas == 77).all()
            assert WP.timing(True) == -1.0                   # no launch was timed
            assert bound == WI.bound_bytes([WP.isometry_frame(AL._box(pm, i), code, 9, -9) for i in rows])
            want = WI.isometry_ref("word", code, 9, -9)
            bits = np.full(bound // 8, CANARY, np.uint64)
            rc, bound2, used, *_ = _isometry_call(pm, code, 9, -9, bits)
            assert rc == 0 and bound2 == bound and used == want.bits.nbytes < bound
            assert WP.timing(True) > 0.0
        name, coef, den = WI.maps()["rotation16"]
        pm = WI.get(name)
        for window in WI.WINDOWS:
            rc, bound, used, *_ = _warp_call(pm, coef, den, window, None)
            frames = [WP.warp_frame(AL._box(pm, i), coef, den, window) for i in range(len(pm)) if AL._rows(pm, i)]
            assert rc == 0 and used == 54321 and bound == WI.bound_bytes(frames), window
    finally:
        WP.timing(False)


@pytest.mark.parametrize("kind", ["isometry", "warp"])
def test_bytes_past_the_result_and_past_the_room_are_never_written(kind):
    if kind == "isometry":
        pm, want = WI.get("word"), WI.isometry_ref("word", 7, 11, 5)
        call = lambda bits, cap=None: _isometry_call(pm, 7, 11, 5, bits, cap)     # noqa: E731
    else:
        name, coef, den = WI.maps()["shear16"]
        pm, want = WI.get(name), WI.warp_ref(name, coef, den, WI.WINDOWS[0])
        call = lambda bits, cap=None: _warp_call(pm, coef, den, WI.WINDOWS[0], bits, cap)     # noqa: E731
    bound = call(None)[1]
    bits = np.full(bound // 8 + 16, CANARY, np.uint64)
    rc, _, used, bounds, offsets, areas = call(bits, bound)
    assert rc == 0 and used == want.bits.nbytes < bound
    assert np.array_equal(bits[:used // 8], want.bits) and (bits[used // 8:] == CANARY).all()
    assert np.array_equal(bounds, want.bounds) and np.array_equal(offsets, want.offsets) and np.array_equal(areas, want.areas)
    # too little room: only the bound is set
    bits[:] = CANARY
    rc, bound2, used, bounds, offsets, areas = call(bits, bound - 8)
    assert rc == INVALID and bound2 == bound and used == 54321 and (bits == CANARY).all()
    assert (bounds == 77).all() and (offsets == 77).all() and (areas == 77).all()


def _refused(entry, pm_args, middle):
    """The call returns MNC_ERR_INVALID and writes nothing into its outputs."""
    n = 8
    bounds, offsets, areas = np.full((n, 4), 77, np.int32), np.full(n, 77, np.int64), np.full(n, 77, np.int64)
    bits = np.full(4096, CANARY, np.uint64)
    bound, used = ctypes.c_size_t(12345), ctypes.c_size_t(54321)
    rc = getattr(_lib.load(), entry)(*(pm_args + middle + (_lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits),
                                                           bits.nbytes, ctypes.addressof(bound), ctypes.addressof(used), 0)))
    assert rc == INVALID, (entry, rc)
    assert (bounds == 77).all() and (offsets == 77).all() and (areas == 77).all() and (bits == CANARY).all()
    assert bound.value == 12345 and used.value == 54321
    return True


def test_every_invalid_argument_is_refused_before_a_launch():
    pm = WI.get("negative")                                  # six instances
    sa = _set_args(pm, areas=False)
    keep = []                                                # (the arrays behind the pointers)

    def warp_args(coef, den, window):
        keep.append((np.array(coef, np.int64), None if window is None else np.array(window, np.int32)))
        return (_lib.ptr(keep[-1][0]), den, _lib.ptr(keep[-1][1]))

    ident, win = (1, 0, 0, 0, 1, 0), (0, 0, 9, 9)
    for code, tx, ty in ((8, 0, 0), (-1, 0, 0), (2, 1 << 24, 0), (4, 0, -(1 << 24)), (2, (1 << 24) - 1, 0), (1, 0, 100 - (1 << 24)),
                         (6, 0, (1 << 24) - 2)):                             # (the last three: a result coordinate out of range)
        assert _refused("mnc_mask_isometry", sa, (code, tx, ty)), (code, tx, ty)
    for coef, den, window in ((ident, 0, win), (ident, -1, win), (ident, (1 << 32) + 1, win), (ident, 1, (0, 0, 1 << 24, 5)),
                              (ident, 1, (-(1 << 24), 0, 5, 5)), (ident, 1, (5, 5, 4, 9)), (ident, 1, (5, 5, 9, 4)), (ident, 1, None),
                              ((1, 2, 0, 2, 4, 0), 1, win), ((0, 0, 0, 0, 0, 0), 1, win), (((1 << 32) + 1, 0, 0, 0, 1, 0), 1, win),
                              ((1, -(1 << 32) - 1, 0, 0, 1, 0), 1, win), ((1, 0, 0, (1 << 32) + 1, 1, 0), 1, win),
                              ((1, 0, 0, 0, -(1 << 32) - 1, 0), 1, win), ((1, 0, (1 << 60) + 1, 0, 1, 0), 1, win),
                              ((1, 0, 0, 0, 1, -(1 << 60) - 1), 1, win)):
        assert _refused("mnc_mask_warp", sa, warp_args(coef, den, window)), (coef, den, window)
    assert _refused("mnc_mask_warp", sa, (None, 1, _lib.ptr(np.array(win, np.int32))))
    # what mnc_mask_combine refuses about a set
    bad = PackedMasks(pm.bounds, pm.offsets + 4, pm.areas, None, None, pm.bits)
    short = (_lib.ptr(pm.bounds), _lib.ptr(pm.offsets), _lib.ptr(pm.bits), pm.bits.nbytes - 8, len(pm))
    wide = PackedMasks(np.array([[-(1 << 24), 0, 5, 5]], np.int32), [0], [0], None, None, np.zeros(8, np.uint64))
    for args in (_set_args(bad, areas=False), short, (None,) + sa[1:], _set_args(wide, areas=False), sa[:4] + (2049,), sa[:4] + (-1,)):
        assert _refused("mnc_mask_isometry", args, (2, 5, 5))
        assert _refused("mnc_mask_warp", args, warp_args(ident, 1, win))
    # more than 2^27 pixels of loose-frame rows: three instances blown up 3000 times each way
    big = PackedMasks(np.array([[0, 0, 9, 9]] * 3, np.int32), [0, 80, 160], [0, 0, 0], None, None, np.zeros(30, np.uint64))
    assert _refused("mnc_mask_warp", _set_args(big, areas=False), warp_args(ident, 3000, (0, 0, 40000, 40000)))
    # null outputs
    lib, bound = _lib.load(), ctypes.c_size_t(0)
    one = np.zeros(1 << 12, np.uint64)
    assert lib.mnc_mask_isometry(*(sa + (2, 5, 5, None, None, None, None, 0, None, None, 0))) == INVALID
    assert lib.mnc_mask_isometry(*(sa + (2, 5, 5, None, None, None, _lib.ptr(one), one.nbytes, ctypes.addressof(bound), None,
                                         0))) == INVALID
    assert lib.mnc_mask_warp(*(sa + warp_args(ident, 1, win) + (None, None, None, None, 0, None, None, 0))) == INVALID
    # the Python side raises ValueError for its own arguments, MncError for the set
    with pytest.raises(ValueError):
        pm.isometry(8)
    with pytest.raises(ValueError):
        pm.warp(ident, 0, win)
    with pytest.raises(_lib.MncError):
        WP.isometry(bad, 2, 5, 5)


# ---- determinism ----

def test_two_calls_give_the_same_bytes():
    pm = WI.get("word")
    name, coef, den = WI.maps()["rotation10"]
    for call in (lambda: WP.isometry(pm, 3, 8, 8), lambda: WP.isometry(pm, 6, -8, 8),
                 lambda: WP.warp(WI.get(name), coef, den, WI.WINDOWS[0])):
        x, y = call(), call()
        for f in PackedMasks.FIELDS:
            assert getattr(x, f).tobytes() == getattr(y, f).tobytes(), f


# ---- the Python surfaces ----

def test_methods_and_mask_transform_wrappers():
    H, W = WI.IMAGES[0]
    pm = WI.get("image0")
    iso = lambda *a: WI.isometry_ref("image0", *a)           # noqa: E731
    for got, want in ((pm.fliplr(W), iso(2, W - 1, 0)), (pm.flipud(H), iso(4, 0, H - 1)), (pm.transpose(), iso(1, 0, 0)),
                      (pm.rot90(1, H, W), iso(5, 0, W - 1)), (pm.rot90(-2, H, W), iso(6, W - 1, H - 1)),
                      (pm.rot90(7, H, W), iso(3, H - 1, 0)), (pm.rot90(4, H, W), iso(0, 0, 0)), (pm.isometry(7, -3, 4), iso(7, -3, 4)),
                      (MT.mask_fliplr(pm, W), iso(2, W - 1, 0)), (MT.mask_flipud(pm, H), iso(4, 0, H - 1)),
                      (MT.mask_transpose(pm), iso(1, 0, 0)), (MT.mask_rot90(pm, 3, H, W), iso(3, H - 1, 0)),
                      (MT.mask_isometry(pm, 7, -3, 4), iso(7, -3, 4))):
        assert WI.same_masks(got, want)
    for i in (0, 3, 4, 5):
        assert np.array_equal(pm.fliplr(W).full(i, H, W), np.fliplr(pm.full(i, H, W)))
        assert np.array_equal(pm.rot90(1, H, W).full(i, W, H), np.rot90(pm.full(i, H, W)))
    moved = pm.translate(-100, 33)
    assert WI.same_masks(moved.translate(100, -33), pm) and WI.same_masks(moved.tighten(), iso(0, -100, 33))
    for bits in (10, 16):
        coef, den = WP.affine_map(WI.ROTATION, bits)
        want = WI.warp_ref("image0", coef, den, (0, 0, 79, 49))
        assert WI.same_masks(pm.warp_affine(WI.ROTATION, 50, 80, frac_bits=bits), want)
        assert WI.same_masks(MT.mask_warp_affine(pm, WI.ROTATION, 50, 80, bits), want)
        assert WI.same_masks(pm.warp(coef, den, (0, 0, 79, 49)), want) and WI.same_masks(MT.mask_warp(pm, coef, den, (0, 0, 79, 49)), want)
    assert WI.same_masks(MT.mask_resize(pm, H, W, 55, 105), WI.warp_ref("image0", *WP.resize_map(H, W, 55, 105), (0, 0, 104, 54)))


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


def test_a_device_resident_result_is_fetched_and_transformed():
    rng = np.random.default_rng(74)
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
        flipped = pm.fliplr(w)
        assert WI.same_masks(flipped, WP.isometry_numpy(flat, 2, w - 1, 0))
        assert WI.same_masks(flipped.fliplr(w), AL.combine_numpy(flat, None, "copy"))
        assert WI.same_masks(flipped.fliplr(w), flat.tighten())
    finally:
        blk.release()
        ctx.close()


# ---- the demo's helper ----

def test_flip_tta_helper_on_the_gpu_equals_the_host():
    import demo
    a, b, W = WI.tta_sets()
    for other in (a, b, AL.combine_numpy(a, a.take([1, 2, 0]), "or")):
        mirrored = WP.isometry_numpy(other, 2, W - 1, 0)
        assert WI.same_masks(demo._flip_tta(a, mirrored, W, 0.5, cpu=False), demo._flip_tta(a, mirrored, W, 0.5, cpu=True))
    assert len(demo._flip_tta(a, WP.isometry_numpy(a, 2, W - 1, 0), W, 0.5)) == len(a)


def test_demo_flip_tta_merges_the_mirrored_run(tmp_path):
    import glob
    import io
    from contextlib import redirect_stdout

    import demo
    from mnc_amd import models
    from mnc_amd.masks import mask_nms_numpy
    jpg = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "demo", "*.jpg")))[0]
    proto = models.write_mnc_5stage_test_prototxt(width_div=8)
    name = os.path.splitext(os.path.basename(jpg))[0]
    saved = {}
    for key, flags in (("plain", []), ("tta", ["--flip-tta"]), ("tta_cpu", ["--flip-tta", "--cpu"]), ("all", ["--flip-tta", "--tta-nms", "1.0"])):
        os.makedirs(str(tmp_path / key))
        with redirect_stdout(io.StringIO()):
            demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-masks", str(tmp_path / key), "--vis-thresh", "0.0"] + flags)
        saved[key] = PackedMasks.load(str(tmp_path / key / (name + "_masks.npz")))
    plain, tta, everything = saved["plain"], saved["tta"], saved["all"]
    assert len(plain) > 1 and WI.same_masks(saved["tta_cpu"], tta)           # --cpu: the numpy statements
    # nothing is suppressed at IoU 1.0 (strict): the image's own instances first, as they were, then the mirrored run's
    assert len(everything) > len(plain) and WI.same_masks(everything.take(range(len(plain))), plain)
    keep = np.sort(mask_nms_numpy(everything, 0.5, class_aware=True))
    assert WI.same_masks(tta, everything.take(keep))
