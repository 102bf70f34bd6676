"""COCO run-length encoding of packed instance masks on the GPU and the way back (csrc/mask_rle.hip: mnc_mask_rle, mnc_mask_rle_dev,
mnc_mask_from_rle and the Python surfaces over them) against the numpy statements (mnc_amd.rle.rle_counts_numpy,
masks_from_counts_numpy, which tests/test_mask_rle_host.py pins to the hand cases).  Every comparison is exact.  The images are
no larger than 200 x 200 and placed where the kernels can go wrong: widths 1, 63, 64, 65, 128, 129 crossed with heights 1, 63, 64,
65, 129, empty, full and checkerboard masks, runs that go on from the bottom of one column into the top of the next, unclipped
bounds leaving the image on every side, instances without rows, dirty padding."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_rle_inputs as RI  # noqa: E402
import render_inputs as RDI  # noqa: E402
from mnc_amd import _lib, rle  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, InstanceBlock, records_from_lists  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

S = RDI.S


def _same_counts(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return True


def _same_masks(got, want):
    for f in ("bounds", "offsets", "areas", "bits"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
    return True


def _both_ways(pm, H, W):
    """Encode against the statement, decode those counts against the statement, and close the loop through the strings."""
    want = rle.rle_counts_numpy(pm, H, W)
    got = rle.rle_counts(pm, H, W)
    assert _same_counts(got, want) and _same_counts(pm.rle_counts(H, W), want)
    back = rle.masks_from_counts(got[0], got[1], H, W)
    assert _same_masks(back, rle.masks_from_counts_numpy(want[0], want[1], H, W))
    loop = PackedMasks.from_rle(pm.rle(H, W))
    assert _same_masks(loop, back)
    assert all(np.array_equal(loop.full(i, H, W), pm.full(i, H, W)) for i in range(len(pm)))
    return want


@pytest.mark.parametrize("H", RI.HEIGHTS)
@pytest.mark.parametrize("W", RI.WIDTHS)
def test_sizes_around_the_tile(H, W):
    pm = RI.size_set(H, W)
    run_ptr, runs = _both_ways(pm, H, W)
    assert runs[run_ptr[3]:run_ptr[4]].tolist() == [H * W] and runs[run_ptr[4]:run_ptr[5]].tolist() == [0, H * W]


def test_checkerboard_has_a_transition_at_every_pixel():
    run_ptr, runs = _both_ways(RI.checkerboard(65), 65, 65)
    assert run_ptr.tolist() == [0, 65 * 65, 2 * 65 * 65 + 1]
    assert (runs[:run_ptr[1]] == 1).all() and runs[run_ptr[1]] == 0 and (runs[run_ptr[1] + 1:] == 1).all()


def test_runs_that_join_two_columns():
    H, W = 65, 140
    pm = RI.column_join(H, W)
    run_ptr, runs = _both_ways(pm, H, W)
    assert runs[run_ptr[0]:run_ptr[1]].tolist() == [H - 1, 2, H * W - H - 1]       # (0, H-1) and (1, 0) are one run
    assert runs[run_ptr[-2]:run_ptr[-1]][:3].tolist() == [5 * H + 3, H - 3, 3]     # closes at row 0, above the bounds' first row


def test_low_masks_on_the_last_rows_have_more_runs_than_pixels():
    H, W = 65, 140
    sets = RI.bottom_rows(H, W)
    for pm in sets:
        _both_ways(pm, H, W)
    run_ptr, runs = rle.rle_counts(sets[0], H, W)                                  # bounds [10, H-1, 20, H-1], all ones: 11 pixels
    assert run_ptr.tolist() == [0, 23] and runs.tolist() == [10 * H + H - 1] + [1, H - 1] * 10 + [1, (W - 21) * H]
    assert len(rle.rle_counts(sets[2], H, W)[1]) == 2 * W


@pytest.mark.parametrize("dirty", [False, True])
def test_bounds_that_leave_the_image_and_dirty_padding(dirty):
    H, W = 70, 200
    clean = RI.leaving(H, W)
    pm = RI.leaving(H, W, dirty=dirty)
    assert dirty == (not np.array_equal(pm.bits, clean.bits))
    want = rle.rle_counts_numpy(clean, H, W)
    assert _same_counts(rle.rle_counts(pm, H, W), want)
    assert [want[1][want[0][i]:want[0][i + 1]].tolist() for i in (5, 6, 7, 8, 9, 10, 11)] == [[H * W]] * 7
    _both_ways(pm, H, W)


@pytest.mark.parametrize("dirty", [False, True])
def test_forty_instances_of_mixed_sizes(dirty):
    H, W = 70, 200
    pm = RI.mixed(dirty)
    assert len(pm) == 40
    want = _both_ways(pm, H, W)
    assert _same_counts(rle.rle_counts(pm, H, W), want)                            # the same bits from run to run
    rles = MT.mask_rle(pm, H, W)
    assert rles == rle.mask_rle_numpy(pm, H, W) and rles[0]["size"] == [H, W]
    back = MT.masks_from_rle(rles, pm.classes, pm.scores)
    assert np.array_equal(back.classes, pm.classes) and np.array_equal(back.scores, pm.scores)
    # what the way back is for: the decoded set goes through overlaps() like any other
    inter, _ = back.overlaps()
    assert np.array_equal(np.diag(inter), back.areas)


def test_full_image_mask_and_empty_set():
    H, W = 129, 200
    pm = RI.whole([np.ones((H, W), bool), np.zeros((H, W), bool)])
    run_ptr, runs = _both_ways(pm, H, W)
    assert run_ptr.tolist() == [0, 2, 3] and runs.tolist() == [0, H * W, H * W]
    none = RI.MI.pack([], [])
    got = rle.rle_counts(none, H, W)
    assert got[0].tolist() == [0] and got[1].shape == (0,)
    assert len(PackedMasks.from_rle([])) == 0 and none.rle(H, W) == []


def test_zero_length_runs_decode_like_the_statement():
    H, W = 65, 70
    rng = np.random.default_rng(3)
    run_ptr, runs = rle.rle_counts_numpy(RI.size_set(H, W), H, W)
    loose, ptr = [], [0]
    for i in range(len(run_ptr) - 1):
        for c in runs[run_ptr[i]:run_ptr[i + 1]]:
            loose += [int(c), 0, 0] if rng.random() < 0.2 else [int(c)]            # (x, 0, 0) leaves the parity as it is
        loose += [0, 0]
        ptr.append(len(loose))
    loose = np.array(loose, np.uint32)
    want = rle.masks_from_counts_numpy(ptr, loose, H, W)
    got = rle.masks_from_counts(ptr, loose, H, W)
    assert _same_masks(got, want) and _same_counts(rle.rle_counts(got, H, W), (run_ptr, runs))
    shifted = np.concatenate((np.zeros(3, np.uint32), loose))                      # a run_ptr that does not begin at 0
    assert _same_masks(rle.masks_from_counts(np.array(ptr) + 3, shifted, H, W), want)


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


def test_device_form_equals_the_host_entry():
    rng = np.random.default_rng(71)
    h, w = 70, 200
    list_mask, list_box = RDI.class_lists(rng, w, h, 0.5)
    cap = 200
    rec, total = records_from_lists(list_mask, list_box, cap, S)
    assert 3 < total < cap
    rec[1, 0], rec[1, 2] = 60.0, 30.0                                              # x2 < x1: an instance without rows
    counts = [total] + [len(b) for b in list_box]
    blk, ctx = _block(rec, counts, cap)
    try:
        view = blk.view()
        pm = view.masks(h, w)
        assert "bits" not in pm._host and pm._device() is not None                # device-resident
        host = view.masks(h, w).fetch()                                            # the same image once more, copied
        with pytest.raises(RuntimeError):
            pm.rle_counts(h, w)                                                    # ... which made the first result stale
        with pytest.raises(RuntimeError):
            pm.rle(h, w)
        pm = view.masks(h, w)
        flat = PackedMasks(**host.arrays())                                        # host arrays alone: the host entry
        want = rle.rle_counts(flat, h, w)
        assert _same_counts(want, rle.rle_counts_numpy(flat, h, w))
        n = len(flat)
        assert 3 < n and min(flat.size(i)[1] for i in range(n)) == 0 and len(want[0]) == n + 1
        got = pm.rle_counts(h, w)
        assert "bits" not in pm._host and _same_counts(got, want)
        # room for too few runs: total_runs is the true total all the same, and the second call has room
        small = rle.device_rle_counts(pm._device(), h, w, runs_cap=7)
        assert len(want[1]) > 7 and _same_counts(small, want)
        d_rle = ctypes.c_void_p()
        dev = pm._device()
        _lib.call("mnc_mask_rle_dev", ctx.h, dev.d_info, dev.d_bits, dev.rows, h, w, 7, ctypes.addressof(d_rle))
        front = np.zeros(256 + 8 * (dev.rows + 1) + 4 * 7, np.uint8)
        _lib.call("mnc_d2h", ctx.h, _lib.ptr(front), d_rle.value, front.nbytes)
        head = front[:256].view(rle.RLE_HEAD)[0]
        assert head["kept"] == n and head["total_runs"] == len(want[1])
        ptr = front[256:256 + 8 * (dev.rows + 1)].view(np.int64)
        assert np.array_equal(ptr[:n + 1], want[0]) and (ptr[n:] == len(want[1])).all()
        assert np.array_equal(front[256 + 8 * (dev.rows + 1):].view(np.uint32), want[1][:7])
        assert pm.rle(h, w) == rle.mask_rle_numpy(flat, h, w)
        # the masks the _dev entry reads are as they were, and a fetched result that is still current goes on using the device
        assert all(np.array_equal(getattr(pm.fetch(), f), getattr(host, f)) for f in PackedMasks.FIELDS)
        assert _same_counts(view.masks(h, w).fetch().rle_counts(h, w), want)
    finally:
        blk.release()
        ctx.close()


def _invalid(name, *args):
    with pytest.raises(_lib.MncError) as e:
        _lib.call(name, *args)
    assert e.value.code == 1                                                       # MNC_ERR_INVALID
    return True


def test_invalid_arguments_are_refused_before_anything_is_launched():
    H, W = 70, 200
    pm = RI.leaving(H, W)
    n = len(pm)
    run_ptr, total, runs = np.zeros(n + 1, np.int64), ctypes.c_size_t(0), np.zeros(8, np.uint32)
    tot = ctypes.addressof(total)

    def enc(bounds=pm.bounds, offsets=pm.offsets, nbytes=pm.bits.nbytes, count=n, h=H, w=W, out=None, cap=0):
        return ("mnc_mask_rle", _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(pm.bits), nbytes, count, h, w, _lib.ptr(run_ptr),
                _lib.ptr(out), cap, tot, 0)

    assert _invalid(*enc(count=-1)) and _invalid(*enc(count=2049))
    for h, w in ((0, W), (H, 0), (32769, W), (H, 32769)):
        assert _invalid(*enc(h=h, w=w))
    bad = pm.bounds.copy()
    bad[0, 2] = 2 ** 24
    assert _invalid(*enc(bounds=bad))
    bad = pm.bounds.copy()
    bad[0] = (0, 0, 2 ** 13, 2 ** 13)                                              # more than 2^26 pixels
    assert _invalid(*enc(bounds=bad))
    for off in (-8, 4):
        bad = pm.offsets.copy()
        bad[0] = off
        assert _invalid(*enc(offsets=bad))
    assert _invalid(*enc(nbytes=pm.bits.nbytes - 8))                               # rows reaching past bytes
    # too little room: MNC_ERR_INVALID with the total set
    want = rle.rle_counts_numpy(pm, H, W)
    assert _invalid(*enc(out=runs, cap=8)) and total.value == len(want[1]) and np.array_equal(run_ptr, want[0])
    _lib.call(*enc())                                                              # sizes only
    assert total.value == len(want[1])

    from mnc_amd.engine import _Ctx
    ctx = _Ctx(0)
    try:
        d_rle = ctypes.c_void_p()
        for rows, h, w in ((-1, H, W), (2049, H, W), (4, 0, W), (4, H, 32769)):
            assert _invalid("mnc_mask_rle_dev", ctx.h, 256, 256, rows, h, w, 16, ctypes.addressof(d_rle))
    finally:
        ctx.close()

    ptr, counts = np.array([0, 1, 3], np.int64), np.array([H * W, 0, H * W], np.uint32)
    bounds, offsets, areas, need = np.zeros((2, 4), np.int32), np.zeros(2, np.int64), np.zeros(2, np.int64), ctypes.c_size_t(0)
    bits = np.zeros(H * 4, np.uint64)

    def dec(p=ptr, c=counts, count=2, h=H, w=W, out=None, cap=0):
        return ("mnc_mask_from_rle", _lib.ptr(p), _lib.ptr(c), count, h, w, _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas),
                _lib.ptr(out), cap, ctypes.addressof(need), 0)

    assert _invalid(*dec(count=-1)) and _invalid(*dec(count=2049)) and _invalid(*dec(h=0)) and _invalid(*dec(w=32769))
    assert _invalid(*dec(p=np.array([-1, 0, 2], np.int64))) and _invalid(*dec(p=np.array([0, 2, 1], np.int64)))
    assert _invalid(*dec(c=np.array([H * W, 1, H * W], np.uint32)))                # sums to H * W + 1
    assert _invalid(*dec(c=np.array([H * W - 1, 0, H * W], np.uint32)))            # ... to H * W - 1
    assert _invalid(*dec(p=np.array([0, 0, 3], np.int64)))                         # a mask without counts
    assert _invalid(*dec(out=bits, cap=bits.nbytes - 8)) and need.value == bits.nbytes     # checked after the bounds pass
    _lib.call(*dec(out=bits, cap=bits.nbytes))
    assert bounds.tolist() == [[0, 0, -1, -1], [0, 0, W - 1, H - 1]] and areas.tolist() == [0, H * W] and offsets.tolist() == [0, 0]
    assert (bits.reshape(H, 4)[:, :3] == np.uint64(2 ** 64 - 1)).all() and (bits.reshape(H, 4)[:, 3] == np.uint64(255)).all()


def test_demo_save_coco_writes_the_results_file(tmp_path):
    import glob
    import io
    import json
    from contextlib import redirect_stdout

    import demo
    from mnc_amd import models
    jpg = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "demo", "*.jpg")))[0]
    proto = models.write_mnc_5stage_test_prototxt(width_div=8)
    out = str(tmp_path / "results.json")
    with redirect_stdout(io.StringIO()) as buf:
        demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-coco", out, "--save-masks", str(tmp_path), "--vis-thresh", "0.0"])
    assert out in buf.getvalue()
    name = os.path.splitext(os.path.basename(jpg))[0]
    pm = PackedMasks.load(str(tmp_path / (name + "_masks.npz")))                  # the same instances, as --save-masks wrote them
    im = demo._read_image_bgr(jpg)
    with open(out) as f:
        got = json.load(f)
    want = demo._coco_results(name, im.shape, pm, cpu=True)                        # --cpu: the numpy statement
    assert len(got) == len(pm) > 0 and got == json.loads(json.dumps(want))
    back = PackedMasks.from_rle([e["segmentation"] for e in got])
    h, w = im.shape[:2]
    assert all(np.array_equal(back.full(i, h, w), pm.full(i, h, w)) for i in range(len(pm)))
