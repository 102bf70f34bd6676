"""The set algebra of packed instance masks on the GPU (csrc/mask_algebra.hip: mnc_mask_combine, mnc_mask_merge, mnc_mask_layer and
the Python surfaces over them) against the numpy statements (mnc_amd.algebra.combine_numpy, merge_numpy, layer_numpy, which
tests/test_mask_algebra_host.py pins to dense arithmetic, inclusion-exclusion, De Morgan and closed forms).  Every comparison is
exact, field by field, dtype and shape included.  The sets are those of tests/mask_algebra_inputs.py; that the word-boundary pairs
can fail is asserted of the numpy statement in the host test."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import mask_algebra_inputs as AI  # noqa: E402
import render_inputs as RI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import algebra as AL  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, InstanceBlock, records_from_lists  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY = np.uint64(0x5555555555555555)


def _combine(name, op, window=None):
    s = AI.get(name)
    a, b = s if isinstance(s, tuple) else (s, None)
    got = AL.combine(a, b, op, window)
    assert AI.same_masks(got, AI.combined(name, op, window))
    return got


# ---- the word-boundary pairs ----

@pytest.mark.parametrize("op", AI.OPS)
def test_word_boundary_pairs(op):
    got = _combine("word", op, (-100, -3, 300, 30) if op == "not" else None)
    assert got.areas.any() and AI.canonical(got)


# ---- bounds relations ----

@pytest.mark.parametrize("op", AI.OPS)
def test_bounds_relations(op):
    got = _combine("relation", op, (-20, -12, 180, 52) if op == "not" else None)
    assert got.areas.any()
    if op == "and":
        assert got.areas[[0, 1, 5, 8, 9, 10, 11, 12, 13, 14]].tolist() == [0] * 10


@pytest.mark.parametrize("op", AI.BINARY)
def test_one_instance_against_every_instance(op):
    a, b = AI.get("broadcast")
    assert len(b) == 1
    _combine("broadcast", op)


# ---- untrusted padding ----

@pytest.mark.parametrize("op", AI.OPS)
def test_set_padding_bits_change_nothing(op):
    window = (-100, -3, 300, 30) if op == "not" else None
    clean, dirty = AI.get("word"), AI.get("word_dirty")
    assert not np.array_equal(clean[0].bits, dirty[0].bits) and np.array_equal(clean[0].bounds, dirty[0].bounds)
    got = AL.combine(dirty[0], dirty[1], op, window)
    assert AI.same_masks(got, AI.combined("word", op, window))


# ---- windows ----

@pytest.mark.parametrize("window", AI.WINDOWS)
def test_windows_cut_at_and_inside_a_word(window):
    got = _combine("window", "copy", window)
    assert got.areas.any() and (got.bounds[got.areas > 0, 0] >= window[0]).all() and (got.bounds[:, 2] <= window[2]).all()
    pm = AI.get("window")
    assert AI.same_masks(AL.combine(pm, pm.take([4]), "xor", window), AL.combine_numpy(pm, pm.take([4]), "xor", window))


@pytest.mark.parametrize("window", AI.NOT_WINDOWS)
def test_complement_in_a_window(window):
    got = _combine("window", "not", window)
    pixels = (window[2] - window[0] + 1) * (window[3] - window[1] + 1)
    assert got.areas[5] == pixels and (got.areas <= pixels).all()


def test_a_window_disjoint_from_everything():
    got = _combine("window", "copy", AI.FAR_WINDOW)
    assert not got.areas.any() and got.bits.size == 0 and (got.bounds == (0, 0, -1, -1)).all()


# ---- merge ----

@pytest.mark.parametrize("intersect", [False, True])
def test_merge_groups(intersect):
    pm, groups = AI.get("crowd"), AI.crowd_groups()
    assert [len(g) for g in groups][:6] == [0, 1, 2, 64, 65, 200]
    csr = AL.groups_csr(groups)
    want = AI.reference(("crowd", "merge", intersect), lambda: AL.merge_numpy(pm, *csr, intersect=intersect))
    got = AL.merge(pm, *csr, intersect=intersect)
    assert AI.same_masks(got, want) and got.areas[0] == 0
    if not intersect:
        assert (got.areas[1:8] > 0).all() and np.array_equal(got.bounds[3], got.bounds[7]) and got.areas[3] == got.areas[7]


def test_intersecting_nested_rectangles_gives_the_innermost():
    pm = AI.get("nested_up")
    got = AL.merge(pm, *AL.groups_csr([np.arange(65), np.arange(64, -1, -1), [0, 10]]), intersect=True)
    assert got.bounds.tolist() == [pm.bounds[64].tolist()] * 2 + [pm.bounds[10].tolist()]
    assert got.areas.tolist() == [int(AI.nested_areas()[64])] * 2 + [int(AI.nested_areas()[10])]
    assert AI.canonical(got)


def test_merge_without_groups():
    got = AL.merge(AI.get("crowd"), np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert AI.same_masks(got, AL.merge_numpy(AI.get("crowd"), np.zeros(1, np.int64), np.zeros(0, np.int32))) and len(got) == 0


# ---- layer ----

def test_layering_nested_rectangles_gives_rings_or_one_survivor():
    areas = AI.nested_areas()
    up = AL.layer(AI.get("nested_up"))
    assert AI.same_masks(up, AI.reference(("nested_up", "layer"), lambda: AL.layer_numpy(AI.get("nested_up"))))
    assert up.areas.tolist() == (areas - np.append(areas[1:], 0)).tolist()
    down = AL.layer(AI.get("nested_down"))
    assert AI.same_masks(down, AI.reference(("nested_down", "layer"), lambda: AL.layer_numpy(AI.get("nested_down"))))
    assert down.areas.tolist() == [int(areas[0])] + [0] * 64


def test_layering_equal_scores_an_explicit_order_and_one_instance():
    pm = AI.get("equal")
    got = AL.layer(pm)
    assert AI.same_masks(got, AL.layer_numpy(pm)) and got.areas[0] == pm.areas[0]
    order = np.array([5, 2, 7, 0, 1, 6, 3, 4], np.int32)
    got = AL.layer(pm, order)
    assert AI.same_masks(got, AL.layer_numpy(pm, order)) and got.areas[5] == pm.areas[5] and got.areas[0] < pm.areas[0]
    one = pm.take([3])
    assert AI.same_masks(AL.layer(one), AL.combine_numpy(one, None, "copy"))


def test_layering_three_hundred_blobs():
    pm = AI.get("blobs")
    got = AL.layer(pm)
    assert AI.same_masks(got, AI.reference(("blobs", "layer"), lambda: AL.layer_numpy(pm)))
    assert (got.areas < pm.areas).sum() > 100 and (got.areas == 0).sum() > 5


# ---- more instances than a scan tile ----

def test_1025_instances_cross_the_size_kernels_blocks_and_the_scans_tile():
    a, b = AI.get("edge")
    assert len(a) == 1025 and len(b) == 1
    sizes = [a.size(i) for i in range(len(a))]
    assert sum(h * w == 0 for h, w in sizes) == 146 and max(sizes) == (3, 65) and sum(w == 65 for h, w in sizes) > 100
    tight = _combine("edge", "copy")
    assert AI.canonical(tight) and (tight.areas[[h * w > 0 for h, w in sizes]] == 0).sum() > 50           # rows, and no pixel
    assert tight.areas[1024] > 0 and tight.offsets[1024] > tight.offsets[1023] > 0           # the second tile begins behind the first
    both = _combine("edge", "or")
    assert AI.canonical(both) and (both.areas >= b.areas[0]).all()


# ---- the C ABI ----

def _combine_call(a, b, op, window, bits, bounds=None, cap=None):
    """mnc_mask_combine as it is -> (status, bound, used, bounds, offsets, areas)."""
    n = len(a)
    bounds = np.full((n, 4), 77, np.int32) if bounds is None else bounds
    offsets, areas = np.full(n, 77, np.int64), np.full(n, 77, np.int64)
    bound, used = ctypes.c_size_t(12345), ctypes.c_size_t(54321)
    win = None if window is None else np.array(window, np.int32)
    args_b = (None, None, None, 0, 0) if b is None else _set_args(b, areas=False)
    rc = getattr(_lib.load(), "mnc_mask_combine")(*(_set_args(a, areas=False) + args_b + (
        int(op), _lib.ptr(win), _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits),
        (bits.nbytes if bits is not None else 0) if cap is None else cap, ctypes.addressof(bound), ctypes.addressof(used), 0)))
    return rc, bound.value, used.value, bounds, offsets, areas


def test_the_size_call_launches_nothing_and_returns_the_bound():
    a, b = AI.get("word")
    AL.timing(True)
    try:
        rc, bound, used, bounds, offsets, areas = _combine_call(a, b, 1, None, None)
        assert rc == 0 and used == 54321 and (bounds == 77).all() and (offsets == 77).all() and (areas == 77).all()
        assert AL.timing(True) == -1.0                       # no launch was timed
        want = 0
        for i in range(len(a)):
            f = AL._hull(AL._box(a, i), AL._box(b, i))
            want += (f[3] - f[1] + 1) * ((f[2] - f[0] + 1 + 63) // 64) * 8
        assert bound == want
        bits = np.full(bound // 8, CANARY, np.uint64)
        rc, bound2, used, *_ = _combine_call(a, b, 1, None, bits)
        assert rc == 0 and bound2 == bound and used == AI.combined("word", "or").bits.nbytes < bound
        assert AL.timing(False) > 0.0
    finally:
        AL.timing(False)


def test_bytes_past_the_result_and_past_the_room_are_never_written():
    a, b = AI.get("word")
    want = AI.combined("word", "xor")
    bound = _combine_call(a, b, 2, None, None)[1]
    bits = np.full(bound // 8 + 16, CANARY, np.uint64)
    rc, _, used, bounds, offsets, areas = _combine_call(a, b, 2, None, bits, cap=bound)
    assert rc == 0 and used == want.bits.nbytes
    assert np.array_equal(bits[:used // 8], want.bits) and (bits[used // 8:] == CANARY).all()
    assert np.array_equal(bounds, want.bounds) and np.array_equal(offsets, want.offsets) and np.array_equal(areas, want.areas)
    # too little room: only the bound is set
    bits[:] = CANARY
    rc, bound2, used, bounds, offsets, areas = _combine_call(a, b, 2, None, bits, cap=bound - 8)
    assert rc == INVALID and bound2 == bound and used == 54321 and (bits == CANARY).all()
    assert (bounds == 77).all() and (offsets == 77).all() and (areas == 77).all()


def _refused(entry, args):
    """The call returns MNC_ERR_INVALID and writes nothing into its outputs."""
    n = 8
    bounds, offsets, areas = np.full((n, 4), 77, np.int32), np.full(n, 77, np.int64), np.full(n, 77, np.int64)
    bits = np.full(4096, CANARY, np.uint64)
    bound, used = ctypes.c_size_t(12345), ctypes.c_size_t(54321)
    rc = getattr(_lib.load(), entry)(*(args + (_lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits), bits.nbytes,
                                               ctypes.addressof(bound), ctypes.addressof(used), 0)))
    assert rc == INVALID, (entry, rc)
    assert (bounds == 77).all() and (offsets == 77).all() and (areas == 77).all() and (bits == CANARY).all()
    assert bound.value == 12345 and used.value == 54321
    return True


def test_every_invalid_argument_is_refused_before_a_launch():
    pm = AI.get("equal")                                     # eight instances of 100 x 30
    sa = _set_args(pm, areas=False)
    none = (None, None, None, 0, 0)
    keep = [np.array(w, np.int32) for w in ((0, 0, 1 << 24, 5), (5, 5, 4, 9), (5, 5, 9, 4), (0, 0, 9, 9))]
    # combine
    assert _refused("mnc_mask_combine", sa + sa + (6, None))
    assert _refused("mnc_mask_combine", sa + sa + (-1, None))
    assert _refused("mnc_mask_combine", sa + _set_args(pm.take([0, 1]), areas=False) + (1, None))        # n_b outside {0, 1, n_a}
    for op in range(4):
        assert _refused("mnc_mask_combine", sa + none + (op, None))                                      # an op that needs b
    assert _refused("mnc_mask_combine", sa + none + (5, None))                                           # not without a window
    for k in range(3):
        assert _refused("mnc_mask_combine", sa + none + (4, _lib.ptr(keep[k])))                          # |c| >= 2^24; empty windows
    far = PackedMasks(np.array([[0, 0, 9, 9], [1 << 23, 1 << 23, (1 << 23) + 9, (1 << 23) + 9]], np.int32), [0, 80], [0, 0], None, None,
                      np.zeros(20, np.uint64))
    assert _refused("mnc_mask_combine", _set_args(far.take([0]), areas=False) + _set_args(far.take([1]), areas=False) + (1, None))
    # what mnc_mask_boundary refuses about a set
    bad = PackedMasks(pm.bounds, pm.offsets + 4, pm.areas, None, None, pm.bits)
    assert _refused("mnc_mask_combine", _set_args(bad, areas=False) + none + (4, None))
    short = (_lib.ptr(pm.bounds), _lib.ptr(pm.offsets), _lib.ptr(pm.bits), pm.bits.nbytes - 8, len(pm))
    assert _refused("mnc_mask_combine", short + none + (4, None))
    assert _refused("mnc_mask_combine", (None,) + sa[1:] + none + (4, None))
    wide = PackedMasks(np.array([[-(1 << 24), 0, 5, 5]], np.int32), [0], [0], None, None, np.zeros(8, np.uint64))
    assert _refused("mnc_mask_combine", _set_args(wide, areas=False) + none + (4, None))
    # merge
    members = np.arange(8, dtype=np.int32)
    gp = lambda *v: np.array(v, np.int64)                    # noqa: E731
    for group_ptr, mem, G in ((gp(1, 8), members, 1), (gp(0, 5, 3), members, 2), (gp(0, 8), None, 1), (None, members, 1),
                              (gp(0, 8), np.array([0, 1, 2, 3, 4, 5, 6, 8], np.int32), 1),
                              (gp(0, 8), np.array([0, 1, 2, -1, 4, 5, 6, 7], np.int32), 1), (gp(0, 8), members, -1),
                              (gp(0, (1 << 20) + 1), members, 1)):
        assert _refused("mnc_mask_merge", sa + (_lib.ptr(group_ptr), _lib.ptr(mem), G, 0)), (group_ptr, G)
    # layer
    scores = pm.scores.copy()
    assert _refused("mnc_mask_layer", sa + (None, None))
    assert _refused("mnc_mask_layer", sa + (_lib.ptr(scores), _lib.ptr(np.array([0, 1, 2, 3, 4, 5, 6, 6], np.int32))))
    assert _refused("mnc_mask_layer", sa + (_lib.ptr(scores), _lib.ptr(np.array([0, 1, 2, 3, 4, 5, 6, 8], np.int32))))
    scores[3] = np.nan
    assert _refused("mnc_mask_layer", sa + (_lib.ptr(scores), None))
    # null outputs
    bound = ctypes.c_size_t(0)
    lib = _lib.load()
    assert lib.mnc_mask_combine(*(sa + none + (4, None, None, None, None, None, 0, None, None, 0))) == INVALID
    one = np.zeros(1 << 12, np.uint64)
    assert lib.mnc_mask_combine(*(sa + none + (4, None, None, None, None, _lib.ptr(one), one.nbytes, ctypes.addressof(bound), None,
                                               0))) == INVALID


def test_more_than_2_27_pixels_of_loose_frames_are_refused():
    a = PackedMasks(np.array([[0, 0, 9, 9]] * 3, np.int32), [0, 80, 160], [0, 0, 0], None, None, np.zeros(30, np.uint64))
    b = PackedMasks(np.array([[8000, 8000, 8009, 8009]] * 3, np.int32), [0, 80, 160], [0, 0, 0], None, None, np.zeros(30, np.uint64))
    assert _refused("mnc_mask_combine", _set_args(a, areas=False) + _set_args(b, areas=False) + (1, None))
    with pytest.raises(ValueError):
        AL.combine_numpy(a, b, "or")
    got = AL.combine(a, b, "and")                            # the intersections are empty: answered on the host
    assert AI.same_masks(got, AL.combine_numpy(a, b, "and")) and got.bits.size == 0


def test_empty_sets():
    e = AI.get("empty")
    for op in AI.OPS:
        got = AL.combine(e, e, op, (0, 0, 5, 5) if op == "not" else None)
        assert AI.same_masks(got, AL.combine_numpy(e, e, op, (0, 0, 5, 5) if op == "not" else None)) and len(got) == 0
    assert AI.same_masks(AL.layer(e), AL.layer_numpy(e))
    assert AI.same_masks(e.merge(), AL.merge_numpy(e, np.array([0, 0]), np.zeros(0, np.int32))) and len(e.merge()) == 1
    a, _ = AI.get("relation")
    rowless = a.take([8, 10, 11])
    assert AI.same_masks(rowless.tighten(), AL.combine_numpy(rowless, None, "copy"))


# ---- determinism ----

def test_two_calls_give_the_same_bytes():
    a, b = AI.get("word")
    pm = AI.get("blobs")
    for call in (lambda: AL.combine(a, b, "xor"), lambda: AL.layer(pm), lambda: pm.merge(by="class")):
        x, y = call(), call()
        for f in PackedMasks.FIELDS:
            assert getattr(x, f).tobytes() == getattr(y, f).tobytes(), f


# ---- the Python surface ----

def test_operators_and_methods():
    a, b = AI.get("word")
    for got, op in ((a & b, "and"), (a | b, "or"), (a ^ b, "xor"), (a - b, "minus"), (a.combine(b, "xor"), "xor"),
                    (a.tighten(), "copy")):
        assert AI.same_masks(got, AI.combined("word", op)), op
    assert AI.same_masks(a.crop(-100, -3, 300, 30), AI.combined("word", "copy", (-100, -3, 300, 30)))
    pm = AI.get("window")
    H, W = AI.IMAGE_H, AI.IMAGE_W
    assert AI.same_masks(pm.complement(H, W), AI.combined("window", "not", (0, 0, W - 1, H - 1)))
    crowd = AI.get("crowd")
    distinct, groups = AL.class_groups(crowd.classes)
    per_class = crowd.merge(by="class")
    assert AI.same_masks(per_class, AL.merge_numpy(crowd, *AL.groups_csr(groups))) and per_class.classes.tolist() == distinct.tolist()
    assert AI.same_masks(crowd.merge(), AL.merge_numpy(crowd, *AL.groups_csr([np.arange(len(crowd))])))
    assert AI.same_masks(crowd.merge([[3, 4], [5]], intersect=True), AL.merge_numpy(crowd, *AL.groups_csr([[3, 4], [5]]), intersect=True))
    assert AI.same_masks(crowd.layered(), AI.reference(("crowd", "layer"), lambda: AL.layer_numpy(crowd)))
    with pytest.raises(ValueError):
        crowd.merge(by="score")
    with pytest.raises(ValueError):
        a.combine(b, "nor")
    with pytest.raises(_lib.MncError):
        a.combine(b.take([0, 1]), "or")


def test_the_mask_transform_wrappers():
    a, b = AI.get("word")
    crowd = AI.get("crowd")
    assert AI.same_masks(MT.mask_combine(a, b, "minus"), AI.combined("word", "minus"))
    assert AI.same_masks(MT.mask_combine(a, None, "copy", (-100, -3, 300, 30)), AI.combined("word", "copy", (-100, -3, 300, 30)))
    assert AI.same_masks(MT.mask_merge(crowd, [[1, 2, 3]]), AL.merge_numpy(crowd, *AL.groups_csr([[1, 2, 3]])))
    assert AI.same_masks(MT.mask_layered(crowd), AI.reference(("crowd", "layer"), lambda: AL.layer_numpy(crowd)))


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


def test_layered_on_a_fetched_device_resident_result():
    rng = np.random.default_rng(73)
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
        got = pm.layered()
        assert AI.same_masks(got, AL.layer_numpy(flat)) and (got.areas < flat.areas).any()
        inter, _ = got.overlaps()
        assert not (inter - np.diag(np.diagonal(inter))).any()
        assert AI.same_masks(pm | pm, AL.combine_numpy(flat, None, "copy"))
    finally:
        blk.release()
        ctx.close()


# ---- the demo ----

def test_demo_exclusive_writes_layered_masks(tmp_path):
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
    for key, flags in (("plain", []), ("exclusive", ["--exclusive"]), ("exclusive_cpu", ["--exclusive", "--cpu"])):
        out = str(tmp_path / (key + ".json"))
        os.makedirs(str(tmp_path / key))
        with redirect_stdout(io.StringIO()):
            demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-coco", out, "--save-masks", str(tmp_path / key),
                       "--vis-thresh", "0.0"] + flags)
        with open(out) as f:
            got[key] = json.load(f)
        saved[key] = PackedMasks.load(str(tmp_path / key / (name + "_masks.npz")))
    pm = saved["plain"]
    assert len(pm) > 1
    want = AL.layer_numpy(pm)
    assert AI.same_masks(saved["exclusive"], want) and AI.same_masks(saved["exclusive_cpu"], want)   # --cpu: the numpy statement
    assert (want.areas < pm.areas).any() and got["exclusive_cpu"] == got["exclusive"]
    assert got["exclusive"] == json.loads(json.dumps(demo._coco_results(name, im.shape, want, cpu=True)))
