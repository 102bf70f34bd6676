"""The moments, convex hulls, rectangles of least area and diameters of packed instance masks on the GPU (csrc/mask_shape.hip:
mnc_mask_moments, mnc_mask_hull, mnc_mask_oriented and the Python surfaces over them) against the numpy statements
(mnc_amd.shape.moments_numpy, hull_numpy, oriented_numpy, which tests/test_mask_shape_host.py pins to scipy, to exact fractions, to
a brute force and to closed forms).  Every comparison is exact, field by field, dtype and shape included, and every call is made
twice: the bytes are equal.  The sets are those of tests/mask_shape_inputs.py.  The implementation keeps the chains of candidates
in the workspace whatever their height, so the 4097-row instance takes the path every other one takes: there is no cap to be
beyond."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import mask_shape_inputs as SI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import shape as SH  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY32 = 0x55555555
CANARY64 = 0x5555555555555555


def _bytes(t):
    return [a.tobytes() for a in t]


def _all(name):
    """Every device call on that set, twice, against the statements -> (Moments, Hulls, OrientedBoxes)."""
    pm = SI.get(name)
    got = []
    for what, call in (("moments", SH.moments), ("hull", SH.hull), ("oriented", SH.oriented)):
        first = call(pm)
        assert SI.same_arrays(first, SI.reference(name, what)), what
        assert _bytes(call(pm)) == _bytes(first), what
        got.append(first)
    # mnc_mask_oriented names edges and vertices of the hull mnc_mask_hull gives
    assert SI.same_arrays(SH.oriented_numpy(pm, got[1]), got[2])
    return got


# ---- the sets ----

def test_word_boundary_widths_and_heights_with_negative_bounds_and_dirty_padding():
    pm = SI.get("sizes")
    assert set(SI.WIDTHS) == set((pm.bounds[:, 2] - pm.bounds[:, 0] + 1).tolist())
    assert set(SI.HEIGHTS) == set((pm.bounds[:, 3] - pm.bounds[:, 1] + 1).tolist())
    assert (pm.bounds[:, 0] < 0).any() and (pm.bounds[:, 1] < 0).all()
    clean = SI.sizes_set(dirty=False)
    assert not np.array_equal(clean.bits, pm.bits)                     # the padding bits of the set are ones
    mom, hulls, boxes = _all("sizes")
    assert SI.same_arrays(SH.moments(clean), mom) and SI.same_arrays(SH.hull(clean), hulls) and SI.same_arrays(SH.oriented(clean), boxes)
    assert np.array_equal(mom.m[:, 0], pm.areas)


def test_staircase_disc_specks_gaps_and_empty_instances():
    pm = SI.get("shapes")
    mom, hulls, boxes = _all("shapes")
    count = np.diff(hulls.vert_ptr).tolist()
    assert count[:3] == [4, 4, 6] and count[3] == 64 and count[4] == 6           # pixel, rectangle, staircase, disc, specks
    assert count[6:10] == [4, 0, 0, 4] and not mom.m[7:9].any() and not boxes.box[7:9].any() and not boxes.diameter[7:9].any()
    assert hulls.area2[6:10].tolist() == [40, 0, 0, 780]
    rows = set((hulls.vertices(5)[:, 1] - pm.bounds[5, 1]).tolist())             # the gaps: no vertex on an empty lattice row
    assert rows <= {3, 6, 12, 14}
    inner = hulls.vertices(10)[:, 1] - pm.bounds[10, 1]
    assert inner.min() == 1 and inner.max() == 29                                # empty first and last rows
    assert boxes.diameter[4, 0] == 70 * 70 + 50 * 50


def test_discs_cross_a_wave_and_a_workgroup_of_edges():
    _, hulls, boxes = _all("discs")
    count = np.diff(hulls.vert_ptr)
    assert count[0] == 64 and 64 < count[1] <= 256 < count[2]
    assert ((boxes.box[:, 0] >= 0) & (boxes.box[:, 0] < count // 4)).all()       # a quarter turn ties: the lowest edge wins


def test_more_than_one_grid_row_of_workgroups_and_no_instance():
    assert len(SI.get("many130")) == 130 and len(SI.get("empty")) == 0
    _all("many130")
    mom, hulls, boxes = _all("empty")
    assert mom.m.shape == (0, 6) and hulls.vert_ptr.tolist() == [0] and hulls.xy.shape == (0, 2) and boxes.box.shape == (0, 8)


def test_a_hundred_instances_of_an_image_through_every_surface():
    pm = SI.get("real")
    assert len(pm) == 100
    mom, hulls, boxes = _all("real")
    assert SI.same_arrays(pm.moments(), mom) and SI.same_arrays(MT.mask_moments(pm), mom)
    assert SI.same_arrays(pm.hull(), hulls) and SI.same_arrays(MT.mask_hull(pm), hulls)
    assert SI.same_arrays(pm.oriented_boxes(), boxes) and SI.same_arrays(MT.mask_oriented_boxes(pm), boxes)
    want = hulls.solidity(pm.areas)
    assert np.array_equal(pm.solidity(), want) and np.array_equal(MT.mask_solidity(pm), want)
    assert ((want > 0) & (want <= 1)).sum() == (pm.areas > 0).sum()


def test_an_instance_4097_rows_tall():
    pm = SI.get("tall")
    assert pm.size(0) == (SI.TALL, 3) and SI.TALL > 4096
    _, hulls, _ = _all("tall")
    assert np.diff(hulls.vert_ptr).tolist() == [6, 4]


def test_a_row_of_32768_columns_at_the_edge_of_the_coordinate_range():
    mom, hulls, boxes = _all("wide")
    assert hulls.area2.tolist() == [2 * 2 * 32768] and boxes.diameter[0, 0] == 32768 ** 2 + 4


# ---- buffers ----

def test_hull_sizes_only_room_to_spare_and_too_little_room():
    pm = SI.get("shapes")
    want = SI.reference("shapes", "hull")
    n, total = len(pm), int(want.vert_ptr[-1])
    # sizes only: vert_ptr and the count, nothing else
    vert_ptr, size = SH.hull_call(pm, None, None)
    assert size == total and np.array_equal(vert_ptr, want.vert_ptr)
    area2, count = np.full(n + 2, CANARY64, np.int64), ctypes.c_size_t(0)
    vp = np.full(n + 3, CANARY64, np.int64)
    _lib.call("mnc_mask_hull", *(_set_args(pm, areas=False) + (_lib.ptr(vp), None, _lib.ptr(area2), 0, ctypes.addressof(count), 0)))
    assert count.value == total and np.array_equal(vp[:n + 1], want.vert_ptr) and (vp[n + 1:] == CANARY64).all()
    assert (area2 == CANARY64).all()
    # room to spare
    xy, area2 = np.full((total + 5, 2), CANARY32, np.int32), np.full(n + 2, CANARY64, np.int64)
    vert_ptr, size = SH.hull_call(pm, xy, area2)
    assert size == total and np.array_equal(vert_ptr, want.vert_ptr)
    assert np.array_equal(xy[:total], want.xy) and (xy[total:] == CANARY32).all()
    assert np.array_equal(area2[:n], want.area2) and (area2[n:] == CANARY64).all()
    # too little room: vert_ptr and the count, and nothing else
    xy, area2 = np.full((total - 1, 2), CANARY32, np.int32), np.full(n, CANARY64, np.int64)
    vp, count = np.zeros(n + 1, np.int64), ctypes.c_size_t(0)
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_mask_hull", *(_set_args(pm, areas=False) + (_lib.ptr(vp), _lib.ptr(xy), _lib.ptr(area2), total - 1,
                                                                   ctypes.addressof(count), 0)))
    assert e.value.code == INVALID and count.value == total and np.array_equal(vp, want.vert_ptr)
    assert (xy == CANARY32).all() and (area2 == CANARY64).all()


def test_moments_and_oriented_write_their_rows_and_nothing_behind_them():
    pm = SI.get("shapes")
    n = len(pm)
    m = np.full((n + 2, 6), CANARY64, np.int64)
    _lib.call("mnc_mask_moments", *(_set_args(pm, areas=False) + (_lib.ptr(m), 0)))
    assert np.array_equal(m[:n], SI.reference("shapes", "moments").m) and (m[n:] == CANARY64).all()
    box, diameter = np.full((n + 2, 8), CANARY64, np.int64), np.full((n + 2, 3), CANARY64, np.int64)
    _lib.call("mnc_mask_oriented", *(_set_args(pm, areas=False) + (_lib.ptr(box), _lib.ptr(diameter), 0)))
    want = SI.reference("shapes", "oriented")
    assert np.array_equal(box[:n], want.box) and (box[n:] == CANARY64).all()
    assert np.array_equal(diameter[:n], want.diameter) and (diameter[n:] == CANARY64).all()
    # a set none of whose instances has a row is answered on the host, with zeros
    none = pm.take([8, 8])
    assert not SH.moments(none).m.any() and not SH.oriented(none).box.any() and SH.hull(none).vert_ptr.tolist() == [0, 0, 0]


# ---- invalid arguments ----

def _refused(pm, null=None, n=None):
    """All three entries refuse that set (or a null pointer in the place `null` names) and write nothing."""
    n = len(pm) if n is None else n
    args = _set_args(pm, areas=False)[:4] + (n,)
    rows = max(n, 1)
    m = np.full((rows, 6), CANARY64, np.int64)
    vp, xy, area2 = np.full(rows + 1, CANARY64, np.int64), np.full((64, 2), CANARY32, np.int32), np.full(rows, CANARY64, np.int64)
    box, diameter, count = np.full((rows, 8), CANARY64, np.int64), np.full((rows, 3), CANARY64, np.int64), ctypes.c_size_t(12345)
    p = {"m": _lib.ptr(m), "vp": _lib.ptr(vp), "xy": _lib.ptr(xy), "area2": _lib.ptr(area2), "box": _lib.ptr(box),
         "diameter": _lib.ptr(diameter), "count": ctypes.addressof(count)}
    if null is not None:
        p[null] = None
    calls = {"mnc_mask_moments": ("m", (p["m"], 0)),
             "mnc_mask_hull": ("vp area2 count", (p["vp"], p["xy"], p["area2"], 64, p["count"], 0)),
             "mnc_mask_oriented": ("box diameter", (p["box"], p["diameter"], 0))}
    for name, (takes, tail) in calls.items():
        if null is not None and null not in takes.split():
            continue
        with pytest.raises(_lib.MncError) as e:
            _lib.call(name, *(args + tail))
        assert e.value.code == INVALID, name
    for a in (m, vp, area2, box, diameter):
        assert (a == CANARY64).all()
    assert (xy == CANARY32).all() and count.value == 12345
    return True


def test_invalid_sets_and_null_pointers_are_refused_and_nothing_is_written():
    pm = SI.get("many130").take([0, 1, 2])
    for null in ("m", "vp", "area2", "count", "box", "diameter"):
        assert _refused(pm, null)
    wide = PackedMasks([[0, 0, 32768, 0]], [0], [0], None, None, np.zeros(513, np.uint64))        # 32769 columns
    high = PackedMasks([[5, -9, 5, 32759]], [0], [0], None, None, np.zeros(32769, np.uint64))      # 32769 rows
    assert _refused(wide) and _refused(high)
    for what in (SH.moments_numpy, SH.hull_numpy, SH.oriented_numpy):
        for bad in (wide, high):
            with pytest.raises(ValueError):
                what(bad)
    ok = PackedMasks([[0, 0, 32767, 0]], [0], [0], None, None, np.zeros(512, np.uint64))           # 32768 columns are taken
    assert not SH.moments(ok).m.any()
    for offset in (4, -8, 8 * 10 ** 6):                                                            # a bad offset
        bad = PackedMasks(pm.bounds, [int(pm.offsets[0]), offset, int(pm.offsets[2])], pm.areas, None, None, pm.bits)
        assert _refused(bad)
    big = np.zeros((2049, 4), np.int32)
    big[:, 2:] = -1
    assert _refused(PackedMasks(big, np.zeros(2049, np.int64), np.zeros(2049, np.int64), None, None, np.zeros(0, np.uint64)))
    assert _refused(PackedMasks([[2 ** 24, 0, 2 ** 24 + 3, 4]], [0], [0], None, None, np.zeros(8, np.uint64)))


# ---- the demo ----

def test_demo_oriented_boxes_writes_rbox_and_solidity(tmp_path):
    import glob
    import io
    import json
    from contextlib import redirect_stdout

    import demo
    from mnc_amd import models
    jpg = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "demo", "*.jpg")))[0]
    proto = models.write_mnc_5stage_test_prototxt(width_div=8)
    name = os.path.splitext(os.path.basename(jpg))[0]
    got, saved = {}, {}
    for key, flags in (("plain", []), ("boxes", ["--oriented-boxes"]), ("boxes_cpu", ["--oriented-boxes", "--cpu"])):
        out = str(tmp_path / (key + ".json"))
        os.makedirs(str(tmp_path / key))
        with redirect_stdout(io.StringIO()):
            demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-annotations", out, "--save-masks", str(tmp_path / key),
                       "--vis-thresh", "0.0"] + flags)
        with open(out) as f:
            got[key] = json.load(f)["annotations"]
        saved[key] = PackedMasks.load(str(tmp_path / key / (name + "_masks.npz")))
    pm = saved["boxes"]
    assert len(pm) > 0 and len(got["boxes"]) == len(got["plain"]) > 0
    assert not any("rbox" in a or "solidity" in a for a in got["plain"])
    hulls = SH.hull_numpy(pm)
    rbox, solid = SH.oriented_numpy(pm, hulls).rbox(), hulls.solidity(pm.areas)
    assert len(pm) == len(got["boxes"]) and (hulls.area2 > 0).any()
    for i, a in enumerate(got["boxes"]):
        assert a["rbox"] == ([float(v) for v in rbox[i]] if hulls.area2[i] else None) and a["solidity"] == float(solid[i])
    assert got["boxes_cpu"] == got["boxes"]
    assert [{k: v for k, v in a.items() if k not in ("rbox", "solidity")} for a in got["boxes"]] == got["plain"]
