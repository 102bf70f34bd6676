"""Outlines of packed instance masks on the GPU (csrc/mask_contours.hip: mnc_mask_contours and the Python surfaces over it) against
the numpy statement mnc_amd.contours.contours_numpy, which tests/test_mask_contours_host.py pins to closed forms, to the polygon
rasteriser and to scipy.ndimage.  Every comparison is exact: dtype, shape and bytes.  The shapes are those of
tests/mask_contours_inputs.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_contours_inputs as TI  # noqa: E402
import mask_overlap_inputs as MI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
FILL = 0x5a
OTHER = {4: 8, 8: 4}


@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(TI.SETS))
def test_contours_equal_the_statement(name, connectivity):
    got = CT.contours(TI.get(name), connectivity)
    want = TI.reference(name, connectivity)
    assert got.loop_ptr.tolist() == want.loop_ptr.tolist()
    assert got.vert_ptr.tolist() == want.vert_ptr.tolist() and got.area.tolist() == want.area.tolist()
    assert TI.same_contours(got, want)


@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
def test_stripes_whose_edges_fill_more_than_256_scan_tiles(connectivity):
    """625 114 edges are 611 tiles of 1024: the scans of the edge ids, the leader flags and the vertex counts all take more than
    one pass of 256 over the tiles."""
    want = TI.reference("stripes", connectivity)
    assert len(want.area) == 3666 and len(want.xy) == 4 * 3666 and int(np.abs(want.area).sum()) == int(TI.get("stripes").areas[0])
    assert TI.same_contours(CT.contours(TI.get("stripes"), connectivity), want)


def test_real_size_twice_the_same_bytes_and_every_surface_agrees():
    pm = TI.get("real")
    for connectivity in TI.CONNECTIVITIES:
        first = CT.contours(pm, connectivity)
        for other in (CT.contours(pm, connectivity), pm.contours(connectivity), MT.mask_contours(pm, connectivity)):
            assert TI.same_contours(other, first)
        assert TI.same_contours(first, TI.reference("real", connectivity))
        polygons = [first.polygons(i) for i in range(len(pm))]
        assert pm.polygons(connectivity) == polygons and MT.mask_polygons(pm, connectivity) == polygons
        assert CT.polygons(pm, connectivity) == polygons


@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["holes", "seam", "lines", "many"])
def test_polygons_through_from_polygons_are_the_masks_with_their_holes_filled(name, connectivity):
    """On the GPU both ways: masks inside the image, so from_polygons(pm.polygons(c)) is fill_holes of the complementary
    connectivity -- with tight bounds, where fill_holes keeps the input's."""
    pm = TI.get(name)
    H, W = TI.image_size(pm)
    back = PackedMasks.from_polygons(pm.polygons(connectivity), H, W)
    want = pm.fill_holes(OTHER[connectivity])
    assert back.areas.tolist() == want.areas.tolist()
    assert all(np.array_equal(back.full(i, H, W), want.full(i, H, W)) for i in range(len(pm)))


# ---- the room ----

def filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


def raw(pm, connectivity, loop_cap, vert_cap, n=None, sizes_only=False):
    """-> (arguments, [loop_ptr, vert_ptr, area, xy] filled with FILL, n_loops, n_verts)."""
    outs = [filled(len(pm) + 1, np.int64), filled(loop_cap + 1, np.int64), filled(loop_cap, np.int64), filled((vert_cap, 2), np.int32)]
    n_loops, n_verts = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
    sa = _set_args(pm, areas=False)
    if n is not None:
        sa = sa[:4] + (n,)
    args = sa + (connectivity, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), None if sizes_only else _lib.ptr(outs[3]),
                 loop_cap, vert_cap, ctypes.addressof(n_loops), ctypes.addressof(n_verts), 0)
    return args, outs, n_loops, n_verts


@pytest.mark.parametrize("name", ["widths", "holes"])
def test_buffers_with_room_to_spare_keep_their_tail(name):
    pm, want = TI.get(name), TI.reference(name, 4)
    L, V = len(want.area), len(want.xy)
    args, outs, n_loops, n_verts = raw(pm, 4, L + 7, V + 9)
    _lib.call("mnc_mask_contours", *args)
    assert (n_loops.value, n_verts.value) == (L, V) and TI.same_array(outs[0], want.loop_ptr)
    assert TI.same_array(outs[1][:L + 1], want.vert_ptr) and untouched(outs[1][L + 1:])
    assert TI.same_array(outs[2][:L], want.area) and untouched(outs[2][L:])
    assert TI.same_array(outs[3][:V], want.xy) and untouched(outs[3][V:])


def test_too_little_room_reports_the_sizes_and_writes_nothing_else():
    pm, want = TI.get("widths"), TI.reference("widths", 8)
    L, V = len(want.area), len(want.xy)
    # the sizes only: no xy at all
    args, outs, n_loops, n_verts = raw(pm, 8, 0, 0, sizes_only=True)
    _lib.call("mnc_mask_contours", *args)
    assert (n_loops.value, n_verts.value) == (L, V) and TI.same_array(outs[0], want.loop_ptr) and all(untouched(o) for o in outs[1:])
    out = CT.contours_call(pm, 8, 0, 0, sizes_only=True)
    assert out[4:] == (L, V) and TI.same_array(out[0], want.loop_ptr)
    for loop_cap, vert_cap in ((L - 1, V), (L, V - 1)):
        args, outs, n_loops, n_verts = raw(pm, 8, loop_cap, vert_cap)
        with pytest.raises(_lib.MncError) as e:
            _lib.call("mnc_mask_contours", *args)
        assert e.value.code == INVALID
        assert "loop_cap %d or vert_cap %d is below the %d loops and %d vertices" % (loop_cap, vert_cap, L, V) in str(e.value)
        assert (n_loops.value, n_verts.value) == (L, V) and TI.same_array(outs[0], want.loop_ptr) and all(untouched(o) for o in outs[1:])
    # exactly enough is enough
    args, outs, n_loops, n_verts = raw(pm, 8, L, V)
    _lib.call("mnc_mask_contours", *args)
    assert TI.same_array(outs[1], want.vert_ptr) and TI.same_array(outs[2], want.area) and TI.same_array(outs[3], want.xy)
    # the wrapper comes back with room when its first guess was too small (the checkerboard at 4 has 4290 loops in one instance)
    assert len(CT.contours(TI.get("checker"), 4).area) == 4290


# ---- refusals: before anything is launched ----

class Flawed:
    """Two 10 x 10 masks of ones with one flaw (tests/test_mask_set_host.py's)."""

    def __init__(self, flaw):
        self.bounds = np.array([[0, 0, 9, 9], [0, 0, 9, 9]], np.int32)
        self.offsets = np.array([0, 80], np.int64)
        self.bits = np.full(20, (1 << 10) - 1, np.uint64)
        self.nbytes = self.bits.nbytes
        if flaw == "coordinate":
            self.bounds[1] = (0, 0, 2 ** 24, 0)
        elif flaw == "offset":
            self.offsets[1] = 4
        elif flaw == "rows":
            self.nbytes = 152
        else:
            assert flaw is None

    def args(self, connectivity=8, n=2, null=None):
        outs = [filled(2100, np.int64), filled(9, np.int64), filled(8, np.int64), filled((64, 2), np.int32), filled(1, np.uint64),
                filled(1, np.uint64)]
        p = [_lib.ptr(o) for o in outs]
        for k in (null or ()):
            p[k] = None
        return ((_lib.ptr(self.bounds), _lib.ptr(self.offsets), _lib.ptr(self.bits), self.nbytes, n, connectivity, p[0], p[1], p[2], p[3],
                 8, 64, p[4], p[5], 0), outs)


def refused(args, outs, message):
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_mask_contours", *args)
    assert e.value.code == INVALID
    assert str(e.value) == "mnc_mask_contours failed (status %d): mnc_mask_contours: %s" % (INVALID, message)
    assert _lib.load().mnc_last_error().decode() == "mnc_mask_contours: " + message
    assert all(untouched(o) for o in outs)


def test_everything_the_header_refuses_is_refused_by_name_with_nothing_written():
    refused(*Flawed(None).args(connectivity=6), message="connectivity=6 is not 4 or 8")
    refused(*Flawed(None).args(connectivity=0), message="connectivity=0 is not 4 or 8")
    refused(*Flawed(None).args(n=-1), message="n=-1 not in [0, 2048]")
    refused(*Flawed(None).args(n=2049), message="n=2049 not in [0, 2048]")
    refused(*Flawed("coordinate").args(), message="masks[1] coordinate 16777216 out of range")
    refused(*Flawed("offset").args(), message="masks[1] offset 4 is negative or not a multiple of 8")
    refused(*Flawed("rows").args(), message="the rows of masks[1] (80 bytes at 80) reach past the 152 bytes given")
    for null in ((0,), (4,), (5,)):
        refused(*Flawed(None).args(null=null), message="null output pointer")
    for null in ((1,), (2,)):
        refused(*Flawed(None).args(null=null), message="null vert_ptr or area")
    # 2048 instances that all point at the same 1023 rows of 16 words: 1024 lattice rows of 17 words each, past 2^25 at 1927
    n, w, h = 2048, 2 ** 10, 2 ** 10 - 1
    s = Flawed(None)
    s.bounds, s.offsets = np.tile(np.array([[0, 0, w - 1, h - 1]], np.int32), (n, 1)), np.zeros(n, np.int64)
    s.bits = np.zeros(h * w // 64, np.uint64)
    s.nbytes = s.bits.nbytes
    at = 2 ** 25 // (1024 * 17)
    refused(*s.args(n=n), message="more than 33554432 words of rows in the set (at masks[%d])" % at)
    # and the good set is taken
    args, outs = Flawed(None).args()
    _lib.call("mnc_mask_contours", *args)
    assert outs[0][:3].tolist() == [0, 1, 2] and outs[1][:3].tolist() == [0, 4, 8] and outs[2][:2].tolist() == [100, 100]
    assert outs[3][:8].tolist() == [[0, 0], [10, 0], [10, 10], [0, 10]] * 2 and untouched(outs[3][8:])


def test_more_than_2_to_the_30_edges_are_refused_after_the_counting_pass():
    """600 instances that all point at the same 1023 x 1024 checkerboard: 10.4 million words of lattice rows (below the limit of
    2^25), 4 edges a set pixel, 1 257 062 400 edges in all.  The counting pass runs, nothing is allocated for the edges."""
    n, w, h = 600, 1024, 1023
    yy, xx = np.mgrid[0:h, 0:w]
    one = MI.pack([[0, 0, w - 1, h - 1]], [(yy + xx) % 2 == 0])
    pm = PackedMasks(np.tile(one.bounds, (n, 1)), np.zeros(n, np.int64), np.tile(one.areas, n), None, None, one.bits)
    edges = 4 * int(one.areas[0]) * n
    assert 2 ** 30 < edges < 2 ** 31
    with pytest.raises(_lib.MncError) as e:
        CT.contours_call(pm, 8, 0, 0, sizes_only=True)
    assert e.value.code == INVALID and e.value.needed == (0, 0)
    assert str(e.value).endswith("mnc_mask_contours: %d boundary edges in the set (limit 2^30)" % edges)


def test_empty_sets_are_answered():
    none = MI.pack([], [])
    norows = MI.pack([[5, 5, 4, 9], [0, 0, 3, -1]], [np.zeros((5, 0), bool), np.zeros((0, 4), bool)], [1, 2], [0.5, 0.25])
    unset = MI.pack([[2, 3, 70, 6], [0, 0, 0, 0]], [np.zeros((4, 69), bool), np.zeros((1, 1), bool)], dirty=True)
    for pm in (none, norows, unset):
        for connectivity in TI.CONNECTIVITIES:
            got = CT.contours(pm, connectivity, device_id=0)
            assert TI.same_contours(got, CT.contours_numpy(pm, connectivity))
            assert got.loop_ptr.tolist() == [0] * (len(pm) + 1) and got.vert_ptr.tolist() == [0] and got.xy.shape == (0, 2)
            assert pm.polygons(connectivity) == [[] for _ in range(len(pm))]


# ---- the demo ----

def test_demo_save_annotations_writes_the_selected_masks_as_polygons_that_eval_coco_loads(tmp_path):
    import glob
    import io
    import json
    from contextlib import redirect_stdout

    import demo
    import eval_coco
    from mnc_amd import components as CC
    from mnc_amd import models
    jpg = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "demo", "*.jpg")))[0]
    proto = models.write_mnc_5stage_test_prototxt(width_div=8)
    name = os.path.splitext(os.path.basename(jpg))[0]
    h, w = demo._read_image_bgr(jpg).shape[:2]
    ann, dt = str(tmp_path / "ann.json"), str(tmp_path / "dt.json")
    with redirect_stdout(io.StringIO()):
        demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-annotations", ann, "--save-coco", dt, "--save-masks", str(tmp_path),
                   "--vis-thresh", "0.0", "--min-component-area", "30", "--largest-component"])
    with open(ann) as f:
        got = json.load(f)
    pm = PackedMasks.load(str(tmp_path / (name + "_masks.npz")))          # the masks after the selection
    assert len(pm) > 0 and sorted(got) == ["annotations", "categories", "images"]
    assert got["images"] == [{"id": name, "file_name": os.path.basename(jpg), "height": h, "width": w}]
    assert [c["id"] for c in got["categories"]] == list(range(1, 21))
    # what the numpy statement gives for those masks, byte for byte
    assert got["annotations"] == json.loads(json.dumps(demo._coco_annotations(name, pm, 1, cpu=True)))
    assert all(a["iscrowd"] == 0 and a["id"] == k + 1 and a["area"] == float(pm.areas[k]) for k, a in enumerate(got["annotations"]))
    # one component each, so one polygon each; read back they are the masks with their holes filled
    assert all(len(a["segmentation"]) == (1 if a["area"] else 0) for a in got["annotations"])
    back = PackedMasks.from_polygons([a["segmentation"] for a in got["annotations"]], h, w)
    want = CC.fill_holes_numpy(pm, 4)
    assert all(np.array_equal(back.full(i, h, w), want.full(i, h, w)) for i in range(len(pm)))
    for i, a in enumerate(got["annotations"]):
        x1, y1, x2, y2 = (int(v) for v in back.bounds[i])
        assert a["bbox"] == ([float(x1), float(y1), float(x2 - x1 + 1), float(y2 - y1 + 1)] if a["area"] else [0.0] * 4)
    with open(dt) as f:
        results = json.load(f)
    ev = eval_coco.evaluate(got, results, polygons=True)
    assert len(ev.lines()) == 12 and ev.stats[1] > 0
