"""Outlines simplified to a tolerance on the GPU (csrc/contour_simplify.hip: mnc_contours_simplify and the Python surfaces over it)
against the numpy statement mnc_amd.contours.simplify_numpy, which tests/test_contour_simplify_host.py pins to closed forms, to a
brute-force check of the tolerance and to scipy's distance transform.  Every comparison is exact: dtype, shape and bytes.  The
shapes are those of tests/contour_simplify_inputs.py."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import contour_simplify_inputs as SI  # noqa: E402
import mask_contours_inputs as TI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
FILL = 0x5a


@pytest.mark.parametrize("q", (0, 8, 16, 40))
@pytest.mark.parametrize("name", [n for n in TI.SETS if n != "real"])
def test_the_standard_sets_equal_the_statement(name, q):
    got = CT.simplify(TI.reference(name, 8), q / 16.0)
    assert isinstance(got, CT.SimplifiedContours) and SI.same_simplified(got, SI.reference(name, 8, q))


def test_real_size_twice_the_same_bytes_and_every_surface_agrees():
    pm = TI.get("real")
    for connectivity in SI.CONNECTIVITIES:
        c = TI.reference("real", connectivity)
        for q in (8, 16, 40):
            want = SI.reference("real", connectivity, q)
            first = CT.simplify(c, q / 16.0)
            for other in (CT.simplify(c, q / 16.0), c.simplify(q / 16.0), CT.contours(pm, connectivity).simplify(q / 16.0, device_id=0)):
                assert SI.same_simplified(other, first)
            assert SI.same_simplified(first, want)
            polygons = [want.polygons(i) for i in range(len(pm))]
            assert pm.polygons(connectivity, epsilon=q / 16.0) == polygons and MT.mask_polygons(pm, connectivity, q / 16.0) == polygons
            assert CT.polygons(pm, connectivity, epsilon=q / 16.0) == polygons
        # the default is the exact outline, as before
        exact = [c.polygons(i) for i in range(len(pm))]
        assert pm.polygons(connectivity) == exact and pm.polygons(connectivity, epsilon=0.0) == exact and MT.mask_polygons(pm, connectivity) == exact


def test_epsilon_0_does_not_call_the_entry(monkeypatch):
    pm = TI.get("seam")
    want = pm.polygons(8)
    monkeypatch.setattr(CT, "simplify", lambda *a, **k: pytest.fail("simplify was called"))
    assert pm.polygons(8, epsilon=0.0) == want and CT.polygons(pm, 8, None, 0.0) == want and MT.mask_polygons(pm, 8, 0.0) == want


def equals_statement(name, q):
    c, want = SI.general(name), SI.general_reference(name, q)
    out_ptr, out_xy, out_index, kept = CT.simplify_call(c.vert_ptr, c.xy, q)
    assert kept == len(want.xy)
    assert SI.same_array(out_ptr, want.vert_ptr) and SI.same_array(out_xy[:kept], want.xy) and SI.same_array(out_index[:kept], want.index)
    assert not out_xy[kept:].any() and not out_index[kept:].any()
    assert SI.same_simplified(c.simplify(q / 16.0), want)


@pytest.mark.parametrize("q", (0, 16, 2 ** 20))
def test_loops_of_0_to_3_vertices_are_unchanged_and_equal_vertices_come_out_as_three(q):
    equals_statement("short", q)
    assert SI.general_reference("short", q).vert_ptr[:6].tolist() == [0, 0, 1, 3, 6, 9]


@pytest.mark.parametrize("q", (8, 16, 40))
def test_staircases_around_the_wave_the_workgroup_the_tile_and_the_lds_stage(q):
    """62 .. 66 vertices: the wave's kernel and the workgroup's; 254 .. 258, 1022 .. 1026: the threads of a workgroup and a scan
    tile; 4094 .. 4098: staged in LDS and read from global memory."""
    assert np.diff(SI.general("stairs").vert_ptr).tolist() == list(SI.STAIR_SIZES)
    equals_statement("stairs", q)
    assert 3 * len(SI.STAIR_SIZES) < len(SI.general_reference("stairs", q).xy) < len(SI.general("stairs").xy)


@pytest.mark.parametrize("q", (16, 80))
def test_one_loop_of_40000_vertices_past_any_lds_stage(q):
    assert len(SI.general("long").xy) == 40000
    equals_statement("long", q)


@pytest.mark.parametrize("q", (0, 16))
def test_tiny_loops_whose_flags_fill_more_than_256_scan_tiles(q):
    """263 173 vertices are 258 tiles of 1024: the scan over the tiles takes a second pass of 256."""
    c, want = SI.general("tiny"), SI.general_reference("tiny", q)
    assert len(c.xy) == 263173 > 257 * 1024 and len(want.xy) == 201425
    assert SI.same_simplified(c.simplify(q / 16.0), want)


def test_the_comb_whose_recursion_is_hundreds_deep():
    equals_statement("comb", 16)


@pytest.mark.parametrize("q", (0, 8, 16, 24))
def test_ties_and_coincident_endpoints(q):
    equals_statement("ties", q)


def test_the_products_need_128_bits():
    """With 64-bit products 256 N = 2^64 wraps to 0."""
    equals_statement("wide", 128)
    equals_statement("wide", 127)
    assert SI.general("wide").simplify(8.0).index.tolist() == [0, 1, 2]
    assert SI.general("wide").simplify(127 / 16.0).index.tolist() == [0, 1, 2, 3]


# ---- the room, empty sets, refusals ----

def filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


def raw(vert_ptr, xy, q, n_loops=None, n_verts=None, spare=(5, 7), null=()):
    """-> (arguments, [out_vert_ptr, out_xy, out_index, out_verts] filled with FILL)."""
    vert_ptr, xy = np.ascontiguousarray(vert_ptr, np.int64), np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    L, V = len(vert_ptr) - 1, len(xy)
    outs = [filled(L + 1 + spare[0], np.int64), filled((V + spare[1], 2), np.int32), filled(V + spare[1], np.int64), filled(1, np.uint64)]
    p = [_lib.ptr(vert_ptr), _lib.ptr(xy)] + [_lib.ptr(o) for o in outs]
    for k in null:
        p[k] = None
    args = (p[0], p[1], L if n_loops is None else n_loops, V if n_verts is None else n_verts, q, p[2], p[3], p[4], p[5], 0)
    return args, outs, (vert_ptr, xy)


def test_buffers_with_room_to_spare_keep_their_tail():
    c, want = TI.reference("holes", 8), SI.reference("holes", 8, 16)
    args, outs, alive = raw(c.vert_ptr, c.xy, 16)
    _lib.call("mnc_contours_simplify", *args)
    L, kept = len(c.area), len(want.xy)
    assert 0 < kept < len(c.xy) and int(outs[3][0]) == kept
    assert SI.same_array(outs[0][:L + 1], want.vert_ptr) and untouched(outs[0][L + 1:])
    assert SI.same_array(outs[1][:kept], want.xy) and untouched(outs[1][kept:])
    assert SI.same_array(outs[2][:kept], want.index) and untouched(outs[2][kept:])


def test_empty_inputs_are_answered():
    # no loops
    args, outs, alive = raw([0], np.zeros((0, 2), np.int32), 16)
    _lib.call("mnc_contours_simplify", *args)
    assert outs[0][:1].tolist() == [0] and untouched(outs[0][1:]) and int(outs[3][0]) == 0 and untouched(outs[1]) and untouched(outs[2])
    # loops without vertices, with and without the vertex pointers
    for null in ((), (1, 3, 4)):
        args, outs, alive = raw([0, 0, 0, 0], np.zeros((0, 2), np.int32), 16, null=null)
        _lib.call("mnc_contours_simplify", *args)
        assert outs[0][:4].tolist() == [0, 0, 0, 0] and untouched(outs[0][4:]) and int(outs[3][0]) == 0 and untouched(outs[1])
    empty = CT.Contours([0, 0, 0], [0], [], np.zeros((0, 2), np.int32))
    got = empty.simplify(1.0, device_id=0)
    assert SI.same_simplified(got, CT.simplify_numpy(empty, 1.0)) and got.vert_ptr.tolist() == [0] and got.index.shape == (0,)
    assert got.loop_ptr.tolist() == [0, 0, 0] and got.xy.shape == (0, 2)


def refused(args, outs, message):
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_contours_simplify", *args)
    assert e.value.code == INVALID
    assert str(e.value) == "mnc_contours_simplify failed (status %d): mnc_contours_simplify: %s" % (INVALID, message)
    assert _lib.load().mnc_last_error().decode() == "mnc_contours_simplify: " + message
    assert all(untouched(o) for o in outs)


def test_everything_the_header_refuses_is_refused_by_name_with_nothing_written():
    ptr, xy = [0, 4, 8], [[0, 0], [10, 0], [10, 10], [0, 10]] * 2
    refused(*raw(ptr, xy, -1)[:2], message="q=-1 not in [0, 1048576]")
    refused(*raw(ptr, xy, 2 ** 20 + 1)[:2], message="q=1048577 not in [0, 1048576]")
    refused(*raw(ptr, xy, 16, n_loops=2 ** 24 + 1)[:2], message="n_loops=16777217 above 16777216")
    refused(*raw(ptr, xy, 16, n_verts=2 ** 27 + 1)[:2], message="n_verts=134217729 above 134217728")
    for null in ((0,), (2,), (5,)):
        refused(*raw(ptr, xy, 16, null=null)[:2], message="null vert_ptr, out_vert_ptr or out_verts")
    for null in ((1,), (3,), (4,)):
        refused(*raw(ptr, xy, 16, null=null)[:2], message="null xy, out_xy or out_index")
    refused(*raw([1, 4, 8], xy, 16)[:2], message="vert_ptr[0]=1 is not 0")
    refused(*raw([0, 5, 4, 8], xy, 16)[:2], message="vert_ptr decreases at loop 1 (4 after 5)")
    refused(*raw([0, 4, 7], xy, 16)[:2], message="vert_ptr ends at 7, not at the 8 vertices given")
    refused(*raw([0, 4, 9], xy, 16)[:2], message="vert_ptr ends at 9, not at the 8 vertices given")
    for bad in (2 ** 24 + 1, -2 ** 24 - 1):
        far = np.array(xy, np.int32)
        far[5, 1] = bad
        refused(*raw(ptr, far, 16)[:2], message="coordinate %d of vertex 5 outside [-16777216, 16777216]" % bad)
    # and the good loops are taken, at the largest coordinates and the largest tolerance as well
    args, outs, alive = raw(ptr, xy, 16)
    _lib.call("mnc_contours_simplify", *args)
    assert outs[0][:3].tolist() == [0, 4, 8] and outs[1][:8].tolist() == xy and outs[2][:8].tolist() == list(range(8)) and int(outs[3][0]) == 8
    edge = [[-2 ** 24, -2 ** 24], [2 ** 24, -2 ** 24], [2 ** 24, 2 ** 24], [-2 ** 24, 2 ** 24]]
    got = SI.as_contours([edge]).simplify(2 ** 20 / 16.0)
    assert SI.same_simplified(got, CT.simplify_numpy(SI.as_contours([edge]), 2 ** 20 / 16.0)) and got.index.tolist() == [0, 1, 2, 3]


def test_the_timing_entry_keeps_the_last_call():
    c = TI.reference("holes", 8)
    CT.simplify_timing(True)                                 # (switching on forgets what was kept before)
    c.simplify(1.0)
    assert CT.simplify_timing(False) > 0.0
    c.simplify(1.0)                                          # not timed
    assert CT.simplify_timing(True) > 0.0 and CT.simplify_timing(False) == -1.0


# ---- the demo ----

def test_demo_polygon_epsilon_writes_simplified_polygons_that_eval_coco_loads(tmp_path):
    import glob
    import io
    import json
    from contextlib import redirect_stdout

    import demo
    import eval_coco
    from mnc_amd import models
    from mnc_amd.masks import PackedMasks
    jpg = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "demo", "*.jpg")))[0]
    proto = models.write_mnc_5stage_test_prototxt(width_div=8)
    name = os.path.splitext(os.path.basename(jpg))[0]
    ann, plain, dt = str(tmp_path / "ann.json"), str(tmp_path / "plain.json"), str(tmp_path / "dt.json")
    common = ["--def", proto, "--images", jpg, "--no-vis", "--save-coco", dt, "--save-masks", str(tmp_path), "--vis-thresh", "0.0",
              "--min-component-area", "30", "--largest-component"]
    with redirect_stdout(io.StringIO()):
        demo.main(common + ["--save-annotations", ann, "--polygon-epsilon", "1.0"])
        demo.main(common + ["--save-annotations", plain])
    with open(ann) as f:
        got = json.load(f)
    with open(plain) as f:
        exact = json.load(f)
    pm = PackedMasks.load(str(tmp_path / (name + "_masks.npz")))
    assert len(pm) > 0
    assert got["annotations"] == json.loads(json.dumps(demo._coco_annotations(name, pm, 1, cpu=True, epsilon=1.0)))
    polygons = [p for a in got["annotations"] for p in a["segmentation"]]
    assert polygons and all(len(p) >= 6 and len(p) % 2 == 0 for p in polygons)
    assert sum(len(p) for p in polygons) < sum(len(p) for a in exact["annotations"] for p in a["segmentation"])
    for a in got["annotations"]:
        if a["segmentation"]:
            xs, ys = [v for p in a["segmentation"] for v in p[0::2]], [v for p in a["segmentation"] for v in p[1::2]]
            assert a["bbox"] == [min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)]
    assert [a["area"] for a in got["annotations"]] == [float(v) for v in pm.areas]
    # without the flag the file is what it is today
    assert exact["annotations"] == json.loads(json.dumps(demo._coco_annotations(name, pm, 1, cpu=True)))
    assert got["images"] == exact["images"] and got["categories"] == exact["categories"]
    with open(dt) as f:
        results = json.load(f)
    ev = eval_coco.evaluate(got, results, polygons=True)
    assert len(ev.lines()) == 12
