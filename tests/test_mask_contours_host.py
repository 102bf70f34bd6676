"""The statement of the outline rule (mnc_amd/contours.py, include/mnc_hip.h n13) without a GPU: against closed forms that do not
come from it, against the polygon rasteriser of mnc_amd.polygons (independent code that must give the mask back), against
scipy.ndimage's component counts, the shoelace areas against the pixel counts, the structural facts of the rule, what Contours
refuses, and the word-level helpers of the kernels driven sequentially under the sanitizers -- nothing here may open a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_contours_inputs as TI  # noqa: E402
import mask_overlap_inputs as MI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import components as CC  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402
from mnc_amd import polygons as PG  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}
OTHER = {4: 8, 8: 4}


def one(m, x=0, y=0):
    m = np.asarray(m, bool)
    h, w = m.shape
    return MI.pack([[x, y, x + w - 1, y + h - 1]], [m], dirty=True)


# ---- closed forms ----

@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
def test_a_rectangle_is_its_four_corners(connectivity):
    for x, y, w, h in ((0, 0, 1, 1), (3, 5, 7, 2), (-4, -9, 64, 3), (10, 0, 65, 1), (0, 20, 1, 130)):
        c = CT.contours_numpy(one(np.ones((h, w), bool), x, y), connectivity)
        assert c.loop_ptr.tolist() == [0, 1] and c.vert_ptr.tolist() == [0, 4] and c.area.tolist() == [w * h]
        assert c.xy.tolist() == [[x, y], [x + w, y], [x + w, y + h], [x, y + h]]
        assert c.xy.dtype == np.int32 and c.area.dtype == np.int64 and c.loop_ptr.dtype == np.int64 and c.vert_ptr.dtype == np.int64


def test_two_diagonal_pixels_share_a_loop_at_8_and_keep_their_own_at_4():
    c = CT.contours_numpy(one(np.eye(2), 10, 20), 8)
    assert c.vert_ptr.tolist() == [0, 8] and c.area.tolist() == [2]
    assert c.xy.tolist() == [[10, 20], [11, 20], [11, 21], [12, 21], [12, 22], [11, 22], [11, 21], [10, 21]]
    c = CT.contours_numpy(one(np.eye(2), 10, 20), 4)
    assert c.vert_ptr.tolist() == [0, 4, 8] and c.area.tolist() == [1, 1]
    assert c.xy.tolist() == [[10, 20], [11, 20], [11, 21], [10, 21], [11, 21], [12, 21], [12, 22], [11, 22]]
    # the other way round: the loop starts at the upper right pixel
    c = CT.contours_numpy(one(np.eye(2)[::-1]), 8)
    assert c.vert_ptr.tolist() == [0, 8] and c.area.tolist() == [2]
    assert c.xy.tolist() == [[1, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2], [0, 1], [1, 1]]
    c = CT.contours_numpy(one(np.eye(2)[::-1]), 4)
    assert c.xy.tolist() == [[1, 0], [2, 0], [2, 1], [1, 1], [0, 1], [1, 1], [1, 2], [0, 2]] and c.area.tolist() == [1, 1]


@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
def test_a_ring_is_an_outer_loop_and_a_hole_whose_first_side_runs_down(connectivity):
    c = CT.contours_numpy(one(TI.CI.ring(12, 20, 2), 3, 5), connectivity)
    assert c.loop_ptr.tolist() == [0, 2] and c.area.tolist() == [240, -128]
    assert c.loop(0).tolist() == [[3, 5], [23, 5], [23, 17], [3, 17]]
    assert c.loop(1).tolist() == [[5, 7], [5, 15], [21, 15], [21, 7]]
    # a pixel in the hole's corner, joined to the ring by two sides: the hole loses it
    m = TI.CI.ring(5, 5, 1)
    m[1, 1] = True
    assert CT.contours_numpy(one(m), 4).area.tolist() == [25, -8] and CT.contours_numpy(one(m), 8).area.tolist() == [25, -8]
    m = np.ones((5, 5), bool)
    m[1, 1] = m[2, 2] = False
    assert CT.contours_numpy(one(m), 8).area.tolist() == [25, -1, -1] and CT.contours_numpy(one(m), 4).area.tolist() == [25, -2]


# ---- against the rasteriser, scipy and the pixel counts ----

@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(TI.SETS))
def test_the_loops_rasterise_back_to_the_mask_and_their_areas_sum_to_its_pixels(name, connectivity):
    """polygon_mask_parity_numpy is rleFrPoly's rule: on lattice points a horizontal edge toggles its columns at its row and a
    vertical edge nothing, so the XOR over the loops is the mask.  Every instance is rasterised in the frame of its own bounds (the
    loops moved by the bounds' corner: the rule reads an image that begins at (0, 0), and a frame of the image's size for each of
    20 000 loops would take minutes), where full(i, h, w) is dense(i)."""
    pm, c = TI.get(name), TI.reference(name, connectivity)
    assert len(c) == len(pm)
    for i in range(len(pm)):
        h, w = pm.size(i)
        if min(h, w) == 0:
            assert c.loops(i) == []
            continue
        got = np.zeros((h, w), bool)
        for xy, _ in c.loops(i):
            got ^= PG.polygon_mask_parity_numpy((xy - pm.bounds[i][:2]).reshape(-1).astype(np.float64), h, w)
        assert np.array_equal(got, pm.dense(i)), i
        assert sum(a for _, a in c.loops(i)) == int(pm.dense(i).sum()), i


def test_the_loops_move_with_the_bounds():
    pm = TI.get("plain")
    moved, dx, dy = TI.inside(pm)
    assert (dx, dy) == (10, 2)
    for connectivity in TI.CONNECTIVITIES:
        c, there = TI.reference("plain", connectivity), CT.contours_numpy(moved, connectivity)
        assert TI.same_array(there.xy, c.xy + np.array([dx, dy], np.int32))
        assert all(TI.same_array(getattr(there, f), getattr(c, f)) for f in ("loop_ptr", "vert_ptr", "area"))
        # in the frame of the image: the whole set at once
        H, W = TI.image_size(moved)
        for i in range(len(moved)):
            got = np.zeros((H, W), bool)
            for xy, _ in there.loops(i):
                got ^= PG.polygon_mask_parity_numpy(xy.reshape(-1).astype(np.float64), H, W)
            assert np.array_equal(got, moved.full(i, H, W)), i


@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(TI.SETS))
def test_outer_loops_number_scipys_components_and_holes_the_enclosed_background(name, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    pm, c = TI.get(name), TI.reference(name, connectivity)
    for i in range(len(pm)):
        areas = [a for _, a in c.loops(i)]
        if min(pm.size(i)) == 0:
            assert areas == []
            continue
        m = pm.dense(i)
        assert sum(a > 0 for a in areas) == ndimage.label(m, STRUCTURE[connectivity])[1], i
        outside = np.pad(~m, 1, constant_values=True)
        assert sum(a < 0 for a in areas) == ndimage.label(outside, STRUCTURE[OTHER[connectivity]])[1] - 1, i
        assert 0 not in areas


@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(TI.SETS))
def test_the_structure_of_every_loop(name, connectivity):
    """Sides alternate, no vertex is collinear, the start vertex is the smallest in (y, x) order and occurs once, a loop is a
    hole exactly when its first side runs +y, the shoelace formula gives the stored area, and the loops of an instance are in the
    order of their start vertices, which differ."""
    pm, c = TI.get(name), TI.reference(name, connectivity)
    assert c.loop_ptr[0] == 0 and c.vert_ptr[0] == 0 and c.loop_ptr[-1] == len(c.area) and c.vert_ptr[-1] == len(c.xy)
    for i in range(len(pm)):
        starts = []
        for xy, area in c.loops(i):
            p = xy.astype(np.int64)
            k = len(p)
            assert k >= 4 and k % 2 == 0
            step = np.roll(p, -1, axis=0) - p
            horizontal = step[:, 1] == 0
            assert ((step != 0).sum(axis=1) == 1).all()                    # one coordinate changes
            assert horizontal[0] != horizontal[1] and (horizontal[::2] == horizontal[0]).all() and (horizontal[1::2] == horizontal[1]).all()
            key = p[:, 1] * 2 ** 32 + p[:, 0]
            assert key.argmin() == 0 and (key == key[0]).sum() == 1
            twice = int((p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]).sum())
            assert twice == 2 * area and area != 0
            first = tuple(step[0])
            assert (area < 0) == (first[0] == 0 and first[1] > 0)
            assert area < 0 or (first[1] == 0 and first[0] > 0)            # an outer loop sets out along +x
            x1, y1, x2, y2 = (int(v) for v in pm.bounds[i])
            assert p[:, 0].min() >= x1 and p[:, 0].max() <= x2 + 1 and p[:, 1].min() >= y1 and p[:, 1].max() <= y2 + 1
            starts.append(int(key[0]))
        assert starts == sorted(starts) and len(set(starts)) == len(starts)


def test_the_loop_totals_of_the_sets():
    """Both connectivities together."""
    for name, loops in (("widths", 8727), ("checker", 8387), ("many", 20212), ("spiral", 4)):
        assert sum(len(TI.reference(name, c).area) for c in TI.CONNECTIVITIES) == loops
    # the checkerboard at 4: every set pixel is a square of its own
    c = TI.reference("checker", 4)
    assert len(c.area) == 4290 and (c.area == 1).all() and (np.diff(c.vert_ptr) == 4).all()
    # the longest loops: more than 2^14 edges
    for k in (0, 1):
        xy = TI.reference("spiral", 8).loops(k)[0][0].astype(np.int64)
        assert np.abs(np.roll(xy, -1, axis=0) - xy).sum() > 2 ** 14


# ---- the polygons ----

@pytest.mark.parametrize("connectivity", TI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(TI.SETS))
def test_the_outer_loops_as_coco_polygons_are_the_masks_with_their_holes_filled(name, connectivity):
    """Every instance in the frame of its own bounds, as above."""
    pm, c = TI.get(name), TI.reference(name, connectivity)
    want = CC.fill_holes_numpy(pm, OTHER[connectivity])
    for i in range(len(pm)):
        h, w = pm.size(i)
        seg = c.polygons(i)
        assert all(isinstance(v, float) for poly in seg for v in poly)
        assert len(c.polygons(i, holes=True)) == len(c.loops(i)) and len(seg) == sum(a > 0 for _, a in c.loops(i))
        if min(h, w) == 0:
            assert seg == []
            continue
        local = [(np.array(poly).reshape(-1, 2) - pm.bounds[i][:2]).reshape(-1).tolist() for poly in seg]
        back = PG.masks_from_polygons_numpy([local], h, w)
        assert np.array_equal(back.full(0, h, w), want.dense(i)), i


def test_the_polygons_of_a_whole_set_in_the_image():
    for name in ("holes", "seam", "lines"):
        pm = TI.get(name)
        H, W = TI.image_size(pm)
        for connectivity in TI.CONNECTIVITIES:
            c = TI.reference(name, connectivity)
            back = PG.masks_from_polygons_numpy([c.polygons(i) for i in range(len(pm))], H, W)
            want = CC.fill_holes_numpy(pm, OTHER[connectivity])
            assert all(np.array_equal(back.full(i, H, W), want.full(i, H, W)) for i in range(len(pm)))


# ---- Contours ----

def test_contours_accessors_and_what_it_refuses():
    c = TI.reference("holes", 8)
    assert len(c) == len(TI.get("holes"))
    loops = c.loops(0)
    assert [a for _, a in loops] == [240, -128] and loops[0][0].dtype == np.int32 and loops[0][0].shape == (4, 2)
    assert c.polygons(0) == [[3.0, 5.0, 23.0, 5.0, 23.0, 17.0, 3.0, 17.0]]
    assert c.polygons(0, holes=True)[1] == [5.0, 7.0, 5.0, 15.0, 21.0, 15.0, 21.0, 7.0]
    for bad in (-1, len(c)):
        with pytest.raises(IndexError, match="Contours: instance %d of %d" % (bad, len(c))):
            c.loops(bad)
        with pytest.raises(IndexError):
            c.polygons(bad)
    empty = CT.Contours([0], [0], [], np.zeros((0, 2), np.int32))
    assert len(empty) == 0 and empty.xy.shape == (0, 2)
    with pytest.raises(ValueError, match="loop_ptr does not run from 0 to 1"):
        CT.Contours([0, 2], [0, 4], [4], np.zeros((4, 2)))
    with pytest.raises(ValueError, match="vert_ptr does not run from 0 to 4"):
        CT.Contours([0, 1], [0, 3], [4], np.zeros((4, 2)))
    with pytest.raises(ValueError, match="vert_ptr does not run from 0 to 4"):
        CT.Contours([0, 2], [0, 5, 4], [4, 1], np.zeros((4, 2)))
    with pytest.raises(ValueError, match="vert_ptr has 2 entries for 2 loops"):
        CT.Contours([0, 2], [0, 4], [4, 1], np.zeros((4, 2)))


def gone(*args, **kw):
    """Stands in for the library: touching it fails the test."""
    raise AssertionError("the library was looked for")


@pytest.mark.parametrize("call, message", [
    (lambda pm: CT.contours(pm, 6), "contours: connectivity=6 is not 4 or 8"),
    (lambda pm: pm.contours(0), "contours: connectivity=0 is not 4 or 8"),
    (lambda pm: pm.polygons(5), "contours: connectivity=5 is not 4 or 8"),
    (lambda pm: CT.contours_numpy(pm, 2), "contours_numpy: connectivity=2 is not 4 or 8"),
])
def test_invalid_arguments_raise_by_name_before_the_library_is_looked_for(monkeypatch, call, message):
    monkeypatch.setattr(_lib, "call", gone)
    monkeypatch.setattr(_lib, "load", gone)
    with pytest.raises(ValueError) as e:
        call(TI.get("seam"))
    assert str(e.value) == message


def test_the_word_limit_is_counted_on_the_lattice_rows():
    # 2048 instances that all point at the same 1023 rows of 16 words: 1024 lattice rows of 17 words each
    n, w, h = 2048, 2 ** 10, 2 ** 10 - 1
    pm = PackedMasks(np.tile(np.array([[0, 0, w - 1, h - 1]], np.int32), (n, 1)), np.zeros(n, np.int64), np.zeros(n, np.int64), None,
                     None, np.zeros(h * w // 64, np.uint64))
    at = 2 ** 25 // (1024 * 17)
    with pytest.raises(ValueError, match=r"contours_numpy: more than 33554432 words of rows in the set \(at masks\[%d\]\)" % at):
        CT.contours_numpy(pm)


def test_n13_is_declared():
    decls = _lib.parse_header()
    assert decls["mnc_mask_contours"][2] == ["bounds", "offsets", "bits", "bytes", "n", "connectivity", "loop_ptr", "vert_ptr", "area",
                                             "xy", "loop_cap", "vert_cap", "n_loops", "n_verts", "device_id"]
    assert decls["mnc_mask_contours_timing"][2] == ["on", "last_ms"]


# ---- the helpers of the kernels, sequentially on the CPU under the sanitizers ----

def test_the_edge_helpers_trace_every_shape_under_asan_and_ubsan(tmp_path):
    """tests/c/mask_contour_main.cpp drives csrc/mask_contour.h (edge masks, edge ids, the turn, the successor) over every mask of
    every set, replays the rounds of the kernels sequentially and compares the loops with the statement's, vertex by vertex; built
    with -fsanitize=address,undefined."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    path, count = str(tmp_path / "masks.bin"), 0
    with open(path, "wb") as f:
        f.write(np.int32(0).tobytes())
        for name in TI.SETS:
            pm = TI.get(name)
            refs = [TI.reference(name, c) for c in (4, 8)]
            for i in range(len(pm)):
                m = pm.dense(i)
                if not m.size:
                    continue
                count += 1
                f.write(np.array(m.shape, np.int32).tobytes())
                f.write(m.astype(np.uint8).tobytes())
                for c in refs:
                    loops = c.loops(i)
                    f.write(np.int32(len(loops)).tobytes())
                    for xy, area in loops:
                        f.write(np.int32(len(xy)).tobytes() + np.int64(area).tobytes())
                        f.write((xy - pm.bounds[i][:2]).astype(np.int32).tobytes())
        f.seek(0)
        f.write(np.int32(count).tobytes())
    exe = str(tmp_path / "mask_contour_main")
    build = subprocess.run([cxx, "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "mask_contour_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler cannot link the sanitizers' runtimes")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
    assert len(lines) == count
    loops = [0, 0]
    for line in lines:
        loops[0] += line[3]
        loops[1] += line[4]
    assert loops == [sum(len(TI.reference(name, c).area) for name in TI.SETS) for c in (4, 8)]
