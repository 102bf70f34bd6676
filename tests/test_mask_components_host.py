"""The statements of the connected-component rule (mnc_amd/components.py, include/mnc_hip.h n12) without a GPU: against
scipy.ndimage on every shape of mask_components_inputs at both connectivities, against closed forms that do not come from the
statements, the selection's and the split's own properties, and every invalid argument refused by name -- nothing here may open a
device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_components_inputs as CI  # noqa: E402
import mask_overlap_inputs as MI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import components as CC  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

INVALID = 1
FILL = 0x5a
STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}


def clean(pm):
    """The input with its padding cleared, rebuilt from the dense masks."""
    return MI.pack(pm.bounds.tolist(), [pm.dense(i) for i in range(len(pm))], pm.classes, pm.scores)


# ---- against scipy ----

@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CI.SETS))
def test_label_maps_equal_scipys_including_the_numbering(name, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    pm = CI.get(name)
    table = CI.reference(name, "components", connectivity)
    for i in range(len(pm)):
        m = pm.dense(i)
        if m.size == 0:
            assert table.comp_ptr[i + 1] == table.comp_ptr[i]
            continue
        want, count = ndimage.label(m, structure=STRUCTURE[connectivity])
        got, got_count = CC.label_numpy(m, connectivity)
        assert got_count == count == table.comp_ptr[i + 1] - table.comp_ptr[i]
        assert np.array_equal(got, want)
        # the table against the label map
        lo = int(table.comp_ptr[i])
        x1, y1 = int(pm.bounds[i][0]), int(pm.bounds[i][1])
        for c, sl in enumerate(ndimage.find_objects(want)):
            assert table.area[lo + c] == int((want == c + 1).sum())
            assert table.bbox[lo + c].tolist() == [x1 + sl[1].start, y1 + sl[0].start, x1 + sl[1].stop - 1, y1 + sl[0].stop - 1]
            ys, xs = np.nonzero(want == c + 1)
            assert table.anchor[lo + c].tolist() == [x1 + xs[0], y1 + ys[0]]


@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CI.SETS))
def test_fill_holes_equals_scipys_binary_fill_holes(name, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    pm = CI.get(name)
    got = CI.reference(name, "fill_holes", connectivity)
    assert CI.same_array(got.bounds, pm.bounds) and CI.same_array(got.offsets, pm.offsets)
    assert CI.same_array(got.classes, pm.classes) and CI.same_array(got.scores, pm.scores) and got.bits.shape == pm.bits.shape
    for i in range(len(pm)):
        m = pm.dense(i)
        if m.size == 0:
            assert got.areas[i] == 0
            continue
        want = ndimage.binary_fill_holes(m, structure=STRUCTURE[connectivity])
        assert np.array_equal(got.dense(i), want) and got.areas[i] == int(want.sum())
    assert CI.same_masks(got, clean(got))               # padding bits are 0


# ---- closed forms ----

def test_the_checkerboard_counts():
    pm = CI.get("checker")
    t4, t8 = CI.reference("checker", "components", 4), CI.reference("checker", "components", 8)
    assert t4.comp_ptr.tolist() == [0, 4290] and (t4.area == 1).all() and t4.area.dtype == np.int64
    assert (t4.bbox[:, :2] == t4.anchor).all() and (t4.bbox[:, 2:] == t4.anchor).all()
    x1, y1 = int(pm.bounds[0][0]), int(pm.bounds[0][1])
    assert t4.anchor[:3].tolist() == [[x1, y1], [x1 + 2, y1], [x1 + 4, y1]] and t4.anchor[65].tolist() == [x1 + 1, y1 + 1]
    assert t8.comp_ptr.tolist() == [0, 1] and t8.area.tolist() == [4290]
    assert t8.bbox.tolist() == [[x1, y1, x1 + 129, y1 + 65]] and t8.anchor.tolist() == [[x1, y1]]


def test_the_seam_and_the_corner():
    t4, t8 = CI.reference("seam", "components", 4), CI.reference("seam", "components", 8)
    # a, b: two pixels across the word seam; c: three pieces chained across it by corners; d: one long run joins what touches it, by
    # an edge (two pieces meet it across a corner only); e: two rectangles that touch at a corner
    assert np.diff(t4.comp_ptr).tolist() == [2, 2, 3, 3, 2]
    assert np.diff(t8.comp_ptr).tolist() == [1, 1, 1, 1, 1]
    assert t4.area.tolist() == [1, 1, 1, 1, 4, 6, 1, 7 + 1 + 171 + 50, 1, 10, 20, 28]
    assert t8.area.tolist() == [2, 2, 11, 240, 48]
    x1, y1 = (int(v) for v in CI.get("seam").bounds[0][:2])
    assert t8.bbox[0].tolist() == [x1 + 63, y1, x1 + 64, y1 + 1] and t8.anchor[0].tolist() == [x1 + 63, y1]
    assert t8.anchor[1].tolist() == [x1 + 130 + 64, y1]            # the mirrored one starts at its bit 64


def test_the_spiral_and_the_comb_are_one_component():
    for name in ("spiral", "comb"):
        for connectivity in CI.CONNECTIVITIES:
            t = CI.reference(name, "components", connectivity)
            pm = CI.get(name)
            assert np.diff(t.comp_ptr).tolist() == [1, 1]
            assert t.area.tolist() == [int(pm.dense(0).sum()), int(pm.dense(1).sum())]
            assert (t.bbox == pm.bounds).all()


def test_the_ring_filled_is_its_rectangle_and_the_open_shapes_are_unchanged():
    pm = CI.get("holes")
    for connectivity in CI.CONNECTIVITIES:
        got = CI.reference("holes", "fill_holes", connectivity)
        assert got.dense(0).all() and got.areas[0] == 12 * 20
        assert np.array_equal(got.dense(1), pm.dense(1))           # the C-shape
        assert np.array_equal(got.dense(2), pm.dense(2))           # the holes that touch the box edge
        assert got.dense(3).all()                                  # the nested rings: everything is filled
        assert got.dense(5).all()
        want = np.ones((5, 130), bool)
        want[1, 0] = want[2, 129] = False                          # the pinholes at the box edge stay
        assert np.array_equal(got.dense(6), want)
    # the hole that meets the outside across a corner: a hole of the 4-connected background only
    assert CI.reference("holes", "fill_holes", 4).dense(4).sum() == 64 - 1
    assert np.array_equal(CI.reference("holes", "fill_holes", 8).dense(4), pm.dense(4))


def test_the_nested_rings_split_into_two_instances_whose_boxes_nest():
    pm = CI.get("holes")
    for connectivity in CI.CONNECTIVITIES:
        parts, source = CI.reference("holes", "split", connectivity)
        mine = np.nonzero(source == 3)[0]
        assert len(mine) == 2
        outer, inner = parts.bounds[mine[0]], parts.bounds[mine[1]]
        assert outer.tolist() == pm.bounds[3].tolist()
        assert outer[0] < inner[0] and outer[1] < inner[1] and inner[2] < outer[2] and inner[3] < outer[3]
        assert np.array_equal(parts.dense(mine[1]), CI.ring(14, 20, 2))


# ---- the selection ----

@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CI.SETS))
def test_select_everything_is_the_input_with_clean_padding(name, connectivity):
    pm = CI.get(name)
    got = CI.reference(name, "select", connectivity, 1, 0)
    want = clean(pm)
    assert CI.same_masks(got, PackedMasks(want.bounds, pm.offsets, want.areas, pm.classes, pm.scores, want.bits))


@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["widths", "many", "holes", "plain"])
def test_select_areas_sum_up(name, connectivity):
    table = CI.reference(name, "components", connectivity)
    for min_area, keep in CI.SELECTIONS:
        got = CI.reference(name, "select", connectivity, min_area, keep)
        for i in range(len(got)):
            area = table.area[table.comp_ptr[i]:table.comp_ptr[i + 1]]
            stay = np.sort(area[area >= min_area])[::-1]
            assert got.areas[i] == int((stay[:keep] if keep else stay).sum()) == int(got.dense(i).sum())


def test_select_area_ties_go_to_the_lower_number():
    m = np.zeros((7, 9), bool)
    m[0, 0:3] = m[2, 0:3] = m[4, 0:3] = m[6, 0:2] = True          # areas 3, 3, 3, 2 in this order
    pm = MI.pack([[0, 0, 8, 6]], [m], [1], [0.5])
    two = CC.select_numpy(pm, 8, 1, 2).dense(0)
    assert two[0, 0:3].all() and two[2, 0:3].all() and two.sum() == 6
    one = CC.select_numpy(pm, 4, 3, 1).dense(0)
    assert one[0, 0:3].all() and one.sum() == 3
    assert CC.select_numpy(pm, 4, 4, 0).dense(0).sum() == 0
    assert CC.select_numpy(pm, 4, 3, 0).dense(0).sum() == 9


# ---- the split ----

@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["widths", "seam", "spiral", "holes_dirty", "plain", "many"])
def test_split_parts_paint_back_to_the_input(name, connectivity):
    pm = CI.get(name)
    parts, source = CI.reference(name, "split", connectivity)
    table = CI.reference(name, "components", connectivity)
    assert source.dtype == np.int32 and np.array_equal(source, np.repeat(np.arange(len(pm)), np.diff(table.comp_ptr)))
    assert np.array_equal(parts.bounds, table.bbox) and np.array_equal(parts.areas, table.area)
    assert np.array_equal(parts.classes, pm.classes[source]) and np.array_equal(parts.scores, pm.scores[source])
    sizes = np.array([parts.size(c)[0] * ((parts.size(c)[1] + 63) // 64) * 8 for c in range(len(parts))], np.int64)
    assert np.array_equal(parts.offsets, np.cumsum(sizes) - sizes) and parts.bits.nbytes == sizes.sum()
    painted = [np.zeros(pm.size(i), bool) for i in range(len(pm))]
    for c in range(len(parts)):
        i = int(source[c])
        d = parts.dense(c)
        assert CC.label_numpy(d, connectivity)[1] == 1                             # exactly one component
        assert d[0].any() and d[-1].any() and d[:, 0].any() and d[:, -1].any()    # tight bounds
        x, y = int(parts.bounds[c][0] - pm.bounds[i][0]), int(parts.bounds[c][1] - pm.bounds[i][1])
        assert not (painted[i][y:y + d.shape[0], x:x + d.shape[1]] & d).any()
        painted[i][y:y + d.shape[0], x:x + d.shape[1]] |= d
    for i in range(len(pm)):
        assert painted[i].size == 0 or np.array_equal(painted[i], pm.dense(i))   # (an instance without rows has no pixels)


# ---- the helpers of the kernels, sequentially on the CPU under the sanitizers ----

def test_the_union_find_helpers_label_every_shape_under_asan_and_ubsan(tmp_path):
    """tests/c/mask_cc_main.cpp drives csrc/mask_cc.h (run starts, run ids, find, unite, the unions of a word with the row above)
    over every mask of every set and over the framed complements fill_holes labels, in three visiting orders, against a flood
    fill; built with -fsanitize=address,undefined.  Its component counts must be the statement's."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    masks = []
    for name in CI.SETS:
        pm = CI.get(name)
        for i in range(len(pm)):
            m = pm.dense(i)
            if m.size:
                masks.append(m)
                if name in ("holes", "seam", "widths"):
                    frame = np.ones((m.shape[0] + 2, m.shape[1] + 2), bool)
                    frame[1:-1, 1:-1] = ~m
                    masks.append(frame)
    path = str(tmp_path / "masks.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(masks)).tobytes())
        for m in masks:
            f.write(np.array(m.shape, np.int32).tobytes())
            f.write(m.astype(np.uint8).tobytes())
    exe = str(tmp_path / "mask_cc_main")
    build = subprocess.run([cxx, "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "mask_cc_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler cannot link the sanitizers' runtimes")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
    assert len(lines) == len(masks)
    for m, (h, w, c4, c8) in zip(masks, lines):
        assert (h, w) == m.shape and c4 == CC.label_numpy(m, 4)[1] and c8 == CC.label_numpy(m, 8)[1]


# ---- refusals, without a device ----

def gone(*args, **kw):
    """Stands in for the library: touching it fails the test."""
    raise AssertionError("the library was looked for")


@pytest.mark.parametrize("call, message", [
    (lambda pm: CC.components(pm, 6), "components: connectivity=6 is not 4 or 8"),
    (lambda pm: CC.select(pm, 0), "select: connectivity=0 is not 4 or 8"),
    (lambda pm: CC.select(pm, 8, -1, 0), "select: min_area=-1 or keep=0 is negative"),
    (lambda pm: CC.select(pm, 8, 1, -2), "select: min_area=1 or keep=-2 is negative"),
    (lambda pm: CC.fill_holes(pm, 5), "fill_holes: connectivity=5 is not 4 or 8"),
    (lambda pm: CC.split(pm, 1), "split: connectivity=1 is not 4 or 8"),
    (lambda pm: pm.components(3), "components: connectivity=3 is not 4 or 8"),
    (lambda pm: pm.select(min_area=-5), "select: min_area=-5 or keep=0 is negative"),
    (lambda pm: pm.fill_holes(6), "fill_holes: connectivity=6 is not 4 or 8"),
    (lambda pm: pm.split(0), "split: connectivity=0 is not 4 or 8"),
    (lambda pm: CC.components_numpy(pm, 2), "components_numpy: connectivity=2 is not 4 or 8"),
    (lambda pm: CC.select_numpy(pm, 8, -1), "select_numpy: min_area=-1 or keep=0 is negative"),
    (lambda pm: CC.fill_holes_numpy(pm, 0), "fill_holes_numpy: connectivity=0 is not 4 or 8"),
    (lambda pm: CC.split_numpy(pm, 16), "split_numpy: connectivity=16 is not 4 or 8"),
])
def test_invalid_arguments_raise_by_name_before_the_library_is_looked_for(monkeypatch, call, message):
    monkeypatch.setattr(_lib, "call", gone)
    monkeypatch.setattr(_lib, "load", gone)
    with pytest.raises(ValueError) as e:
        call(CI.get("seam"))
    assert str(e.value) == message


def test_rows_out_of_order_are_refused_by_the_statements_of_select_and_fill_holes():
    pm = CI.get("seam")
    swapped = PackedMasks(pm.bounds[:2], pm.offsets[[1, 0]], pm.areas[:2], pm.classes[:2], pm.scores[:2], pm.bits)
    for f in (CC.select_numpy, CC.fill_holes_numpy):
        with pytest.raises(ValueError, match=r"the rows of masks\[1\] \(offset 0\) begin before the end of the rows before \(64\)"):
            f(swapped)
    CC.components_numpy(swapped), CC.split_numpy(swapped)          # these two write nowhere near the input's rows


class Set:
    """Two 10 x 10 masks of ones, good or with one flaw (tests/test_mask_set_host.py's); the arrays live as long as the object."""

    def __init__(self, flaw=None):
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
        elif flaw == "order":
            self.offsets[:] = (80, 0)
        else:
            assert flaw is None

    def args(self):
        return _lib.ptr(self.bounds), _lib.ptr(self.offsets), _lib.ptr(self.bits), self.nbytes, 2


FLAWS = {
    "coordinate": "masks[1] coordinate 16777216 out of range",
    "offset": "masks[1] offset 4 is negative or not a multiple of 8",
    "rows": "the rows of masks[1] (80 bytes at 80) reach past the 152 bytes given",
}


def out(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def entry(name, s, connectivity=8, min_area=1, keep=0, n=None):
    """-> (entry point, its arguments with every output filled with FILL, the outputs)."""
    p = _lib.ptr
    sa = s.args() if n is None else s.args()[:4] + (n,)
    if name == "mnc_mask_components":
        outs = [out(2100, np.int64), out(8, np.int64), out((8, 4), np.int32), out((8, 2), np.int32), out(1, np.uint64)]
        return name, sa + (connectivity,) + tuple(p(o) for o in outs[:4]) + (8, p(outs[4]), 0), outs
    if name == "mnc_mask_select":
        outs = [out(2, np.int64), out(20, np.uint64)]
        return name, sa + (connectivity, min_area, keep, p(outs[0]), p(outs[1]), outs[1].nbytes, 0), outs
    if name == "mnc_mask_fill_holes":
        outs = [out(2, np.int64), out(20, np.uint64)]
        return name, sa + (connectivity, p(outs[0]), p(outs[1]), outs[1].nbytes, 0), outs
    outs = [out((8, 4), np.int32), out(8, np.int64), out(8, np.int64), out(8, np.int32), out(1, np.uint64), out(40, np.uint64),
            out(1, np.uint64)]
    return name, sa + (connectivity,) + tuple(p(o) for o in outs[:4]) + (8, p(outs[4]), p(outs[5]), outs[5].nbytes, p(outs[6]), 0), outs


ENTRIES = ["mnc_mask_components", "mnc_mask_select", "mnc_mask_fill_holes", "mnc_mask_split"]


def refused(call, message):
    name, args, outs = call
    with pytest.raises(_lib.MncError) as e:
        _lib.call(name, *args)
    assert e.value.code == INVALID
    assert str(e.value) == "%s failed (status %d): %s: %s" % (name, INVALID, name, message)
    for o in outs:
        assert (o.view(np.uint8) == FILL).all()


@pytest.mark.parametrize("flaw", list(FLAWS))
@pytest.mark.parametrize("name", ENTRIES)
def test_a_flawed_set_is_refused_by_name_before_a_device_is_opened(name, flaw):
    refused(entry(name, Set(flaw)), FLAWS[flaw])


@pytest.mark.parametrize("name", ENTRIES)
def test_a_refused_parameter_writes_nothing(name):
    refused(entry(name, Set(), connectivity=6), "connectivity=6 is not 4 or 8")
    refused(entry(name, Set(), n=-1), "n=-1 not in [0, 2048]")
    refused(entry(name, Set(), n=2049), "n=2049 not in [0, 2048]")
    if name == "mnc_mask_select":
        refused(entry(name, Set(), min_area=-1), "min_area=-1 or keep=0 is negative")
        refused(entry(name, Set(), keep=-1), "min_area=1 or keep=-1 is negative")
    if name in ("mnc_mask_select", "mnc_mask_fill_holes"):
        refused(entry(name, Set("order")), "the rows of masks[1] (offset 0) begin before the end of the rows before (160)")


def test_the_word_limit_is_refused_by_the_library_and_by_the_statements():
    # 2048 instances that all point at the same 1025 rows of 16 words: past the limit of 2^25 words at instance 2046
    n, w, h = 2048, 2 ** 10, 2 ** 10 + 1
    bounds = np.tile(np.array([[0, 0, w - 1, h - 1]], np.int32), (n, 1))
    offsets = np.zeros(n, np.int64)
    bits = np.zeros(h * w // 64, np.uint64)
    s = Set()
    s.bounds, s.offsets, s.bits, s.nbytes = bounds, offsets, bits, bits.nbytes
    at = 2 ** 25 // (h * 16)
    for name in ("mnc_mask_components", "mnc_mask_split"):
        refused(entry(name, s, n=n), "more than 33554432 words of rows in the set (at masks[%d])" % at)
    pm = PackedMasks(bounds, offsets, np.zeros(n, np.int64), None, None, bits)
    with pytest.raises(ValueError, match=r"components_numpy: more than 33554432 words of rows in the set \(at masks\[%d\]\)" % at):
        CC.components_numpy(pm)


def test_empty_sets_are_answered_on_the_host():
    """n == 0 and sets without a single row: no device is opened (this test runs without one)."""
    none = MI.pack([], [])
    norows = MI.pack([[5, 5, 4, 9], [0, 0, 3, -1]], [np.zeros((5, 0), bool), np.zeros((0, 4), bool)], [1, 2], [0.5, 0.25])
    for pm in (none, norows):
        n = len(pm)
        for connectivity in CI.CONNECTIVITIES:
            t = CC.components(pm, connectivity, device_id=0)
            assert CI.same_components(t, CC.components_numpy(pm, connectivity)) and t.comp_ptr.tolist() == [0] * (n + 1)
            assert CI.same_masks(CC.select(pm, connectivity, device_id=0), CC.select_numpy(pm, connectivity))
            assert CI.same_masks(CC.fill_holes(pm, connectivity, device_id=0), CC.fill_holes_numpy(pm, connectivity))
            parts, source = CC.split(pm, connectivity, device_id=0)
            want, want_source = CC.split_numpy(pm, connectivity)
            assert CI.same_masks(parts, want) and CI.same_array(source, want_source) and len(parts) == 0


def test_n12_is_declared_and_exported():
    decls = _lib.parse_header()
    lib = _lib.load()
    for name in ENTRIES + ["mnc_mask_components_timing"]:
        assert name in decls and hasattr(lib, name)
    assert decls["mnc_mask_components"][2] == ["bounds", "offsets", "bits", "bytes", "n", "connectivity", "comp_ptr", "area", "bbox",
                                               "anchor", "comp_cap", "n_comp", "device_id"]
    assert decls["mnc_mask_select"][2] == ["bounds", "offsets", "bits", "bytes", "n", "connectivity", "min_area", "keep", "out_areas",
                                           "out_bits", "bits_cap", "device_id"]
    assert decls["mnc_mask_fill_holes"][2] == ["bounds", "offsets", "bits", "bytes", "n", "connectivity", "out_areas", "out_bits",
                                               "bits_cap", "device_id"]
    assert decls["mnc_mask_split"][2] == ["bounds", "offsets", "bits", "bytes", "n", "connectivity", "out_bounds", "out_offsets",
                                          "out_areas", "out_source", "comp_cap", "n_comp", "out_bits", "bits_cap", "bits_bytes",
                                          "device_id"]
