"""Connected components of packed instance masks on the GPU (csrc/mask_components.hip: mnc_mask_components, mnc_mask_select,
mnc_mask_fill_holes, mnc_mask_split and the Python surfaces over them) against the numpy statements of mnc_amd.components, which
tests/test_mask_components_host.py pins to scipy.ndimage and to closed forms.  Every comparison is exact: dtype, shape and bytes.
The shapes are those of tests/mask_components_inputs.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_components_inputs as CI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import components as CC  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
FILL = 0x5a


@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CI.SETS))
def test_components_equal_the_statement(name, connectivity):
    got = CC.components(CI.get(name), connectivity)
    want = CI.reference(name, "components", connectivity)
    assert got.comp_ptr.tolist() == want.comp_ptr.tolist()
    assert CI.same_components(got, want)


@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CI.SETS))
def test_select_equals_the_statement(name, connectivity):
    for min_area, keep in CI.SELECTIONS:
        got = CC.select(CI.get(name), connectivity, min_area, keep)
        want = CI.reference(name, "select", connectivity, min_area, keep)
        assert got.areas.tolist() == want.areas.tolist(), (min_area, keep)
        assert CI.same_masks(got, want), (min_area, keep)


@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CI.SETS))
def test_fill_holes_equals_the_statement(name, connectivity):
    got = CC.fill_holes(CI.get(name), connectivity)
    want = CI.reference(name, "fill_holes", connectivity)
    assert got.areas.tolist() == want.areas.tolist()
    assert CI.same_masks(got, want)


@pytest.mark.parametrize("connectivity", CI.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(CI.SETS))
def test_split_equals_the_statement(name, connectivity):
    got, source = CC.split(CI.get(name), connectivity)
    want, want_source = CI.reference(name, "split", connectivity)
    assert CI.same_array(source, want_source)
    assert got.bounds.tolist() == want.bounds.tolist() and got.areas.tolist() == want.areas.tolist()
    assert CI.same_masks(got, want)


def test_stripes_whose_runs_fill_more_than_256_scan_tiles():
    """308 891 runs are 302 tiles of 1024: the scan over the tiles takes a second pass of 256, for the words' counts (the run ids)
    and for the root flags (the component numbers) alike."""
    pm = CI.get("stripes")
    for connectivity in CI.CONNECTIVITIES:
        want = CI.reference("stripes", "components", connectivity)
        assert len(want.area) == 3666 and int(pm.areas[0]) > 257 * 1024      # every set pixel is a run
        assert CI.same_components(CC.components(pm, connectivity), want)
    assert CI.same_masks(CC.select(pm, 4, 50, 0), CI.reference("stripes", "select", 4, 50, 0))
    got, source = CC.split(pm, 4)
    want, want_source = CI.reference("stripes", "split", 4)
    assert CI.same_array(source, want_source) and CI.same_masks(got, want)


def test_real_size_twice_the_same_bytes_and_every_surface_agrees():
    pm = CI.get("real")
    for connectivity in CI.CONNECTIVITIES:
        first = (CC.components(pm, connectivity), CC.select(pm, connectivity, 20, 1), CC.fill_holes(pm, connectivity),
                 CC.split(pm, connectivity))
        again = (CC.components(pm, connectivity), CC.select(pm, connectivity, 20, 1), CC.fill_holes(pm, connectivity),
                 CC.split(pm, connectivity))
        method = (pm.components(connectivity), pm.select(connectivity, 20, 1), pm.fill_holes(connectivity), pm.split(connectivity))
        export = (MT.mask_components(pm, connectivity), MT.mask_select(pm, connectivity, 20, 1), MT.mask_fill_holes(pm, connectivity),
                  MT.mask_split(pm, connectivity))
        for other in (again, method, export):
            assert CI.same_components(other[0], first[0])
            assert CI.same_masks(other[1], first[1]) and CI.same_masks(other[2], first[2])
            assert CI.same_masks(other[3][0], first[3][0]) and CI.same_array(other[3][1], first[3][1])
        assert CI.same_masks(first[1], CI.reference("real", "select", connectivity, 20, 1))


# ---- the room ----

def filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


def raw_components(pm, connectivity, cap):
    outs = [filled(len(pm) + 1, np.int64), filled(cap, np.int64), filled((cap, 4), np.int32), filled((cap, 2), np.int32)]
    count = ctypes.c_size_t(12345)
    args = _set_args(pm, areas=False) + (connectivity,) + tuple(_lib.ptr(o) for o in outs) + (cap, ctypes.addressof(count), 0)
    return args, outs, count


def raw_split(pm, connectivity, cap, words):
    outs = [filled((cap, 4), np.int32), filled(cap, np.int64), filled(cap, np.int64), filled(cap, np.int32), filled(words, np.uint64)]
    count, nbytes = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
    args = (_set_args(pm, areas=False) + (connectivity,) + tuple(_lib.ptr(o) for o in outs[:4]) +
            (cap, ctypes.addressof(count), _lib.ptr(outs[4]), outs[4].nbytes, ctypes.addressof(nbytes), 0))
    return args, outs, count, nbytes


@pytest.mark.parametrize("name", ["widths", "holes"])
def test_buffers_with_room_to_spare_keep_their_tail(name):
    pm = CI.get(name)
    want = CI.reference(name, "components", 4)
    C = len(want.area)
    args, outs, count = raw_components(pm, 4, C + 7)
    _lib.call("mnc_mask_components", *args)
    assert count.value == C and CI.same_array(outs[0], want.comp_ptr)
    for o, w in zip(outs[1:], want[1:]):
        assert CI.same_array(o[:C], w) and untouched(o[C:])
    parts, source = CI.reference(name, "split", 4)
    args, outs, count, nbytes = raw_split(pm, 4, C + 5, parts.bits.size + 9)
    _lib.call("mnc_mask_split", *args)
    assert count.value == C and nbytes.value == parts.bits.nbytes
    for o, w in zip(outs, (parts.bounds, parts.offsets, parts.areas, source)):
        assert CI.same_array(o[:C], w) and untouched(o[C:])
    assert CI.same_array(outs[4][:parts.bits.size], parts.bits) and untouched(outs[4][parts.bits.size:])
    # select and fill_holes: the words behind the rows stay as they were
    for entry, head, ref in (("mnc_mask_select", (4, 1, 0), CI.reference(name, "select", 4, 1, 0)),
                             ("mnc_mask_fill_holes", (4,), CI.reference(name, "fill_holes", 4))):
        areas, bits = filled(len(pm), np.int64), filled(pm.bits.size + 11, np.uint64)
        _lib.call(entry, *(_set_args(pm, areas=False) + head + (_lib.ptr(areas), _lib.ptr(bits), bits.nbytes, 0)))
        assert CI.same_array(areas, ref.areas) and CI.same_array(bits[:pm.bits.size], ref.bits) and untouched(bits[pm.bits.size:])


def test_too_little_room_reports_the_sizes_and_writes_nothing_else():
    pm = CI.get("widths")
    want = CI.reference("widths", "components", 8)
    C = len(want.area)
    args, outs, count = raw_components(pm, 8, C - 1)
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_mask_components", *args)
    assert e.value.code == INVALID and "comp_cap %d is below the %d components" % (C - 1, C) in str(e.value)
    assert count.value == C and CI.same_array(outs[0], want.comp_ptr) and all(untouched(o) for o in outs[1:])
    # no table at all: the sizes only
    t, n_comp = CC.components_call(pm, 8, 0, sizes_only=True)
    assert n_comp == C and CI.same_array(t.comp_ptr, want.comp_ptr)
    parts, _ = CI.reference("widths", "split", 8)
    for cap, words in ((C - 1, parts.bits.size), (C, parts.bits.size - 1)):
        args, outs, count, nbytes = raw_split(pm, 8, cap, words)
        with pytest.raises(_lib.MncError) as e:
            _lib.call("mnc_mask_split", *args)
        assert e.value.code == INVALID and count.value == C and nbytes.value == parts.bits.nbytes
        assert all(untouched(o) for o in outs)
    assert CC.split_call(pm, 8, 0, None)[4:] == (C, parts.bits.nbytes)
    # the wrappers come back with room when their first guess was too small (the checkerboard has 4290 components)
    assert len(CC.components(CI.get("checker"), 4).area) == 4290 and len(CC.split(CI.get("checker"), 4)[0]) == 4290
    for entry, head in (("mnc_mask_select", (8, 1, 0)), ("mnc_mask_fill_holes", (8,))):
        areas, bits = filled(len(pm), np.int64), filled(pm.bits.size - 1, np.uint64)
        with pytest.raises(_lib.MncError) as e:
            _lib.call(entry, *(_set_args(pm, areas=False) + head + (_lib.ptr(areas), _lib.ptr(bits), bits.nbytes, 0)))
        assert e.value.code == INVALID and "bits_cap" in str(e.value) and untouched(areas) and untouched(bits)


def test_invalid_arguments_are_refused_with_nothing_written():
    pm = CI.get("seam")
    for connectivity, n in ((5, len(pm)), (8, -1), (4, 4096)):
        args, outs, count = raw_components(pm, connectivity, 64)
        args = args[:4] + (n,) + args[5:]
        with pytest.raises(_lib.MncError) as e:
            _lib.call("mnc_mask_components", *args)
        assert e.value.code == INVALID and count.value == 12345 and all(untouched(o) for o in outs)
        args, outs, count, nbytes = raw_split(pm, connectivity, 64, 1024)
        args = args[:4] + (n,) + args[5:]
        with pytest.raises(_lib.MncError) as e:
            _lib.call("mnc_mask_split", *args)
        assert e.value.code == INVALID and count.value == 12345 and nbytes.value == 12345 and all(untouched(o) for o in outs)
    for entry, head in (("mnc_mask_select", (8, -1, 0)), ("mnc_mask_select", (8, 1, -1)), ("mnc_mask_select", (3, 1, 0)),
                        ("mnc_mask_fill_holes", (0,))):
        areas, bits = filled(len(pm), np.int64), filled(pm.bits.size, np.uint64)
        with pytest.raises(_lib.MncError) as e:
            _lib.call(entry, *(_set_args(pm, areas=False) + head + (_lib.ptr(areas), _lib.ptr(bits), bits.nbytes, 0)))
        assert e.value.code == INVALID and untouched(areas) and untouched(bits)


# ---- the demo ----

def test_demo_min_component_area_selects_what_is_written(tmp_path):
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
    h, w = im.shape[:2]
    got, saved = {}, {}
    for key, flags in (("plain", []), ("selected", ["--min-component-area", "30", "--largest-component"])):
        out = str(tmp_path / (key + ".json"))
        os.makedirs(str(tmp_path / key))
        with redirect_stdout(io.StringIO()):
            demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-coco", out, "--save-masks", str(tmp_path / key),
                       "--vis-thresh", "0.0"] + flags)
        with open(out) as f:
            got[key] = json.load(f)
        saved[key] = PackedMasks.load(str(tmp_path / key / (name + "_masks.npz")))
    # without the flags: what the statement of the existing output gives (tests/test_gpu_mask_rle.py's check), byte for byte
    pm = saved["plain"]
    assert len(pm) > 0 and got["plain"] == json.loads(json.dumps(demo._coco_results(name, im.shape, pm, cpu=True)))
    # with them: every written mask is select_numpy of the unflagged one
    want = CC.select_numpy(pm, 8, 30, 1)
    assert CI.same_masks(saved["selected"], want)
    assert got["selected"] == json.loads(json.dumps(demo._coco_results(name, im.shape, want, cpu=True)))
    back = PackedMasks.from_rle([e["segmentation"] for e in got["selected"]])
    assert all(np.array_equal(back.full(i, h, w), want.full(i, h, w)) for i in range(len(pm)))
    assert int(want.areas.sum()) < int(pm.areas.sum())             # the selection removed something
