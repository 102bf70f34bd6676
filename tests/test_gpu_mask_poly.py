"""COCO polygon segmentations rasterised into packed masks on the GPU (csrc/mask_poly.hip: mnc_mask_from_polygons and the Python
surfaces over it) against the numpy statement (mnc_amd.polygons.masks_from_polygons_numpy, which tests/test_mask_poly_host.py pins
to two facts that do not come from it).  Every comparison is exact.  The cases are those of tests/mask_poly_inputs.py: images no
larger than 180 x 200, placed where the kernels can go wrong."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_poly_inputs as PI  # noqa: E402
from mnc_amd import _lib, polygons, rle  # noqa: E402
from mnc_amd.masks import PackedMasks, mask_overlaps_numpy  # noqa: E402

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in PI.CASES}


def _same_masks(got, want):
    for f in ("bounds", "offsets", "areas", "bits"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
    return True


@pytest.mark.parametrize("case", PI.CASES, ids=PI.IDS)
def test_device_equals_the_numpy_statement(case):
    want = PI.reference(case)
    got = polygons.masks_from_polygons(case.segs, case.H, case.W)
    assert _same_masks(got, want)
    again = PackedMasks.from_polygons(case.segs, case.H, case.W)                   # the same bytes from run to run
    assert all(getattr(again, f).tobytes() == getattr(got, f).tobytes() for f in PackedMasks.FIELDS)


def test_sizes_only_and_too_little_room():
    case = BY_NAME["unions"]
    want = PI.reference(case)
    segs, H, W = polygons._check_segs("test", case.segs, case.H, case.W)
    xy, vert_ptr, poly_ptr = polygons._flatten(segs)
    bounds, offsets, areas, need = polygons.masks_from_polygons_call(xy, vert_ptr, poly_ptr, H, W)        # bits == NULL
    assert need == want.bits.nbytes and np.array_equal(bounds, want.bounds) and np.array_equal(offsets, want.offsets)
    assert np.array_equal(areas, want.areas)
    n = len(case.segs)
    out, size = np.zeros((n, 4), np.int32), ctypes.c_size_t(0)
    small = np.full(need // 8 - 1, 0x5555555555555555, np.uint64)
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_mask_from_polygons", _lib.ptr(xy), _lib.ptr(vert_ptr), _lib.ptr(poly_ptr), n, H, W, _lib.ptr(out),
                  _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(small), small.nbytes, ctypes.addressof(size), 0)
    assert e.value.code == 1 and size.value == need and (small == np.uint64(0x5555555555555555)).all()
    assert np.array_equal(out, want.bounds)
    # room to spare: the bytes behind the masks stay as they were
    roomy = np.full(need // 8 + 4, 0x5555555555555555, np.uint64)
    polygons.masks_from_polygons_call(xy, vert_ptr, poly_ptr, H, W, roomy)
    assert np.array_equal(roomy[:need // 8], want.bits) and (roomy[need // 8:] == np.uint64(0x5555555555555555)).all()
    # a poly_ptr and a vert_ptr that do not begin at 0
    shifted = polygons.masks_from_polygons_call(np.concatenate(([9.0, 9.0, 9.0, 9.0], xy)), np.concatenate(([0], vert_ptr + 2)),
                                                poly_ptr + 1, H, W, roomy)
    assert np.array_equal(shifted[0], want.bounds) and np.array_equal(roomy[:need // 8], want.bits)
    none = polygons.masks_from_polygons([], 5, 5)
    assert len(none) == 0 and none.bits.size == 0
    only_empty = polygons.masks_from_polygons([[], [[-9.0, -9.0, -5.0, -9.0, -5.0, -5.0]]], 5, 5)
    assert only_empty.bounds.tolist() == [[0, 0, -1, -1]] * 2 and only_empty.bits.size == 0


def test_rle_counts_of_the_rasterised_masks():
    for name in ("leaving_and_outside", "size_37x130"):
        case = BY_NAME[name]
        want = rle.rle_counts_numpy(PI.reference(case), case.H, case.W)
        got = PackedMasks.from_polygons(case.segs, case.H, case.W).rle_counts(case.H, case.W)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_from_segmentations_on_a_mixed_list():
    case = BY_NAME["unions"]
    H, W = case.H, case.W
    other = PI.reference(BY_NAME["leaving_and_outside"])
    rles = rle.mask_rle_numpy(other, H, W)
    loose = {"size": [H, W], "counts": rle.string_to_counts(rles[1]["counts"]).tolist()}      # an uncompressed one
    segs = [rles[0], case.segs[0], case.segs[1], loose, case.segs[3], rles[6], case.segs[2]]
    classes, scores = np.arange(7) + 1, np.linspace(0.1, 0.7, 7)
    got = PackedMasks.from_segmentations(segs, H, W, classes, scores)
    want = polygons.masks_from_segmentations(segs, H, W, classes, scores, cpu=True)
    assert _same_masks(got, want) and np.array_equal(got.classes, classes) and np.array_equal(got.scores, scores.astype(np.float32))
    polys, decoded = PI.reference(case), rle.masks_from_rle_numpy(rles)
    picks = [(decoded, 0), (polys, 0), (polys, 1), (decoded, 1), (polys, 3), (decoded, 6), (polys, 2)]
    for k, (pm, i) in enumerate(picks):
        assert got.bounds[k].tolist() == pm.bounds[i].tolist() and np.array_equal(got.full(k, H, W), pm.full(i, H, W))


def test_overlaps_between_a_polygon_set_and_an_rle_set():
    case = BY_NAME["unions"]
    H, W = case.H, case.W
    a = PackedMasks.from_polygons(case.segs, H, W)
    b = PackedMasks.from_rle(rle.mask_rle_numpy(PI.reference(BY_NAME["leaving_and_outside"]), H, W))
    inter, iou = a.overlaps(b)
    want = mask_overlaps_numpy(PI.reference(case), b)
    assert np.array_equal(inter, want[0]) and np.array_equal(iou, want[1]) and (inter > 0).any()


def test_eval_coco_polygons_on_the_gpu_prints_the_cpu_lines(tmp_path):
    gt, _, dt, _ = PI.coco_files(tmp_path)
    dev = PI.tool("--gt", gt, "--dt", dt, "--polygons")
    cpu = PI.tool("--gt", gt, "--dt", dt, "--polygons", "--cpu")
    assert dev.returncode == 0 and cpu.returncode == 0, (dev.stderr[-2000:], cpu.stderr[-2000:])
    assert dev.stdout == cpu.stdout and len([ln for ln in dev.stdout.splitlines() if ln.startswith(" Average")]) == 12
