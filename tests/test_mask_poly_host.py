"""COCO polygon segmentations rasterised into packed masks, the parts that need no GPU (mnc_amd/polygons.py): the numpy statement of
maskApi.c's rule against two facts that do not come from it -- an integer rectangle sets exactly its pixels, and the mask differs
from an even-odd test at the pixel centres only within half a pixel of an edge -- its two forms (sort and merge; parity of the
toggles) against each other, the PackedMasks invariants, tools/eval_coco.py --cpu --polygons, and the argument checks of
mnc_mask_from_polygons, all of which happen before a device is looked for."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_poly_inputs as PI  # noqa: E402
from mnc_amd import _lib, polygons, rle  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402


def _mask(xy, H, W):
    return polygons._decode(polygons.polygon_counts_numpy(xy, H, W), H, W)


def test_independent_an_integer_rectangle_sets_exactly_its_pixels():
    sizes = [(6, 7, 1), (8, 10, 3), (5, 130, 9), (37, 65, 11)]
    for H, W, step in sizes:
        xs = sorted(set(range(0, W + 1, step)) | {0, W, min(63, W), min(64, W), min(65, W)})
        ys = sorted(set(range(0, H + 1, step)) | {0, H})
        for x0 in xs:
            for x1 in (x for x in xs if x > x0):
                for y0 in ys:
                    for y1 in (y for y in ys if y > y0):
                        want = np.zeros((H, W), bool)
                        want[y0:y1, x0:x1] = True
                        assert np.array_equal(_mask(PI.rect(x0, y0, x1, y1), H, W), want), (H, W, x0, y0, x1, y1)
    want = np.zeros((8, 10), bool)
    want[1:5, 2:7] = True
    assert np.array_equal(_mask([2, 1, 7, 1, 7, 5, 2, 5], 8, 10), want)


def _even_odd(pts, H, W):
    """bool [H, W]: the crossing-number test at the pixel centres (x + .5, y + .5)."""
    px, py = np.meshgrid(np.arange(W) + .5, np.arange(H) + .5)
    inside = np.zeros((H, W), bool)
    for (xi, yi), (xj, yj) in zip(pts, np.roll(pts, -1, axis=0)):
        if yi == yj:
            continue
        hit = ((yi > py) != (yj > py)) & (px < xi + (py - yi) * (xj - xi) / (yj - yi))
        inside ^= hit
    return inside


def _distance_to_edges(pts, x, y):
    best = np.full(len(x), np.inf)
    for a, b in zip(pts, np.roll(pts, -1, axis=0)):
        ab = b - a
        t = np.clip(((x - a[0]) * ab[0] + (y - a[1]) * ab[1]) / max(float(ab @ ab), 1e-300), 0.0, 1.0)
        best = np.minimum(best, np.hypot(x - (a[0] + t * ab[0]), y - (a[1] + t * ab[1])))
    return best


def test_independent_disagreement_with_an_even_odd_test_lies_within_half_a_pixel_of_an_edge():
    rng = np.random.default_rng(0)
    worst = disagreeing = 0
    for _ in range(300):
        H, W = int(rng.integers(5, 70)), int(rng.integers(5, 90))
        k = int(rng.integers(3, 9))
        pts = rng.uniform((0, 0), (W, H), (k, 2))                                  # inside the image
        got = _mask(pts.reshape(-1), H, W)
        ys, xs = np.nonzero(got != _even_odd(pts, H, W))
        if len(xs):
            d = _distance_to_edges(pts, xs + .5, ys + .5)
            worst, disagreeing = max(worst, float(d.max())), disagreeing + len(xs)
    print("pixels that disagree: %d, the farthest %.3f px from an edge" % (disagreeing, worst))
    assert worst <= 0.5


@pytest.mark.parametrize("case", PI.CASES, ids=PI.IDS)
def test_parity_form_equals_sort_and_merge(case):
    for polys in case.segs:
        for xy in polys:
            counts = polygons.polygon_counts_numpy(xy, case.H, case.W)
            assert counts.dtype == np.uint32 and int(counts.astype(np.int64).sum()) == case.H * case.W
            assert np.array_equal(polygons._decode(counts, case.H, case.W), polygons.polygon_mask_parity_numpy(xy, case.H, case.W))


def test_the_inputs_hold_clamped_crossings_and_odd_carries():
    facts = {c.name: PI.clamped_and_carried(c) for c in PI.CASES}
    assert facts["leaving_and_outside"][0] > 0 and facts["leaving_and_outside"][1] > 0
    assert facts["windings_and_starts"] == (0, 0)                                  # ... and none where the polygon stays inside


@pytest.mark.parametrize("case", PI.CASES, ids=PI.IDS)
def test_packed_masks_invariants(case):
    pm = PI.reference(case)
    H, W = case.H, case.W
    assert len(pm) == len(case.segs) and pm.bounds.dtype == np.int32 and pm.offsets.dtype == np.int64 and pm.bits.dtype == np.uint64
    at = 0
    for i, polys in enumerate(case.segs):
        want = np.zeros((H, W), bool)
        for xy in polys:
            want |= polygons.polygon_mask_parity_numpy(xy, H, W)
        assert np.array_equal(pm.full(i, H, W), want) and pm.areas[i] == want.sum()
        assert pm.offsets[i] == at and at % 8 == 0
        h, w = pm.size(i)
        if not want.any():
            assert pm.bounds[i].tolist() == [0, 0, -1, -1] and (h, w) == (0, 0)
            continue
        ys, xs = np.nonzero(want)
        assert pm.bounds[i].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]
        words = pm.bits[at // 8:at // 8 + h * ((w + 63) // 64)].reshape(h, -1)
        if w % 64:
            assert not (words[:, -1] >> np.uint64(w % 64)).any()                   # padding bits are 0
        at += words.size * 8
    assert pm.bits.nbytes == at


def test_union_empty_outside_and_degenerate_cases():
    by_name = {c.name: c for c in PI.CASES}
    un, pm = by_name["unions"], PI.reference(by_name["unions"])
    a, b = (_mask(xy, un.H, un.W) for xy in un.segs[0])
    assert (a & b).any() and np.array_equal(pm.full(0, un.H, un.W), a | b) and pm.areas[0] == (a | b).sum() > (a ^ b).sum()
    assert pm.areas[3] == 0 and pm.bounds[3].tolist() == [0, 0, -1, -1]            # no polygons
    assert pm.areas[4] == 100                                                      # the same polygon twice is itself, not nothing
    assert pm.areas[5] == 36 and pm.bounds[5].tolist() == [3, 3, 8, 8]
    out = PI.reference(by_name["leaving_and_outside"])
    assert (out.areas[:6] > 0).all() and (out.areas[6:] == 0).all()                # the five polygons outside are empty
    deg = PI.reference(by_name["degenerate"])
    assert deg.areas[0] == 0 and deg.areas[3] == 0 and deg.areas[2] == 400         # one vertex; thrice one vertex; doubled vertices
    empty = polygons.masks_from_polygons_numpy([], 5, 5)
    assert len(empty) == 0 and empty.bits.size == 0


def test_argument_checks_of_the_python_side():
    with pytest.raises(ValueError, match="polygon 1 of segmentation 2"):
        polygons.masks_from_polygons_numpy([[], [[1, 1, 2, 2, 3, 1]], [[1, 1, 2, 2, 3, 1], [1, 2, 3]]], 5, 5)
    with pytest.raises(ValueError, match="polygon 0 of segmentation 1"):
        PackedMasks.from_polygons([[], [[1.0, 2.0, 3.0]]], 5, 5)                   # refused before the library is looked for
    with pytest.raises(ValueError, match="polygon 0 of segmentation 0"):
        PackedMasks.from_polygons([[[]]], 5, 5)
    for bad in (float("nan"), float("inf"), 2.0 ** 20 + 1):
        with pytest.raises(ValueError):
            polygons.masks_from_polygons_numpy([[[1, 1, bad, 2, 3, 1]]], 5, 5)
    with pytest.raises(ValueError):
        polygons.masks_from_polygons_numpy([[[1, 1, 2, 2, 3, 1]]], 0, 5)
    with pytest.raises(ValueError):
        polygons.masks_from_polygons_numpy([[[1, 1, 2, 2, 3, 1]]], 32768, 32768 + 1)
    with pytest.raises(ValueError, match="segmentation 1"):
        polygons.masks_from_segmentations([[[1, 1, 4, 1, 4, 4]], {"size": [4, 5], "counts": [20]}], 5, 5, cpu=True)
    mixed = polygons.masks_from_segmentations([{"size": [5, 5], "counts": [0, 25]}, [[1, 1, 4, 1, 4, 4, 1, 4]],
                                               {"size": [5, 5], "counts": rle.counts_to_string([6, 2, 17])}], 5, 5, [3, 4, 5], cpu=True)
    assert mixed.areas.tolist() == [25, 9, 2] and mixed.classes.tolist() == [3, 4, 5] and mixed.offsets.tolist() == [0, 40, 64]
    assert mixed.bounds.tolist() == [[0, 0, 4, 4], [1, 1, 3, 3], [1, 1, 1, 2]]


def _call(xy, vert_ptr, poly_ptr, n, H, W, bits=None, cap=0):
    """mnc_mask_from_polygons as it is -> (the status, the message, *bits_bytes)."""
    xy = np.ascontiguousarray(xy, np.float64)
    vert_ptr, poly_ptr = np.ascontiguousarray(vert_ptr, np.int64), np.ascontiguousarray(poly_ptr, np.int64)
    m = max(n, 1)
    bounds, offsets, areas, need = np.zeros((m, 4), np.int32), np.zeros(m, np.int64), np.zeros(m, np.int64), ctypes.c_size_t(77)
    try:
        _lib.call("mnc_mask_from_polygons", _lib.ptr(xy), _lib.ptr(vert_ptr), _lib.ptr(poly_ptr), n, H, W, _lib.ptr(bounds),
                  _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits), cap, ctypes.addressof(need), 0)
    except _lib.MncError as e:
        return e.code, str(e), need.value
    return 0, "", need.value


def test_c_abi_refusals_come_before_any_device_work():
    tri = [1.0, 1.0, 4.0, 1.0, 4.0, 4.0]
    invalid = 1                                                                    # MNC_ERR_INVALID
    assert _call(tri, [0, 3], [0, 1], 0, 5, 5) == (0, "", 0)                       # n == 0: nothing to do, no device looked for
    assert _call(tri, [0, 3], [0, 1], -1, 5, 5)[0] == invalid and _call(tri, [0, 3], [0] * 2050, 2049, 5, 5)[0] == invalid
    for H, W in ((0, 5), (5, 0), (32769, 5), (5, 32769), (-1, 5), (32769, 32769)):
        assert _call(tri, [0, 3], [0, 1], 1, H, W)[0] == invalid, (H, W)
    assert _call(tri, [0, 3], [-1, 0], 1, 5, 5)[0] == invalid                      # a negative poly_ptr
    assert _call(tri, [0, 3], [1, 0], 1, 5, 5)[0] == invalid                       # a decreasing one
    assert _call(tri, [0, 3, 2], [0, 2], 1, 5, 5)[0] == invalid                    # a decreasing vert_ptr
    assert _call(tri, [-1, 3], [0, 1], 1, 5, 5)[0] == invalid                      # a negative one
    code, msg, _ = _call(tri, [0, 3, 3], [0, 2], 1, 5, 5)
    assert code == invalid and "polygon 1 has no vertices" in msg
    for bad in (float("nan"), float("inf"), -float("inf"), 2.0 ** 20 + 1, -(2.0 ** 20) - 1):
        assert _call([1.0, 1.0, bad, 1.0, 4.0, 4.0], [0, 3], [0, 1], 1, 5, 5)[0] == invalid, bad
    # two vertices 2^20 apart walk 5 * 2^20 + 1 points there and as many back: 103 such polygons pass 2^30
    far = np.tile([0.0, 0.0, 2.0 ** 20, 0.0], 103)
    code, msg, _ = _call(far, np.arange(104) * 2, [0, 103], 1, 5, 5)
    assert code == invalid and "2^30 points" in msg


def test_eval_coco_cpu_polygons_equals_the_prerasterised_file(tmp_path):
    gt, gt_rle, dt, dt_rle = PI.coco_files(tmp_path)
    got = PI.tool("--gt", gt, "--dt", dt, "--cpu", "--polygons", "--out", str(tmp_path / "a.json"))
    want = PI.tool("--gt", gt_rle, "--dt", dt_rle, "--cpu", "--out", str(tmp_path / "b.json"))
    assert got.returncode == 0 and want.returncode == 0, (got.stderr[-2000:], want.stderr[-2000:])
    with open(str(tmp_path / "a.json")) as f:
        a = json.load(f)
    with open(str(tmp_path / "b.json")) as f:
        b = json.load(f)
    assert len(a["stats"]) == 12 and a["stats"] == b["stats"] and a["lines"] == b["lines"] and got.stdout == want.stdout
    assert 0 < a["stats"]["AP"] < 1
    # with the flag an RLE-only file scores as without it; without it a polygon is still refused
    assert PI.tool("--gt", gt_rle, "--dt", dt_rle, "--cpu", "--polygons").stdout == want.stdout
    refused = PI.tool("--gt", gt, "--dt", dt_rle, "--cpu")
    assert refused.returncode != 0 and "polygon" in refused.stderr
