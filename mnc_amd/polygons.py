"""COCO polygon segmentations rasterised into packed masks (include/mnc_hip.h n9, csrc/mask_poly.hip): the rule of the published
maskApi.c, rleFrPoly per polygon and the union of an annotation's polygons (annToRLE: frPyObjects, then merge).  A polygon is
walked edge by edge at five times the image's resolution; where the walk passes from one image column into the next stands a
crossing; the crossings' positions in the column-major pixel order (p = x * H + y, as mnc_amd/rle.py), sorted, are the ends of
the runs.

    polygon_walk_numpy(xy)                  steps 1 and 2 of the rule: the points (u, v) of one polygon's walk
    polygon_crossings_numpy(xy, H, W)       step 3: the positions the crossings toggle, in walk order
    polygon_counts_numpy(xy, H, W)          step 4, sort and merge: the counts of one polygon (uint32)
    polygon_mask_parity_numpy(xy, H, W)     the same pixels said the other way: set where the toggles at positions <= p are odd
    masks_from_polygons_numpy(segs, H, W)   the CPU statement: per annotation the OR of its polygons' decoded counts -> PackedMasks
    masks_from_polygons(segs, H, W)         the same PackedMasks through mnc_mask_from_polygons (the GPU)
    masks_from_segmentations(segs, H, W)    polygon lists and RLE dicts mixed, order kept (PackedMasks.from_segmentations)

segs[i] is the `segmentation` of annotation i: a list of polygons, each a flat list [x0, y0, x1, y1, ...].  There is no fallback:
without the library or a GPU the device functions raise."""
import ctypes
import math

import numpy as np

from . import _lib
from .masks import PackedMasks, _device_id, merge_sets, sized_then_filled  # noqa: F401 (merge_sets: its public name here)
from .rle import MAX_MASKS, _check_image, counts_of_rles, masks_from_counts, masks_from_counts_numpy

MAX_COORD = 2.0 ** 20
MAX_PIXELS = 2 ** 30


def _trunc(a):
    return np.trunc(a).astype(np.int64)


def _vertices(xy, who="polygon"):
    xy = np.asarray(xy, np.float64).reshape(-1)
    if xy.size == 0 or xy.size % 2:
        raise ValueError("%s: %d coordinates are not x, y pairs of at least one vertex" % (who, xy.size))
    if not (np.isfinite(xy).all() and (np.abs(xy) <= MAX_COORD).all()):
        raise ValueError("%s: a coordinate is not finite or of magnitude above 2^20" % who)
    return xy


def polygon_walk_numpy(xy):
    """Steps 1 and 2: the vertices rounded to a fifth of a pixel, every edge (the last one back to the first vertex) walked one
    unit of its longer side at a time.  -> (u, v) int64, the points of all edges in edge order."""
    xy = _vertices(xy)
    X, Y = _trunc(5 * xy[0::2] + .5), _trunc(5 * xy[1::2] + .5)
    X, Y = np.append(X, X[0]), np.append(Y, Y[0])
    us, vs = [], []
    for j in range(len(X) - 1):
        xs, xe, ys, ye = int(X[j]), int(X[j + 1]), int(Y[j]), int(Y[j + 1])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        d = np.arange(max(dx, dy) + 1, dtype=np.int64)
        t = (max(dx, dy) - d if flip else d)
        if dx >= dy:
            # (0 / 0 in the published code when dx == dy == 0; that v is never read: u does not change across the point)
            s = float(ye - ys) / dx if dx else 0.0
            us.append(t + xs)
            vs.append(_trunc(ys + s * t.astype(np.float64) + .5))
        else:
            s = float(xe - xs) / dy
            vs.append(t + ys)
            us.append(_trunc(xs + s * t.astype(np.float64) + .5))
    return np.concatenate(us), np.concatenate(vs)


def polygon_crossings_numpy(xy, H, W):
    """Step 3 as the plain loop over the walk: -> (x, y) int64 of the crossings in walk order, 0 <= x <= W - 1, 0 <= y <= H
    (y == H: clamped; its position x * H + H is the first pixel of the next column)."""
    u, v = polygon_walk_numpy(xy)
    xs, ys = [], []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / 5 - .5
        if math.floor(xd) != xd or xd < 0 or xd > W - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / 5 - .5
        yd = math.ceil(0.0 if yd < 0 else float(H) if yd > H else yd)
        xs.append(int(xd))
        ys.append(int(yd))
    return np.array(xs, np.int64), np.array(ys, np.int64)


def polygon_counts_numpy(xy, H, W):
    """The counts of one polygon in an H x W image (uint32, summing to H * W): the crossings' positions sorted, H * W appended,
    their differences, every run of length 0 but the first merged into its neighbours -- rleFrPoly's last loop as it stands."""
    H, W = int(H), int(W)
    _check_image("polygon_counts_numpy", H, W)
    x, y = polygon_crossings_numpy(xy, H, W)
    a = np.diff(np.concatenate((np.sort(x * H + y), [H * W])), prepend=0).tolist()
    b, j = [a[0]], 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return np.array(b, np.uint32)


def polygon_mask_parity_numpy(xy, H, W):
    """bool [H, W]: pixel p = x * H + y is set when the number of toggles at positions <= p is odd -- what the sorted and merged
    counts decode to, without sorting."""
    x, y = polygon_crossings_numpy(xy, H, W)
    toggles = np.zeros(H * W + 1, np.int64)
    np.add.at(toggles, x * H + y, 1)
    return (np.cumsum(toggles[:-1]) & 1).astype(bool).reshape(W, H).T


def _decode(counts, H, W):
    c = np.asarray(counts, np.int64)
    return np.repeat(np.arange(len(c)) & 1, c).astype(bool).reshape(W, H).T


def _check_segs(who, segs, H, W):
    """-> [[float64 xy per polygon] per annotation]; an odd-length or empty coordinate list is refused by its indices."""
    H, W = int(H), int(W)
    _check_image(who, H, W)
    if H * W > MAX_PIXELS:
        raise ValueError("%s: image %d x %d has more than 2^30 pixels" % (who, H, W))
    segs = list(segs)
    if len(segs) > MAX_MASKS:
        raise ValueError("%s: %d annotations not in [0, %d]" % (who, len(segs), MAX_MASKS))
    out = []
    for i, polys in enumerate(segs):
        if isinstance(polys, dict) or isinstance(polys, (str, bytes)):
            raise ValueError("%s: segmentation %d is not a list of polygons" % (who, i))
        out.append([_vertices(p, "%s: polygon %d of segmentation %d" % (who, q, i)) for q, p in enumerate(polys)])
    return out, H, W


def masks_from_polygons_numpy(segs, H, W, classes=None, scores=None):
    """The rule as the plain sequential loops on the host: per annotation the OR of its polygons' masks, each decoded from
    polygon_counts_numpy as rle.masks_from_counts_numpy decodes counts; an annotation without polygons is empty.  -> PackedMasks
    with tight bounds (an empty mask gets (0, 0, -1, -1) and no rows).  Raises ValueError where mnc_mask_from_polygons returns
    MNC_ERR_INVALID."""
    segs, H, W = _check_segs("masks_from_polygons_numpy", segs, H, W)
    run_ptr, runs = np.zeros(len(segs) + 1, np.int64), []
    for i, polys in enumerate(segs):
        m = np.zeros((H, W), bool)
        for xy in polys:
            m |= _decode(polygon_counts_numpy(xy, H, W), H, W)
        t = np.flatnonzero(np.diff(m.reshape(-1, order="F").astype(np.int8), prepend=np.int8(0)))
        runs.append(np.diff(np.concatenate(([0], t, [H * W]))).astype(np.uint32))
        run_ptr[i + 1] = run_ptr[i] + len(runs[-1])
    return masks_from_counts_numpy(run_ptr, np.concatenate(runs) if runs else np.zeros(0, np.uint32), H, W, classes, scores)


def _flatten(segs):
    """[[xy per polygon] per annotation] -> (xy float64, vert_ptr int64 [polygons + 1], poly_ptr int64 [n + 1])."""
    poly_ptr = np.zeros(len(segs) + 1, np.int64)
    poly_ptr[1:] = np.cumsum([len(p) for p in segs])
    flat = [xy for polys in segs for xy in polys]
    vert_ptr = np.zeros(len(flat) + 1, np.int64)
    vert_ptr[1:] = np.cumsum([len(xy) // 2 for xy in flat])
    return (np.ascontiguousarray(np.concatenate(flat)) if flat else np.zeros(2, np.float64)), vert_ptr, poly_ptr


def masks_from_polygons_call(xy, vert_ptr, poly_ptr, H, W, bits=None, device_id=0):
    """mnc_mask_from_polygons as it is: bits None asks for bounds, offsets, areas and the size only.  -> (bounds, offsets, areas,
    bytes needed)."""
    n = len(poly_ptr) - 1
    bounds, offsets, areas = np.zeros((n, 4), np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    need = ctypes.c_size_t(0)
    _lib.call("mnc_mask_from_polygons", _lib.ptr(xy), _lib.ptr(vert_ptr), _lib.ptr(poly_ptr), n, int(H), int(W), _lib.ptr(bounds),
              _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits), bits.nbytes if bits is not None else 0, ctypes.addressof(need),
              int(device_id))
    return bounds, offsets, areas, int(need.value)


def masks_from_polygons(segs, H, W, classes=None, scores=None, device_id=None):
    """masks_from_polygons_numpy on the GPU (mnc_mask_from_polygons, csrc/mask_poly.hip): the same PackedMasks field by field.
    As rle.masks_from_counts: a sizes-only call, then the call with room, both in the device's host-entry workspace."""
    segs, H, W = _check_segs("masks_from_polygons", segs, H, W)
    device_id = _device_id(device_id)
    xy, vert_ptr, poly_ptr = _flatten(segs)
    bounds, offsets, areas, bits = sized_then_filled(
        lambda bits: masks_from_polygons_call(xy, vert_ptr, poly_ptr, H, W, bits, device_id))
    return PackedMasks(bounds, offsets, areas, classes, scores, bits)


def _is_rle(seg):
    return isinstance(seg, dict) and "counts" in seg and "size" in seg


def masks_from_segmentations(segs, H, W, classes=None, scores=None, device_id=None, cpu=False):
    """COCO `segmentation` entries of one H x W image, each a polygon list, a compressed RLE dict or an uncompressed RLE dict
    -> PackedMasks in the entries' order.  One device call per kind (mnc_mask_from_polygons, mnc_mask_from_rle), merged on the
    host; cpu=True takes the numpy statements of both instead.  An RLE of another size than H x W is refused by its index."""
    segs = list(segs)
    H, W = int(H), int(W)
    kinds = [1 if _is_rle(s) else 0 for s in segs]
    for i, s in enumerate(segs):
        if kinds[i] and (int(s["size"][0]), int(s["size"][1])) != (H, W):
            raise ValueError("masks_from_segmentations: segmentation %d is of size %s, not %s" % (i, list(s["size"]), [H, W]))
    polys, rles = [s for s, k in zip(segs, kinds) if not k], [s for s, k in zip(segs, kinds) if k]
    try:
        if cpu:
            a = masks_from_polygons_numpy(polys, H, W)
        else:
            a = masks_from_polygons(polys, H, W, device_id=device_id)
    except ValueError as e:
        raise ValueError("%s (the polygon segmentations are entries %s)" % (e, [i for i, k in enumerate(kinds) if not k]))
    run_ptr, runs, _, _ = counts_of_rles(rles)
    b = masks_from_counts_numpy(run_ptr, runs, H, W) if cpu else masks_from_counts(run_ptr, runs, H, W, device_id=device_id)
    at = [0, 0]
    order = []
    for k in kinds:
        order.append((k, at[k]))
        at[k] += 1
    bounds, offsets, areas, bits = merge_sets((a, b), order)
    return PackedMasks(bounds, offsets, areas, classes, scores, bits)
