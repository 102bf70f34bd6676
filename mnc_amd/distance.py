"""The squared Euclidean distance transform of packed instance masks, the largest inscribed disc, and erosion, dilation, opening
and closing by a disc (include/mnc_hip.h n15, csrc/mask_distance.hip) on mnc_amd.masks.PackedMasks.

    radius_sq(radius)                          floor(radius * radius): the R2 of a disc given by its radius
    distance_numpy(pm)                         -> DistanceMaps(dist_ptr, sq): the CPU statement of the inside distance
    inscribed_numpy(pm)                        -> (xy int32 [n, 2], r2 int32 [n]): the deepest pixel of every instance
    morph_numpy(pm, op, r2, H=None, W=None)    -> PackedMasks: op "erode", "dilate", "open" or "close" (or 0 .. 3) by the disc
    distance / inscribed / morph               the same through mnc_mask_distance / _inscribed / _morph (the GPU);
                                               PackedMasks.distance / .inscribed / .erode / .dilate / .open / .close are the methods

The rules.  All arithmetic is integer and frame-free: a mask M is a set of lattice pixels that is empty outside its bounds (padding
bits of the input are not trusted); the image size enters only as an optional final clip of dilate.

    inside distance   D(p) = min |p - q|^2 over all pixels q not in M -- pixels beyond the bounds are not in M -- for p in M, and
                      D(p) = 0 for p not in M: scipy.ndimage.distance_transform_edt of the mask padded by a one-pixel frame of
                      zeros, squared.  Instance i has h * w values, row-major with row stride w, uint32, from dist_ptr[i] on.
    inscribed disc    the pixel of maximal D, the lowest (y, x) on ties, in image coordinates, and that D; (-1, -1) and 0 for an
                      instance without rows or without a set pixel.
    the disc          of squared radius R2 >= 0 is {(dx, dy): dx^2 + dy^2 <= R2}; rho = isqrt(R2).
    erode             p is kept iff D(p) > R2.
    dilate            p is set iff some pixel of M lies within R2: the same transform on the complement, in the bounds grown by rho
                      on every side (beyond which nothing can be set).
    open, close       dilate(erode) and erode(dilate), the erosion of close taken in the unclipped grown frame: clipping to the
                      image first would eat into an object that touches the image edge.  Neither leaves the input's bounds.

The result of a morphology has the layout boundary() gives: offsets are multiples of 8, in order, without gaps; areas are the true
bit counts; padding bits are 0; classes and scores are carried over.  erode, open and close keep the input's bounds (an instance
without rows keeps them and gets no rows); dilate has (x1 - rho, y1 - rho, x2 + rho, y2 + rho), not tightened, with H, W
intersected with the image by boundary.clipped_bounds' rule, (0, 0, -1, -1) where nothing is left or the instance had no rows
(without H, W an instance without rows keeps its bounds).  There is no fallback: without the library or a GPU the device functions
raise.  They read host arrays: a device-resident PackedMasks (engine results) is fetched to the host first."""
import collections
import ctypes
import math

import numpy as np

from . import _lib
from .boundary import clipped_bounds
from .masks import MAX_AREA, MAX_COORD, MAX_SIDE, PackedMasks, _device_id, _set_args, sized_then_filled

MAX_N = 2048
MAX_R2 = 1024 * 1024
MAX_PIXELS = 2 ** 27
OPS = ("erode", "dilate", "open", "close")
_FAR = 2 ** 20                                  # a row distance no mask reaches; its square fits int64 with room to add


class DistanceMaps(collections.namedtuple("DistanceMaps", "dist_ptr sq shapes", defaults=(None,))):
    """dist_ptr int64 [n + 1], sq uint32 [dist_ptr[n]]: the squared inside distances of every instance, row-major; shapes int32
    [n, 2] the (h, w) of the instances (0 x 0 for one without rows), which map() needs."""
    __slots__ = ()

    def map(self, i):
        """uint32 [h, w]: the map of instance i."""
        return self.sq[int(self.dist_ptr[i]):int(self.dist_ptr[i + 1])].reshape(tuple(int(v) for v in self.shapes[i]))


def _shapes(pm):
    """int32 [n, 2]: (h, w) per instance, (0, 0) for one without rows."""
    s = np.array([pm.size(i) for i in range(len(pm))], np.int32).reshape(len(pm), 2)
    s[(s == 0).any(axis=1)] = 0
    return s


def radius_sq(radius):
    """R2 = floor(radius * radius) of a disc given by a radius >= 0.  The product is taken in doubles, so a radius that is
    itself a rounded root may land one below: sqrt(3) ** 2 < 3 in doubles, and radius_sq(math.sqrt(3)) is 2.  Every surface also
    takes an exact r2=."""
    radius = float(radius)
    if not radius >= 0.0 or math.isinf(radius):
        raise ValueError("radius_sq: radius=%r is not a finite number >= 0" % radius)
    return int(math.floor(radius * radius))


def _r2(who, radius, r2):
    if (radius is None) == (r2 is None):
        raise ValueError("%s: give exactly one of radius and r2" % who)
    r2 = radius_sq(radius) if r2 is None else int(r2)
    if not 0 <= r2 <= MAX_R2:
        raise ValueError("%s: r2=%d not in [0, %d]" % (who, r2, MAX_R2))
    return r2


def _op(who, op):
    if isinstance(op, str):
        if op not in OPS:
            raise ValueError("%s: op=%r is not one of %s" % (who, op, ", ".join(OPS)))
        return OPS.index(op)
    op = int(op)
    if not 0 <= op <= 3:
        raise ValueError("%s: op=%d not in [0, 3]" % (who, op))
    return op


def _image(who, H, W):
    """-> (H, W) with (0, 0) for no clip."""
    if H is None and W is None:
        return 0, 0
    if H is None or W is None:
        raise ValueError("%s: H and W go together" % who)
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("%s: image %d x %d not in [1, %d]" % (who, H, W, MAX_SIDE))
    return H, W


def _check_set(who, pm, grow=0):
    """What the library refuses about the set beyond HostMaskSet::check: the count, and the pixels of the rows, on the bounds
    grown by `grow` (dilate and close)."""
    n = len(pm)
    if n > MAX_N:
        raise ValueError("%s: n=%d not in [0, %d]" % (who, n, MAX_N))
    pixels = 0
    for i in range(n):
        h, w = pm.size(i)
        if h == 0 or w == 0:
            continue
        x1, y1, x2, y2 = (int(v) for v in pm.bounds[i])
        if grow and not (x1 - grow > -MAX_COORD and y1 - grow > -MAX_COORD and x2 + grow < MAX_COORD and y2 + grow < MAX_COORD):
            raise ValueError("%s: masks[%d] grown by %d leaves the coordinate range" % (who, i, grow))
        p = (h + 2 * grow) * (w + 2 * grow)
        if p > MAX_AREA:
            raise ValueError("%s: masks[%d] grown by %d covers %d pixels (limit %d)" % (who, i, grow, p, MAX_AREA))
        pixels += p
    if pixels > MAX_PIXELS:
        raise ValueError("%s: %d pixels of rows in the call (limit %d)" % (who, pixels, MAX_PIXELS))


# ---- the statements ----

def _row_gap(t):
    """bool [h, w] -> int64 [h, w]: per pixel the distance along its row to the nearest False (0 on one), _FAR where the row has
    none."""
    h, w = t.shape
    x = np.arange(w, dtype=np.int64)[None, :]
    before = np.maximum.accumulate(np.where(t, -_FAR, x), axis=1)                    # the column of the last False at or before
    after = np.minimum.accumulate(np.where(t, 2 * _FAR, x)[:, ::-1], axis=1)[:, ::-1]  # of the first False at or after
    return np.minimum(np.minimum(x - before, after - x), _FAR)


def sqdist_numpy(t, reach=None):
    """bool [h, w] -> int64 [h, w]: min over the False pixels q OF THE ARRAY of |p - q|^2 (nothing beyond the array counts; at
    least _FAR^2 where there is none).  g^2 of the row itself, then of the rows dy above and below plus dy^2, while dy^2 is below
    the largest value left.  reach: dy stops there -- the values below (reach + 1)^2 are exact, the others are not below it."""
    t = np.asarray(t, bool)
    g2 = _row_gap(t) ** 2
    best = g2.copy()
    dy = 1
    while dy < t.shape[0] and (reach is None or dy <= reach) and dy * dy < int(best.max()):
        np.minimum(best[:-dy], g2[dy:] + dy * dy, out=best[:-dy])
        np.minimum(best[dy:], g2[:-dy] + dy * dy, out=best[dy:])
        dy += 1
    return best


def inside_numpy(m, reach=None):
    """bool [h, w] -> int64 [h, w]: the inside distance D of one dense mask, everything beyond the array counting as unset."""
    return sqdist_numpy(np.pad(np.asarray(m, bool), 1), reach)[1:-1, 1:-1] if m.size else np.zeros(m.shape, np.int64)


def erode_numpy(m, r2):
    """bool [h, w] -> the pixels with D > r2."""
    return inside_numpy(m, math.isqrt(r2)) > r2


def dilate_numpy(m, r2):
    """bool [h, w] -> bool [h + 2 rho, w + 2 rho]: the pixels of the grown frame within r2 of a set pixel."""
    rho = math.isqrt(r2)
    t = np.ones((m.shape[0] + 2 * rho, m.shape[1] + 2 * rho), bool)
    t[rho:rho + m.shape[0], rho:rho + m.shape[1]] = ~np.asarray(m, bool)
    return sqdist_numpy(t, rho) <= r2


def open_numpy(m, r2):
    rho = math.isqrt(r2)
    return dilate_numpy(erode_numpy(m, r2), r2)[rho:rho + m.shape[0], rho:rho + m.shape[1]]


def close_numpy(m, r2):
    rho = math.isqrt(r2)
    return erode_numpy(dilate_numpy(m, r2), r2)[rho:rho + m.shape[0], rho:rho + m.shape[1]]


def distance_numpy(pm):
    """The inside distances as a plain loop on the host -- the specification csrc/mask_distance.hip is tested against.  ->
    DistanceMaps.  Raises ValueError where mnc_mask_distance returns MNC_ERR_INVALID for the count or the pixels."""
    _check_set("distance_numpy", pm)
    n = len(pm)
    dist_ptr, parts = np.zeros(n + 1, np.int64), []
    for i in range(n):
        h, w = pm.size(i)
        if h and w:
            parts.append(inside_numpy(pm.dense(i)).reshape(-1).astype(np.uint32))
            dist_ptr[i + 1] = h * w
    np.cumsum(dist_ptr, out=dist_ptr)
    return DistanceMaps(dist_ptr, np.concatenate(parts) if parts else np.zeros(0, np.uint32), _shapes(pm))


def inscribed_numpy(pm):
    """The inscribed discs as a plain loop on the host -> (xy int32 [n, 2], r2 int32 [n])."""
    _check_set("inscribed_numpy", pm)
    n = len(pm)
    xy, r2 = np.full((n, 2), -1, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        h, w = pm.size(i)
        if not (h and w):
            continue
        d = inside_numpy(pm.dense(i)).reshape(-1)
        at = int(np.argmax(d))                                    # the first of the largest: the lowest (y, x)
        if d[at] > 0:
            xy[i] = (int(pm.bounds[i][0]) + at % w, int(pm.bounds[i][1]) + at // w)
            r2[i] = d[at]
    return xy, r2


def morph_numpy(pm, op, r2, H=None, W=None):
    """The morphology as a plain loop on the host -> PackedMasks.  Raises ValueError where mnc_mask_morph returns MNC_ERR_INVALID
    for op, r2, H, W, the count or the pixels."""
    who = "morph_numpy"
    op, r2 = _op(who, op), _r2(who, None, r2)
    H, W = _image(who, H, W)
    rho = math.isqrt(r2)
    _check_set(who, pm, rho if op in (1, 3) else 0)
    n = len(pm)
    bounds, dense = np.array(pm.bounds, np.int32).reshape(n, 4), [None] * n
    for i in range(n):
        h, w = pm.size(i)
        if not (h and w):
            if op == 1 and H:
                bounds[i] = (0, 0, -1, -1)
            continue
        m = pm.dense(i)
        if op != 1:
            dense[i] = (erode_numpy, None, open_numpy, close_numpy)[op](m, r2)
            continue
        x1, y1 = int(bounds[i][0]) - rho, int(bounds[i][1]) - rho
        grown = np.array([[x1, y1, int(bounds[i][2]) + rho, int(bounds[i][3]) + rho]])
        bounds[i] = clipped_bounds(grown, H, W)[0] if H else grown[0]
        bx1, by1, bx2, by2 = (int(v) for v in bounds[i])
        if bx2 >= bx1 and by2 >= by1:
            dense[i] = dilate_numpy(m, r2)[by1 - y1:by2 - y1 + 1, bx1 - x1:bx2 - x1 + 1]
    return PackedMasks.from_dense(bounds, dense, pm.classes, pm.scores)


# ---- the device ----

def distance_call(pm, sq=None, device_id=0):
    """mnc_mask_distance as it is: sq None asks for dist_ptr and the total only (nothing is launched).  -> (dist_ptr, total)."""
    dist_ptr, total = np.zeros(len(pm) + 1, np.int64), ctypes.c_size_t(0)
    _lib.call("mnc_mask_distance", *(_set_args(pm, areas=False) + (
        _lib.ptr(dist_ptr), _lib.ptr(sq), sq.size if sq is not None else 0, ctypes.addressof(total), int(device_id))))
    return dist_ptr, int(total.value)


def distance(pm, device_id=None):
    """distance_numpy on the GPU (mnc_mask_distance): the same DistanceMaps field by field, four bytes a pixel copied back.  A
    sizes-only call, then the call with room.  Invalid sets raise _lib.MncError (MNC_ERR_INVALID) before anything is launched.  A
    device-resident PackedMasks is fetched to the host first."""
    pm = pm.fetch()
    dev = _device_id(device_id)
    total = distance_call(pm, None, dev)[1]
    sq = np.zeros(total, np.uint32)
    dist_ptr, _ = distance_call(pm, sq if total else np.zeros(1, np.uint32), dev)
    return DistanceMaps(dist_ptr, sq, _shapes(pm))


def inscribed(pm, device_id=None):
    """inscribed_numpy on the GPU (mnc_mask_inscribed): three numbers per instance come back."""
    pm = pm.fetch()
    n = len(pm)
    xy, r2 = np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
    _lib.call("mnc_mask_inscribed", *(_set_args(pm, areas=False) + (
        _lib.ptr(xy if n else np.zeros(2, np.int32)), _lib.ptr(r2 if n else np.zeros(1, np.int32)), _device_id(device_id))))
    return xy, r2


def morph_call(pm, op, r2, H=0, W=0, bits=None, device_id=0):
    """mnc_mask_morph as it is: bits None asks for bounds, offsets and the size only (nothing is launched).  -> (bounds, offsets,
    areas, bytes needed)."""
    n = len(pm)
    bounds, offsets, areas = np.zeros((n, 4), np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    need = ctypes.c_size_t(0)
    _lib.call("mnc_mask_morph", *(_set_args(pm, areas=False) + (
        int(op), int(r2), int(H), int(W), _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits),
        bits.nbytes if bits is not None else 0, ctypes.addressof(need), int(device_id))))
    return bounds, offsets, areas, int(need.value)


def morph(pm, op, radius=None, r2=None, H=None, W=None, device_id=None):
    """morph_numpy on the GPU (mnc_mask_morph): the same PackedMasks field by field.  The disc is given by radius (radius_sq) or by
    an exact r2.  Invalid arguments raise ValueError, invalid sets _lib.MncError (MNC_ERR_INVALID), before anything is launched.  A
    device-resident PackedMasks is fetched to the host first."""
    op, r2 = _op("morph", op), _r2("morph", radius, r2)
    H, W = _image("morph", H, W)
    pm = pm.fetch()
    dev = _device_id(device_id)
    bounds, offsets, areas, bits = sized_then_filled(lambda bits: morph_call(pm, op, r2, H, W, bits, dev))
    return PackedMasks(bounds, offsets, areas, pm.classes, pm.scores, bits)


def timing(on):
    """mnc_mask_distance_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_distance_timing", on)
