"""Surface distances between packed instance masks: the surfaces, and for pairs of instances of two sets the squared distances
from the surface pixels of the one to the surface of the other -- the Hausdorff distance, its 95th percentile (HD95), the average
symmetric surface distance (ASSD), the boundary F-measure (the F of DAVIS's J&F) and the normalised surface Dice (include/mnc_hip.h
n22, csrc/mask_surface.hip) on mnc_amd.masks.PackedMasks.

    surface_numpy(pm)                                        -> PackedMasks: the CPU statement of the surfaces
    surface_stats_numpy(a, b, pairs=None, tau2=())           -> SurfaceStats: the CPU statement of the reduced distances
    surface_distances_numpy(a, b, pairs=None)                -> SurfaceDistances: the CPU statement of the distances themselves
    surface / surface_stats / surface_distances              the same through mnc_mask_surface / _surface_stats / _surface_dist
                                                             (the GPU); PackedMasks.surface / .surface_stats / .surface_distances
                                                             are the methods
    tolerance_sq(H, W, ratio=0.008)                          DAVIS's boundary tolerance of an H x W image as a squared radius

The rules.  Everything is integer and frame-free, by the conventions of mnc_amd/distance.py and mnc_amd/algebra.py: a mask is a set
of lattice pixels that is empty outside its bounds, bounds may be negative or unclipped, padding bits of the input are not trusted.

    surface     S(M) = the pixels of M that have at least one of their four edge neighbours outside M = M & ~erode(M, r2=1).  The
                result of surface() is a PackedMasks in the input's frames: the input's bounds (an instance without rows keeps them
                and gets no rows), offsets in order without gaps, areas the surface pixel counts, padding bits 0, classes and
                scores carried over.
    pairs       int32 [P, 2] of (i, j), instance i of a against instance j of b, in any order, repeats allowed; None: all
                len(a) x len(b) pairs in row-major order, as overlaps() orders them.
    direction   0 is a[i] -> b[j], 1 is b[j] -> a[i]; every field of a result is shaped [P, 2] over the two.
    distances   d2(p) = min over q in S(dst) of |p - q|^2 for every p in S(src), in image coordinates, an integer.
    stats       count = |S(src)|; max_d2 the greatest d2; argmax the (x, y) of the source pixel that attains it, the lowest (y, x)
                on ties; sum_d2 the sum; within[.., t] the source pixels with d2 <= tau2[t], for up to 8 squared tolerances.  Where
                S(src) or S(dst) is empty: max_d2 -1, argmax (-1, -1), sum_d2 0, within 0, and count stays true.
    raw         ptr int64 [2 P + 1], d2 uint32 [ptr[-1]]: pair k in direction d owns ptr[2 k + d] .. ptr[2 k + d + 1] - 1, the d2
                of its source surface pixels in raster (y, x) order; 0xffffffff throughout where the destination surface is empty.

Every number the device gives is an integer; the floats (roots, ratios, percentiles) are made on the host by the methods of the
result classes, so the numpy path and the device path share them.

Refused with ValueError, by the statements and the device functions alike (the library says MNC_ERR_INVALID, before a launch and
with nothing written): more than 2048 instances in a set, a coordinate with |c| >= 2^24, more than 2^26 pixels in one bound; more
than 65536 pairs; a pair index out of range; more than 8 tolerances or one outside [0, 2^31); a hull of the bounds of all instances
with rows of both sets that spans 32768 pixels or more in either axis -- below it every d2 < 2^31 and every sum fits int64; more
than 2^27 pixels of rows in the call; more than 2^28 raw distances.  There is no fallback: without the library or a GPU the device
functions raise.  They read host arrays: a device-resident PackedMasks (engine results) is fetched to the host first."""
import collections
import ctypes
import math

import numpy as np

from . import _lib
from .distance import radius_sq
from .masks import MAX_AREA, MAX_COORD, PackedMasks, _device_id, _set_args, sized_then_filled

MAX_N = 2048
MAX_PAIRS = 65536
MAX_TAU = 8
MAX_SPAN = 32768
MAX_PIXELS = 2 ** 27
MAX_ENTRIES = 2 ** 28
NONE = 0xffffffff                               # the raw distance to an empty surface
_CHUNK = 2 ** 22                                # point pairs of one step of the statement's brute force


def tolerance_sq(H, W, ratio=0.008):
    """DAVIS's boundary tolerance as a squared integer radius: the radius is ratio itself when ratio >= 1, else ceil(ratio *
    sqrt(H^2 + W^2)) pixels (0.008 of the diagonal: 8 at 480 x 854), squared as distance.radius_sq squares.  A surface pixel
    within it of the other surface -- d2 <= tolerance_sq -- is one that DAVIS's dilation by disk(radius) reaches."""
    H, W, ratio = int(H), int(W), float(ratio)
    if H < 1 or W < 1 or not ratio >= 0.0 or math.isinf(ratio):
        raise ValueError("tolerance_sq: H=%d, W=%d, ratio=%r" % (H, W, ratio))
    return radius_sq(ratio if ratio >= 1.0 else math.ceil(ratio * math.sqrt(H * H + W * W)))


def _ratio(num, den, empty):
    out = np.full(np.shape(num), float(empty))
    np.divide(num, den, out=out, where=np.asarray(den) > 0)
    return out


class SurfaceStats(collections.namedtuple("SurfaceStats", "count max_d2 argmax sum_d2 within tau2")):
    """count, max_d2, sum_d2 int64 [P, 2]; argmax int32 [P, 2, 2] = (x, y); within int64 [P, 2, T]; tau2 the T squared tolerances.
    Direction 0 measures a's surface against b's, direction 1 b's against a's."""
    __slots__ = ()

    def _t(self, t):
        t = int(t)
        if not 0 <= t < len(self.tau2):
            raise ValueError("tolerance %d not in [0, %d)" % (t, len(self.tau2)))
        return t

    def hausdorff(self):
        """float64 [P]: sqrt of the greater max_d2 of the two directions; inf where exactly one surface is empty, nan where both
        are."""
        out = np.sqrt(np.maximum(self.max_d2[:, 0], self.max_d2[:, 1]).astype(np.float64), where=(self.count > 0).all(1),
                      out=np.full(len(self.count), np.inf))
        out[(self.count == 0).all(1)] = np.nan
        return out

    def precision(self, t=0):
        """float64 [P]: the share of a's surface pixels within tolerance t of b's surface (a the result, b the truth).  DAVIS's
        convention for empty sides: a empty gives 1; a not empty and b empty gives 0."""
        t = self._t(t)
        return _ratio(self.within[:, 0, t], self.count[:, 0], 1.0)

    def recall(self, t=0):
        """float64 [P]: the share of b's surface pixels within tolerance t of a's surface.  DAVIS's convention for empty sides: b
        empty gives 1; b not empty and a empty gives 0."""
        t = self._t(t)
        return _ratio(self.within[:, 1, t], self.count[:, 1], 1.0)

    def boundary_f(self, t=0):
        """float64 [P]: 2 P R / (P + R) of precision(t) and recall(t), 0 where P + R == 0 -- the F of DAVIS's J&F (f_measure of
        davis2017-evaluation) at the squared tolerance tau2[t], with its convention for empty sides: both surfaces empty give P =
        R = 1 and F = 1; exactly one empty gives P or R = 0 and F = 0."""
        p, r = self.precision(t), self.recall(t)
        return _ratio(2.0 * p * r, p + r, 0.0)

    def nsd(self, t=0):
        """float64 [P]: the normalised surface Dice (within0 + within1) / (count0 + count1) at tolerance t; nan where both
        surfaces are empty."""
        t = self._t(t)
        return _ratio(self.within[:, :, t].sum(1), self.count.sum(1), np.nan)


class SurfaceDistances(collections.namedtuple("SurfaceDistances", "ptr d2")):
    """ptr int64 [2 P + 1], d2 uint32 [ptr[-1]]: slot 2 k + d holds the squared distances of pair k in direction d."""
    __slots__ = ()

    def __len__(self):
        return (len(self.ptr) - 1) // 2

    def slot(self, k, d):
        """uint32: the squared distances of pair k in direction d, in raster order of the source's surface."""
        s = 2 * int(k) + int(d)
        return self.d2[int(self.ptr[s]):int(self.ptr[s + 1])]

    def _roots(self, k):
        """float64: the distances of both directions of pair k, one after the other; inf where the other surface is empty."""
        v = self.d2[int(self.ptr[2 * k]):int(self.ptr[2 * k + 2])]
        return np.where(v == NONE, np.inf, np.sqrt(v.astype(np.float64)))

    def percentile(self, q):
        """float64 [P]: np.percentile(q) over the distances of both directions together (MedPy's hd95 at q = 95); nan for a pair
        without a surface pixel, inf where exactly one surface is empty."""
        out = np.full(len(self), np.nan)
        for k in range(len(self)):
            r = self._roots(k)
            if r.size:
                out[k] = np.inf if np.isinf(r).any() else np.percentile(r, q)
        return out

    def hd95(self):
        return self.percentile(95)

    def assd(self):
        """float64 [P]: the average symmetric surface distance, the mean of the distances of both directions together -- (sum over
        S(a) + sum over S(b)) / (|S(a)| + |S(b)|), summed with math.fsum.  (MedPy's assd averages the two directed means instead,
        which weighs the smaller surface more.)  nan and inf as percentile gives them."""
        out = np.full(len(self), np.nan)
        for k in range(len(self)):
            r = self._roots(k)
            if r.size:
                out[k] = np.inf if np.isinf(r).any() else math.fsum(r) / r.size
        return out


def _check_sets(who, sets):
    """What the library refuses about the sets: mnc_mask_boundary's limits, the hull and the pixels of the rows."""
    hull, pixels = [None] * 4, 0
    for name, pm in sets:
        n = len(pm)
        if n > MAX_N:
            raise ValueError("%s: %d instances in set %s (limit %d)" % (who, n, name, MAX_N))
        for i in range(n):
            x1, y1, x2, y2 = (int(v) for v in pm.bounds[i])
            if not all(-MAX_COORD < v < MAX_COORD for v in (x1, y1, x2, y2)):
                raise ValueError("%s: %s[%d] coordinate out of range" % (who, name, i))
            h, w = pm.size(i)
            if h == 0 or w == 0:
                continue
            if h * w > MAX_AREA:
                raise ValueError("%s: %s[%d] covers %d pixels (limit %d)" % (who, name, i, h * w, MAX_AREA))
            pixels += h * w
            hull = [x1, y1, x2, y2] if hull[0] is None else [min(hull[0], x1), min(hull[1], y1), max(hull[2], x2), max(hull[3], y2)]
    if hull[0] is not None and (hull[2] - hull[0] + 1 >= MAX_SPAN or hull[3] - hull[1] + 1 >= MAX_SPAN):
        raise ValueError("%s: the bounds span %d x %d pixels (limit %d a side)"
                         % (who, hull[2] - hull[0] + 1, hull[3] - hull[1] + 1, MAX_SPAN - 1))
    if pixels > MAX_PIXELS:
        raise ValueError("%s: %d pixels of rows in the call (limit %d)" % (who, pixels, MAX_PIXELS))


def _check_pairs(who, a, b, pairs):
    """-> int32 [P, 2], C-contiguous."""
    n, m = len(a), len(b)
    if pairs is None:
        if n * m > MAX_PAIRS:
            raise ValueError("%s: %d x %d pairs (limit %d)" % (who, n, m, MAX_PAIRS))
        return np.ascontiguousarray(np.stack(np.divmod(np.arange(n * m, dtype=np.int32), np.int32(max(m, 1))), axis=1), np.int32)
    pairs = np.asarray(pairs)
    if pairs.size == 0:
        return np.zeros((0, 2), np.int32)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError("%s: pairs is not an integer array [P, 2] (shape %s, dtype %s)" % (who, pairs.shape, pairs.dtype))
    if len(pairs) > MAX_PAIRS:
        raise ValueError("%s: %d pairs (limit %d)" % (who, len(pairs), MAX_PAIRS))
    if pairs.min() < 0 or pairs[:, 0].max() >= n or pairs[:, 1].max() >= m:
        raise ValueError("%s: a pair index not in [0, %d) x [0, %d)" % (who, n, m))
    return np.ascontiguousarray(pairs, np.int32)


def _check_tau(who, tau2):
    tau = [int(t) for t in np.asarray(tau2).reshape(-1)]
    if len(tau) > MAX_TAU:
        raise ValueError("%s: %d tolerances (limit %d)" % (who, len(tau), MAX_TAU))
    if any(not 0 <= t < 2 ** 31 for t in tau):
        raise ValueError("%s: a tau2 not in [0, 2^31)" % who)
    return np.array(tau, np.int32)


# ---- the statements ----

def surface_of(m):
    """bool [h, w] -> bool [h, w]: the pixels with an edge neighbour outside the mask, everything beyond the array counting as
    outside."""
    m = np.asarray(m, bool)
    p = np.pad(m, 1)
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def surface_numpy(pm):
    """The surfaces as a plain loop on the host -- the specification csrc/mask_surface.hip is tested against.  -> PackedMasks."""
    _check_sets("surface_numpy", [("masks", pm)])
    dense = [surface_of(pm.dense(i)) if min(pm.size(i)) else None for i in range(len(pm))]
    return PackedMasks.from_dense(np.array(pm.bounds, np.int32).reshape(len(pm), 4), dense, pm.classes, pm.scores)


def surface_points(pm, i):
    """-> (x, y) int64: the surface pixels of instance i in image coordinates, in raster (y, x) order."""
    if not min(pm.size(i)):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    y, x = np.nonzero(surface_of(pm.dense(i)))
    return x.astype(np.int64) + int(pm.bounds[i][0]), y.astype(np.int64) + int(pm.bounds[i][1])


def nearest_sq(src, dst):
    """(x, y) of the sources, (x, y) of the destinations (at least one) -> int64: per source the least squared distance, by brute
    force over all point pairs, a chunk of sources at a time."""
    (sx, sy), (dx, dy) = src, dst
    out = np.zeros(len(sx), np.int64)
    step = max(_CHUNK // len(dx), 1)
    for k in range(0, len(sx), step):
        out[k:k + step] = ((sx[k:k + step, None] - dx[None, :]) ** 2 + (sy[k:k + step, None] - dy[None, :]) ** 2).min(axis=1)
    return out


def _slots(who, a, b, pairs, entries=None):
    """The checked call -> (pairs, for every slot (source points, the d2 of them or None where the destination is empty)).
    entries: the most source points of all slots together, looked at before any distance is made."""
    _check_sets(who, [("a", a), ("b", b)])
    pairs = _check_pairs(who, a, b, pairs)
    pa = {i: surface_points(a, i) for i in set(pairs[:, 0].tolist())}
    pb = {j: surface_points(b, j) for j in set(pairs[:, 1].tolist())}
    total = sum(len(pa[i][0]) + len(pb[j][0]) for i, j in pairs.tolist())
    if entries is not None and total > entries:
        raise ValueError("%s: %d distances (limit %d)" % (who, total, entries))
    out = []
    for i, j in pairs.tolist():
        for src, dst in ((pa[i], pb[j]), (pb[j], pa[i])):
            out.append((src, nearest_sq(src, dst) if len(dst[0]) else None))
    return pairs, out


def surface_stats_numpy(a, b, pairs=None, tau2=()):
    """The reduced distances as a plain loop on the host -- the specification csrc/mask_surface.hip is tested against.
    -> SurfaceStats."""
    who = "surface_stats_numpy"
    tau = _check_tau(who, tau2)
    pairs, slots = _slots(who, a, b, pairs)
    P, T = len(pairs), len(tau)
    count, top, total = np.zeros((P, 2), np.int64), np.full((P, 2), -1, np.int64), np.zeros((P, 2), np.int64)
    at, within = np.full((P, 2, 2), -1, np.int32), np.zeros((P, 2, T), np.int64)
    for s, ((x, y), d2) in enumerate(slots):
        k, d = divmod(s, 2)
        count[k, d] = len(x)
        if d2 is None or not len(x):
            continue
        first = int(np.argmax(d2))                                  # the first of the largest in raster order: the lowest (y, x)
        top[k, d], total[k, d], at[k, d] = d2[first], d2.sum(), (x[first], y[first])
        within[k, d] = [(d2 <= t).sum() for t in tau]
    return SurfaceStats(count, top, at, total, within, tau)


def surface_distances_numpy(a, b, pairs=None):
    """The distances themselves as a plain loop on the host -- the specification csrc/mask_surface.hip is tested against.
    -> SurfaceDistances."""
    pairs, slots = _slots("surface_distances_numpy", a, b, pairs, MAX_ENTRIES)
    ptr = np.zeros(2 * len(pairs) + 1, np.int64)
    parts = []
    for s, ((x, _), d2) in enumerate(slots):
        ptr[s + 1] = ptr[s] + len(x)
        parts.append(np.full(len(x), NONE, np.uint32) if d2 is None else d2.astype(np.uint32))
    return SurfaceDistances(ptr, np.concatenate(parts) if parts else np.zeros(0, np.uint32))


# ---- the device ----

def _call(name, *args):
    """An entry whose MNC_ERR_INVALID is this module's ValueError."""
    try:
        _lib.call(name, *args)
    except _lib.MncError as e:
        if e.code == 1:
            raise ValueError(str(e))
        raise


def surface_call(pm, bits=None, device_id=0):
    """mnc_mask_surface as it is: bits None asks for bounds, offsets and the size only (nothing is launched).  -> (bounds, offsets,
    areas, bytes needed)."""
    n = len(pm)
    bounds, offsets, areas = np.zeros((n, 4), np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    need = ctypes.c_size_t(0)
    _call("mnc_mask_surface", *(_set_args(pm, areas=False) + (
        _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits), bits.nbytes if bits is not None else 0,
        ctypes.addressof(need), int(device_id))))
    return bounds, offsets, areas, int(need.value)


def surface(pm, device_id=None):
    """surface_numpy on the GPU (mnc_mask_surface): the same PackedMasks field by field.  ValueError for what the statement
    refuses.  A device-resident PackedMasks is fetched first."""
    pm = pm.fetch()
    dev = _device_id(device_id)
    bounds, offsets, areas, bits = sized_then_filled(lambda bits: surface_call(pm, bits, dev))
    return PackedMasks(bounds, offsets, areas, pm.classes, pm.scores, bits)


def stats_call(a, b, pairs, tau, device_id=0):
    """mnc_mask_surface_stats as it is on checked arrays: pairs int32 [P, 2], tau int32 [T] -> SurfaceStats."""
    P, T = len(pairs), len(tau)
    count, top, total = (np.zeros((P, 2), np.int64) for _ in range(3))
    at, within = np.zeros((P, 2, 2), np.int32), np.zeros((P, 2, T), np.int64)
    _call("mnc_mask_surface_stats", *(_set_args(a, areas=False) + _set_args(b, areas=False) + (
        _lib.ptr(pairs) if P else None, P, _lib.ptr(tau) if T else None, T, _lib.ptr(count) if P else None,
        _lib.ptr(top) if P else None, _lib.ptr(at) if P else None, _lib.ptr(total) if P else None,
        _lib.ptr(within) if P and T else None, int(device_id))))
    return SurfaceStats(count, top, at, total, within, tau)


def surface_stats(a, b, pairs=None, tau2=(), device_id=None):
    """surface_stats_numpy on the GPU (mnc_mask_surface_stats): the same SurfaceStats field by field; both sets go up once and
    11 + T numbers per pair and direction come back.  ValueError for what the statement refuses.  Device-resident PackedMasks are
    fetched first."""
    a, b = a.fetch(), b.fetch()
    tau = _check_tau("surface_stats", tau2)
    return stats_call(a, b, _check_pairs("surface_stats", a, b, pairs), tau, _device_id(device_id))


def dist_call(a, b, pairs, d2=None, device_id=0):
    """mnc_mask_surface_dist as it is: d2 None asks for ptr and the total only.  -> (ptr, total)."""
    P = len(pairs)
    ptr, total = np.zeros(2 * P + 1, np.int64), ctypes.c_size_t(0)
    _call("mnc_mask_surface_dist", *(_set_args(a, areas=False) + _set_args(b, areas=False) + (
        _lib.ptr(pairs) if P else None, P, _lib.ptr(ptr), _lib.ptr(d2), d2.size if d2 is not None else 0,
        ctypes.addressof(total), int(device_id))))
    return ptr, int(total.value)


def surface_distances(a, b, pairs=None, device_id=None):
    """surface_distances_numpy on the GPU (mnc_mask_surface_dist): the same SurfaceDistances field by field, four bytes a surface
    pixel and pair copied back.  A sizes-only call, then the call with room.  ValueError for what the statement refuses.
    Device-resident PackedMasks are fetched first."""
    a, b = a.fetch(), b.fetch()
    pairs = _check_pairs("surface_distances", a, b, pairs)
    dev = _device_id(device_id)
    total = dist_call(a, b, pairs, None, dev)[1]
    d2 = np.zeros(total, np.uint32)
    ptr, _ = dist_call(a, b, pairs, d2 if total else np.zeros(1, np.uint32), dev)
    return SurfaceDistances(ptr, d2)


def timing(on):
    """mnc_mask_surface_timing: switch the event pairs on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_surface_timing", on)
