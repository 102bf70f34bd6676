"""Region descriptors of packed instance masks: the moments of order up to two, the convex hull, and from the hull the rectangle
of least area and the diameter (include/mnc_hip.h n16, csrc/mask_shape.hip) on mnc_amd.masks.PackedMasks.

    moments_numpy(pm)      -> Moments(m int64 [n, 6], origin int32 [n, 2]): the CPU statement of the sums
    hull_numpy(pm)         -> Hulls(vert_ptr int64 [n + 1], xy int32 [V, 2], area2 int64 [n])
    oriented_numpy(pm)     -> OrientedBoxes(box int64 [n, 8], diameter int64 [n, 3])
    moments / hull / oriented   the same through mnc_mask_moments / _hull / _oriented (the GPU); PackedMasks.moments / .hull /
                                .solidity / .oriented_boxes are the methods

The rules.  Every number the device gives is an integer; the floats (centroid, axes, corners, rbox) are made on the host from
those integers by the methods of the result classes, so the numpy path and the device path share them.

    moments    m_pq = sum of x^p y^q over the set pixels, x and y the pixel's column and row relative to the bound's (x1, y1),
               in the order (m00, m10, m01, m20, m11, m02).  Padding bits are not counted.  Within the limits every sum stays
               below 2^56.  An instance without a set pixel gives zeros.
    hull       the convex hull of the union of the closed unit squares [x, x + 1] x [y, y + 1] of the set pixels.  Vertices are
               lattice points in image coordinates, with contours()'s conventions: clockwise on screen (y down: the set lies on
               the right of every edge), from the smallest (y, x) vertex on, no three consecutive vertices collinear, the first
               not repeated.  area2 is twice the shoelace area.  The candidates are, per lattice row Y, the least first set
               column and the greatest (last set column + 1) over the pixel rows Y - 1 and Y; the statement is the monotone chain
               over them.  An instance without a set pixel has no vertices and area2 = 0.
    oriented   for every hull edge k with tail a and vector e = (ex, ey), over the hull vertices p: t = (p - a) . e and
               s = ex (p_y - a_y) - ey (p_x - a_x) (s >= 0, min s = 0).  The rectangle on that edge has the area
               (tmax - tmin) smax / |e|^2; the edge of least area wins, the lowest k on ties, fractions compared by
               cross-multiplication.  box = (k, ax, ay, ex, ey, tmin, tmax, smax), a in image coordinates.  The rectangle of
               least area of a convex polygon has a side on one of its edges (Freeman and Shapira 1975).
    diameter   (d2, i, j): the greatest squared distance between two hull vertices i < j, the lexicographically lowest pair on
               ties.  Zeros for an instance without a set pixel.

Refused with ValueError here, MNC_ERR_INVALID by the library, before anything is launched: everything mnc_mask_boundary refuses
about a set (n outside [0, 2048], |coordinate| >= 2^24, more than 2^26 pixels in one bound), and any bound wider or taller than
32768 -- which keeps the differences below 2^15 + 1 and every quantity above inside the width stated for it.  There is no
fallback: without the library or a GPU the device functions raise.  They read host arrays: a device-resident PackedMasks (engine
results) is fetched to the host first."""
import collections
import ctypes
import math

import numpy as np

from . import _lib
from .masks import MAX_AREA, MAX_COORD, _device_id, _set_args

MAX_N = 2048
MAX_EXTENT = 32768


def _origins(pm):
    return np.ascontiguousarray(np.asarray(pm.bounds, np.int32).reshape(len(pm), 4)[:, :2])


class Moments(collections.namedtuple("Moments", "m origin")):
    """m int64 [n, 6] = (m00, m10, m01, m20, m11, m02) relative to origin int32 [n, 2] = the bounds' (x1, y1)."""
    __slots__ = ()

    def centroid(self):
        """float64 [n, 2]: (x1 + m10 / m00, y1 + m01 / m00), image coordinates of pixel indices (the centre of pixel 0 is 0.0);
        NaN for an instance without a set pixel."""
        out = np.full((len(self.m), 2), np.nan)
        for i, (m00, m10, m01) in enumerate(self.m[:, :3].tolist()):
            if m00:
                out[i] = (int(self.origin[i][0]) + m10 / m00, int(self.origin[i][1]) + m01 / m00)
        return out

    def central(self):
        """float64 [n, 3]: (mu20, mu11, mu02), the second moments about the centroid: mu20 = (m00 m20 - m10^2) / m00, mu11 =
        (m00 m11 - m10 m01) / m00, mu02 = (m00 m02 - m01^2) / m00, the numerators in Python integers and one division each; NaN
        for an instance without a set pixel."""
        out = np.full((len(self.m), 3), np.nan)
        for i, (m00, m10, m01, m20, m11, m02) in enumerate(self.m.tolist()):
            if m00:
                out[i] = ((m00 * m20 - m10 * m10) / m00, (m00 * m11 - m10 * m01) / m00, (m00 * m02 - m01 * m01) / m00)
        return out

    def _eig(self):
        mu = self.central()
        with np.errstate(invalid="ignore", divide="ignore"):
            c = mu / self.m[:, :1].astype(np.float64)              # the covariance of the pixel centres
        a, b, d = c[:, 0], c[:, 1], c[:, 2]
        root = np.sqrt((a - d) ** 2 + 4.0 * b * b)
        return a, b, d, root

    def orientation(self):
        """float64 [n]: the angle of the major axis of the ellipse with the same second moments, theta = atan2(2 mu11,
        mu20 - mu02) / 2 in (-pi/2, pi/2], measured from +x towards +y (y points down: clockwise on screen); 0 where the
        ellipse is a circle; NaN for an instance without a set pixel."""
        a, b, d, _ = self._eig()
        return 0.5 * np.arctan2(2.0 * b, a - d)

    def axes(self):
        """float64 [n, 2]: the full lengths (major, minor) of that ellipse, 4 sqrt(lambda) of the eigenvalues lambda = ((a + d)
        +- sqrt((a - d)^2 + 4 b^2)) / 2 of the covariance (a, b, d) = (mu20, mu11, mu02) / m00 (a single pixel gives 0, 0; the
        area of a unit pixel is not added); NaN for an instance without a set pixel."""
        a, b, d, root = self._eig()
        return 4.0 * np.sqrt(np.stack([np.maximum((a + d + root) / 2.0, 0.0), np.maximum((a + d - root) / 2.0, 0.0)], axis=1))


class Hulls(collections.namedtuple("Hulls", "vert_ptr xy area2")):
    """vert_ptr int64 [n + 1], xy int32 [V, 2] (x, y), area2 int64 [n]: instance i has the vertices vert_ptr[i] ..
    vert_ptr[i + 1] - 1."""
    __slots__ = ()

    def vertices(self, i):
        return self.xy[int(self.vert_ptr[i]):int(self.vert_ptr[i + 1])]

    def polygon(self, i):
        """The flat COCO list [x0, y0, x1, y1, ...] of instance i's hull (floats); [] without a set pixel."""
        return [float(v) for v in self.vertices(i).reshape(-1)]

    def solidity(self, areas):
        """float64 [n]: 2 area / area2, the share of the hull the mask fills; 0 for an instance without a set pixel."""
        areas = np.asarray(areas, np.int64).reshape(len(self.area2))
        out = np.zeros(len(self.area2), np.float64)
        keep = self.area2 > 0
        out[keep] = 2.0 * areas[keep] / self.area2[keep]
        return out


class OrientedBoxes(collections.namedtuple("OrientedBoxes", "box diameter")):
    """box int64 [n, 8] = (k, ax, ay, ex, ey, tmin, tmax, smax), diameter int64 [n, 3] = (d2, i, j)."""
    __slots__ = ()

    def corners(self):
        """float64 [n, 4, 2]: the corners a + (t e + s (-ey, ex)) / |e|^2 at (t, s) = (tmin, 0), (tmax, 0), (tmax, smax),
        (tmin, smax) -- clockwise on screen, the first two on the line of the chosen hull edge; NaN for an instance without a
        set pixel."""
        out = np.full((len(self.box), 4, 2), np.nan)
        for i, (_, ax, ay, ex, ey, tmin, tmax, smax) in enumerate(self.box.tolist()):
            d = ex * ex + ey * ey
            if d:
                for c, (t, s) in enumerate(((tmin, 0), (tmax, 0), (tmax, smax), (tmin, smax))):
                    out[i, c] = (ax + (t * ex - s * ey) / d, ay + (t * ey + s * ex) / d)
        return out

    def rbox(self):
        """float64 [n, 5] = (cx, cy, w, h, angle): the centre, w = (tmax - tmin) / |e| the side along the chosen edge, h =
        smax / |e| the other side, angle = atan2(ey, ex) in degrees in (-180, 180], the direction of the w side measured from
        +x towards +y (y points down: clockwise on screen, as CVAT and labelme turn a box); NaN for an instance without a set
        pixel."""
        out = np.full((len(self.box), 5), np.nan)
        for i, (_, ax, ay, ex, ey, tmin, tmax, smax) in enumerate(self.box.tolist()):
            d = ex * ex + ey * ey
            if d:
                t, s = tmin + tmax, smax
                out[i] = (ax + (t * ex - s * ey) / (2.0 * d), ay + (t * ey + s * ex) / (2.0 * d), (tmax - tmin) / math.sqrt(d),
                          smax / math.sqrt(d), math.degrees(math.atan2(ey, ex)))
        return out

    def area(self):
        """float64 [n]: the rectangles' areas (tmax - tmin) smax / |e|^2; 0 for an instance without a set pixel."""
        out = np.zeros(len(self.box), np.float64)
        for i, (_, _, _, ex, ey, tmin, tmax, smax) in enumerate(self.box.tolist()):
            if ex or ey:
                out[i] = (tmax - tmin) * smax / (ex * ex + ey * ey)
        return out


def _check_set(who, pm):
    """What the library refuses about the bounds: mnc_mask_boundary's limits and the extent."""
    n = len(pm)
    if n > MAX_N:
        raise ValueError("%s: n=%d not in [0, %d]" % (who, n, MAX_N))
    for i in range(n):
        b = [int(v) for v in pm.bounds[i]]
        if not all(-MAX_COORD < v < MAX_COORD for v in b):
            raise ValueError("%s: masks[%d] coordinate out of range" % (who, i))
        h, w = pm.size(i)
        if h == 0 or w == 0:
            continue
        if w > MAX_EXTENT or h > MAX_EXTENT:
            raise ValueError("%s: masks[%d] is %d x %d (limit %d a side)" % (who, i, w, h, MAX_EXTENT))
        if h * w > MAX_AREA:
            raise ValueError("%s: masks[%d] covers %d pixels (limit %d)" % (who, i, h * w, MAX_AREA))


# ---- the statements ----

def moments_numpy(pm):
    """The sums as a plain loop on the host -- the specification csrc/mask_shape.hip is tested against.  -> Moments."""
    _check_set("moments_numpy", pm)
    m = np.zeros((len(pm), 6), np.int64)
    for i in range(len(pm)):
        h, w = pm.size(i)
        if h and w:
            y, x = (v.astype(np.int64) for v in np.nonzero(pm.dense(i)))
            m[i] = (x.size, x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum())
    return Moments(m, _origins(pm))


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _chain(points):
    """Points sorted by y -> those on the strictly convex chain that turns clockwise on screen (cross > 0 at every kept point)."""
    out = []
    for p in points:
        while len(out) >= 2 and _cross(out[-2], out[-1], p) <= 0:
            out.pop()
        out.append(p)
    return out


def hull_dense(m):
    """bool [h, w] -> [(x, y)]: the hull of one dense mask by the rule, relative to the array's corner; [] for no set pixel."""
    first, last = {}, {}
    for y in range(m.shape[0]):
        xs = np.flatnonzero(m[y])
        if xs.size:
            for Y in (y, y + 1):
                first[Y] = min(first.get(Y, int(xs[0])), int(xs[0]))
                last[Y] = max(last.get(Y, int(xs[-1]) + 1), int(xs[-1]) + 1)
    rows = sorted(first)
    if not rows:
        return []
    right = _chain([(last[Y], Y) for Y in rows])                             # downwards
    left = _chain([(first[Y], Y) for Y in reversed(rows)])                   # upwards
    return [left[-1]] + right + left[:-1]


def hull_numpy(pm):
    """The hulls as a plain loop on the host -- the specification csrc/mask_shape.hip is tested against.  -> Hulls."""
    _check_set("hull_numpy", pm)
    n = len(pm)
    vert_ptr, area2, parts = np.zeros(n + 1, np.int64), np.zeros(n, np.int64), []
    for i in range(n):
        h, w = pm.size(i)
        v = hull_dense(pm.dense(i)) if h and w else []
        vert_ptr[i + 1] = vert_ptr[i] + len(v)
        if v:
            area2[i] = sum(v[k][0] * v[(k + 1) % len(v)][1] - v[(k + 1) % len(v)][0] * v[k][1] for k in range(len(v)))
            parts.append(np.array(v, np.int64) + np.asarray(pm.bounds[i][:2], np.int64))
    xy = np.concatenate(parts).astype(np.int32) if parts else np.zeros((0, 2), np.int32)
    return Hulls(vert_ptr, np.ascontiguousarray(xy).reshape(-1, 2), area2)


def oriented_vertices(v):
    """[(x, y)] hull vertices (Python integers) -> ((k, ax, ay, ex, ey, tmin, tmax, smax), (d2, i, j)); zeros for none."""
    m = len(v)
    if m == 0:
        return (0,) * 8, (0,) * 3
    best = None
    for k in range(m):
        ax, ay = v[k]
        ex, ey = v[(k + 1) % m][0] - ax, v[(k + 1) % m][1] - ay
        t = [(px - ax) * ex + (py - ay) * ey for px, py in v]
        s = [ex * (py - ay) - ey * (px - ax) for px, py in v]
        A, D = (max(t) - min(t)) * max(s), ex * ex + ey * ey
        if best is None or A * best[1] < best[0] * D:
            best = (A, D, (k, ax, ay, ex, ey, min(t), max(t), max(s)))
    far = (0, 0, 0)
    for i in range(m):
        for j in range(i + 1, m):
            d2 = (v[i][0] - v[j][0]) ** 2 + (v[i][1] - v[j][1]) ** 2
            if d2 > far[0]:
                far = (d2, i, j)
    return best[2], far


def oriented_numpy(pm, hulls=None):
    """The rectangles of least area and the diameters as a plain loop on the host over hull_numpy(pm) (or the Hulls given) -- the
    specification csrc/mask_shape.hip is tested against.  -> OrientedBoxes."""
    hulls = hull_numpy(pm) if hulls is None else hulls
    n = len(hulls.area2)
    box, diameter = np.zeros((n, 8), np.int64), np.zeros((n, 3), np.int64)
    for i in range(n):
        box[i], diameter[i] = oriented_vertices([tuple(p) for p in hulls.vertices(i).tolist()])
    return OrientedBoxes(box, diameter)


# ---- the device ----

def moments(pm, device_id=None):
    """moments_numpy on the GPU (mnc_mask_moments): the same Moments field by field, six numbers per instance come back.  Invalid
    sets raise _lib.MncError (MNC_ERR_INVALID) before anything is launched.  A device-resident PackedMasks is fetched first."""
    pm = pm.fetch()
    m = np.zeros((len(pm), 6), np.int64)
    _lib.call("mnc_mask_moments", *(_set_args(pm, areas=False) + (_lib.ptr(m if len(pm) else np.zeros(6, np.int64)),
                                                                  _device_id(device_id))))
    return Moments(m, _origins(pm))


def hull_call(pm, xy=None, area2=None, device_id=0):
    """mnc_mask_hull as it is: xy None asks for vert_ptr and the count only (area2 is not written).  -> (vert_ptr, V)."""
    vert_ptr, total = np.zeros(len(pm) + 1, np.int64), ctypes.c_size_t(0)
    _lib.call("mnc_mask_hull", *(_set_args(pm, areas=False) + (
        _lib.ptr(vert_ptr), _lib.ptr(xy), _lib.ptr(area2), xy.size // 2 if xy is not None else 0, ctypes.addressof(total),
        int(device_id))))
    return vert_ptr, int(total.value)


def hull(pm, device_id=None):
    """hull_numpy on the GPU (mnc_mask_hull): the same Hulls field by field.  A sizes-only call, then the call with room."""
    pm = pm.fetch()
    dev = _device_id(device_id)
    total = hull_call(pm, None, None, dev)[1]
    xy, area2 = np.zeros((total, 2), np.int32), np.zeros(len(pm), np.int64)
    vert_ptr, _ = hull_call(pm, xy if total else np.zeros((1, 2), np.int32), area2 if len(pm) else np.zeros(1, np.int64), dev)
    return Hulls(vert_ptr, xy, area2)


def oriented(pm, device_id=None):
    """oriented_numpy on the GPU (mnc_mask_oriented): hull and calipers in one call, the hull vertices stay on the device; eleven
    numbers per instance come back."""
    pm = pm.fetch()
    n = len(pm)
    box, diameter = np.zeros((n, 8), np.int64), np.zeros((n, 3), np.int64)
    _lib.call("mnc_mask_oriented", *(_set_args(pm, areas=False) + (
        _lib.ptr(box if n else np.zeros(8, np.int64)), _lib.ptr(diameter if n else np.zeros(3, np.int64)), _device_id(device_id))))
    return OrientedBoxes(box, diameter)


def timing(on):
    """mnc_mask_shape_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_shape_timing", on)
