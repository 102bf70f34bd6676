"""Outlines of packed instance masks as closed rectilinear polygons (include/mnc_hip.h n13, csrc/mask_contours.hip) on
mnc_amd.masks.PackedMasks: the way out of the packed layout as vectors.

    contours_numpy(pm, connectivity=8)             -> Contours(loop_ptr, vert_ptr, area, xy): the rule as a plain sequential walk
    contours(pm, connectivity=8, device_id=None)   the same through mnc_mask_contours (the GPU)
    contours_call(pm, connectivity, loop_cap, vert_cap, ...)   the entry as it is
    PackedMasks.contours / .polygons               the methods
    simplify_numpy(c, epsilon)                     -> SimplifiedContours: the outlines simplified to a tolerance in pixels, the rule
                                                   of n14 below in Python integers
    simplify(c, epsilon, device_id=None)           the same through mnc_contours_simplify (the GPU); Contours.simplify is the method
    simplify_call(vert_ptr, xy, q, ...)            the entry as it is

The rule.  Pixel (x, y) of the image is the unit square [x, x + 1] x [y, y + 1]; vertices are lattice points in image coordinates
(the instance's bounds added in), int32.  A boundary edge is a unit side between a set pixel of instance i and an unset one; pixels
outside the instance's bounds are unset, padding bits are not trusted.  An edge is directed so that the set pixel is on its right,
y pointing down: the top side runs +x, the right side +y, the bottom side -x, the left side -y.  Outer boundaries then run clockwise
on screen and holes the other way.  The successor of an edge is the boundary edge that leaves its head vertex.  Two leave only where
two set pixels touch at a corner alone: there connectivity = 8 takes the left turn, so that the two pixels share one loop, and
connectivity = 4 the right turn, so that each keeps its own.  The successor relation is a permutation of the edges; its cycles are
the loops.

The vertices of a loop are the tails of those of its edges whose predecessor has another direction: consecutive vertices differ in
exactly one coordinate, horizontal and vertical sides alternate, no three consecutive vertices are collinear.  The list starts at
the loop's smallest vertex in (y, x) order and follows the direction of travel; the first vertex is not repeated at the end.  A
loop passes through its start vertex once, and a vertex is the start of at most one loop.  A loop is a hole exactly when its first
side runs +y.  The loops of an instance are ordered by their start vertex (y, x); the loops of a set are those of instance 0, then
of instance 1, ...  An instance without rows or without a set pixel has no loops.

    Contours   loop_ptr int64 [n + 1]: instance i has the loops loop_ptr[i] .. loop_ptr[i + 1] - 1; vert_ptr int64 [L + 1]: loop l
               has the vertices xy[vert_ptr[l] : vert_ptr[l + 1]]; area int64 [L]: the signed shoelace area, positive for an outer
               loop, negative for a hole -- the areas of an instance's loops sum to its pixel count; xy int32 [V, 2] (x, y)

A rectilinear polygon on lattice points is rasterised exactly by the rule of mnc_amd.polygons (a horizontal edge at y = k from
x = a to x = b toggles exactly the columns a .. b - 1 at row k, vertical edges toggle nothing): the XOR of an instance's loops,
rasterised one by one, is the instance.

The simplification (include/mnc_hip.h n14, csrc/contour_simplify.hip) is Douglas-Peucker on closed loops in exact integer arithmetic,
so that the parallel form equals this sequential one bit for bit.  The loops are any closed integer loops (vert_ptr, xy), the first
vertex not repeated.  epsilon is in pixels and is quantised to sixteenths: q = int(round(epsilon * 16)), Python's round-half-even of
the double.  For a loop v_0 .. v_(k-1), v_k = v_0:
    k <= 3: unchanged.
    The anchors are index 0 and B, the index in 1 .. k - 1 with the largest |v_B - v_0|^2, the lowest on ties.  The chains are
    (0, B) and (B, k).
    The deviation of m in the segment (i, j), i < m < j, with a = v_i, b = v_(j mod k), p = v_m, ab = b - a, ap = p - a, L = ab.ab
    and t = ap.ab is the pair (N, D): L == 0 gives (|ap|^2, 1); t <= 0 gives (|ap|^2 L, L); t >= L gives (|p - b|^2 L, L); otherwise
    ((ab x ap)^2, L).  N / D is the squared distance of p from the segment; D is common to the segment.
    split(i, j): nothing if j - i < 2; m* is the m with the largest N, the lowest on ties; if 256 N > q^2 D, m* is kept and
    split(i, m*) and split(m*, j) follow.
    Both chains are split.  If only 0 and B are kept after that, the third anchor applies: the m with the largest N over both
    chains (they share L, so the N compare), the lowest index on ties, is kept whatever q is, and the two halves of its chain are
    split.  A closed loop never comes out with fewer than three vertices, and the vertex count does not rise with epsilon.
    The output is the kept vertices in index order; v_0 is always first.
Like every plain Douglas-Peucker the rule does not preserve topology: a simplified loop may touch or cross itself or another.
Coordinates are accepted in [-2^24, 2^24] and q in [0, 2^20]: N is below 2^102.

    SimplifiedContours   a Contours whose loop_ptr is the input's (loops are never dropped) and whose area is the input's, carried
               over: the area of the UNSIMPLIFIED loop, whose sign still tells a hole; index int64 [V']: the position of each kept
               vertex in the input's xy

There is no fallback: without the library or a GPU the device functions raise.  They read host arrays: a device-resident
PackedMasks (engine results) is fetched to the host first."""
import ctypes

import numpy as np

from . import _lib
from .masks import _device_id, _set_args

MAX_N = 2048
MAX_WORDS = 2 ** 25
MAX_Q = 2 ** 20                                        # the tolerance in sixteenths of a pixel
MAX_COORD = 2 ** 24
MAX_LOOPS = 2 ** 24
MAX_VERTS = 2 ** 27
INVALID = 1
# east, south, west, north: clockwise on screen, so that a right turn is + 1 and a left turn is - 1
_DX = (1, 0, -1, 0)
_DY = (0, 1, 0, -1)


class Contours(object):
    """The loops of one set.  The four arrays are checked against each other: lengths, dtypes, pointers that start at 0, do not
    decrease and end at the sizes."""
    FIELDS = ("loop_ptr", "vert_ptr", "area", "xy")

    def __init__(self, loop_ptr, vert_ptr, area, xy):
        self.loop_ptr = np.ascontiguousarray(loop_ptr, np.int64).reshape(-1)
        self.vert_ptr = np.ascontiguousarray(vert_ptr, np.int64).reshape(-1)
        self.area = np.ascontiguousarray(area, np.int64).reshape(-1)
        self.xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        for name, ptr, size in (("loop_ptr", self.loop_ptr, len(self.area)), ("vert_ptr", self.vert_ptr, len(self.xy))):
            if len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != size or (np.diff(ptr) < 0).any():
                raise ValueError("Contours: %s does not run from 0 to %d without decreasing" % (name, size))
        if len(self.vert_ptr) != len(self.area) + 1:
            raise ValueError("Contours: vert_ptr has %d entries for %d loops" % (len(self.vert_ptr), len(self.area)))

    def __len__(self):
        """The instances."""
        return len(self.loop_ptr) - 1

    def _instance(self, i):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError("Contours: instance %d of %d" % (i, len(self)))
        return range(int(self.loop_ptr[i]), int(self.loop_ptr[i + 1]))

    def loop(self, l):
        """int32 [k, 2]: the vertices of loop l of the set."""
        return self.xy[int(self.vert_ptr[l]):int(self.vert_ptr[l + 1])]

    def loops(self, i):
        """[(xy int32 [k, 2], area int)] of instance i, in loop order."""
        return [(self.loop(l), int(self.area[l])) for l in self._instance(i)]

    def polygons(self, i, holes=False):
        """Instance i as flat [x0, y0, x1, y1, ...] float lists, the form PackedMasks.from_polygons reads: its outer loops, and
        with holes=True the holes as well, in loop order (a reader that ORs the polygons, as COCO's does, fills them; one that XORs
        them gets the mask back)."""
        return [[float(v) for v in self.loop(l).reshape(-1)] for l in self._instance(i) if holes or self.area[l] > 0]

    def simplify(self, epsilon, device_id=None):
        """The loops simplified to epsilon pixels on the GPU (simplify below) -> SimplifiedContours."""
        return simplify(self, epsilon, device_id)


class SimplifiedContours(Contours):
    """The loops of a Contours after simplify: loop_ptr and area are the input's (area is that of the unsimplified loop),
    index [V'] is the position of each vertex in the input's xy."""
    FIELDS = Contours.FIELDS + ("index",)

    def __init__(self, loop_ptr, vert_ptr, area, xy, index):
        Contours.__init__(self, loop_ptr, vert_ptr, area, xy)
        self.index = np.ascontiguousarray(index, np.int64).reshape(-1)
        if len(self.index) != len(self.xy):
            raise ValueError("SimplifiedContours: index has %d entries for %d vertices" % (len(self.index), len(self.xy)))


def _check(who, connectivity):
    connectivity = int(connectivity)
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity=%d is not 4 or 8" % (who, connectivity))
    return connectivity


def _check_set(who, pm):
    """What the library refuses about the set beyond HostMaskSet::check: the count and the words of the lattice rows."""
    n = len(pm)
    if n > MAX_N:
        raise ValueError("%s: n=%d not in [0, %d]" % (who, n, MAX_N))
    words = 0
    for i in range(n):
        h, w = pm.size(i)
        if h and w:
            words += (h + 1) * ((w + 64) // 64)
        if words > MAX_WORDS:
            raise ValueError("%s: more than %d words of rows in the set (at masks[%d])" % (who, MAX_WORDS, i))


def _trace(m, eight, x0, y0):
    """The loops of one dense mask whose pixel (0, 0) is pixel (x0, y0) of the image -> [(vertices [(x, y)], area)] in loop order."""
    h, w = m.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = m
    # pixel (X, Y) is p[Y + 1, X + 1]; the edges that leave lattice point (X, Y), 0 <= X <= w, 0 <= Y <= h
    up, dn, upl, dnl = p[:-1, 1:], p[1:, 1:], p[:-1, :-1], p[1:, :-1]
    leaves = np.stack((dn & ~up, dnl & ~dn, upl & ~dnl, up & ~upl))
    ys, xs = np.nonzero(leaves.any(axis=0))
    out = leaves.tolist()
    seen = np.zeros(leaves.shape, bool).tolist()
    turns = (3, 0, 1) if eight else (1, 0, 3)          # at a point with two ways on: the left turn, resp. the right turn
    loops = []
    for y, x in zip(ys.tolist(), xs.tolist()):         # raster order of the tail: a loop is met first at its smallest vertex
        for d in range(4):
            if not out[d][y][x] or seen[d][y][x]:
                continue
            verts, twice, cx, cy, cd, before = [], 0, x, y, d, -1
            while not seen[cd][cy][cx]:                # the successor is a permutation: the walk comes back to its first edge
                seen[cd][cy][cx] = True
                if cd != before:
                    verts.append((cx + x0, cy + y0))
                before = cd
                nx, ny = cx + _DX[cd], cy + _DY[cd]
                twice += (cx + x0) * (ny + y0) - (nx + x0) * (cy + y0)
                cx, cy = nx, ny
                cd = next((cd + t) & 3 for t in turns if out[(cd + t) & 3][cy][cx])
            if (cx, cy, cd) != (x, y, d) or before == d:
                raise AssertionError("contours_numpy: the loop from (%d, %d) does not close in a turn at its start" % (x, y))
            loops.append((verts, twice // 2))
    return loops


def contours_numpy(pm, connectivity=8):
    """The outlines as a plain sequential walk on the host -- the specification csrc/mask_contours.hip is tested against.  Raises
    ValueError where mnc_mask_contours returns MNC_ERR_INVALID for the connectivity, the instance count or the words."""
    eight = _check("contours_numpy", connectivity) == 8
    _check_set("contours_numpy", pm)
    n = len(pm)
    loop_ptr, vert_ptr, area, xy = np.zeros(n + 1, np.int64), [0], [], []
    for i in range(n):
        h, w = pm.size(i)
        if h and w:
            for verts, a in _trace(pm.dense(i), eight, int(pm.bounds[i][0]), int(pm.bounds[i][1])):
                xy.extend(verts)
                vert_ptr.append(len(xy))
                area.append(a)
        loop_ptr[i + 1] = len(area)
    return Contours(loop_ptr, np.array(vert_ptr, np.int64), np.array(area, np.int64), np.array(xy, np.int32).reshape(-1, 2))


# ---- the device ----

def contours_call(pm, connectivity, loop_cap, vert_cap, device_id=0, sizes_only=False):
    """mnc_mask_contours as it is, with room for loop_cap loops and vert_cap vertices -> (loop_ptr, vert_ptr [loop_cap + 1], area
    [loop_cap], xy [vert_cap, 2], L, V).  Too little room raises _lib.MncError (MNC_ERR_INVALID) with .needed = (L, V); sizes_only
    passes no xy at all."""
    n = len(pm)
    loop_ptr = np.zeros(n + 1, np.int64)
    vert_ptr, area, xy = np.zeros(loop_cap + 1, np.int64), np.zeros(loop_cap, np.int64), np.zeros((vert_cap, 2), np.int32)
    n_loops, n_verts = ctypes.c_size_t(0), ctypes.c_size_t(0)
    try:
        _lib.call("mnc_mask_contours", *(_set_args(pm, areas=False) + (
            int(connectivity), _lib.ptr(loop_ptr), _lib.ptr(vert_ptr), _lib.ptr(area), None if sizes_only else _lib.ptr(xy),
            int(loop_cap), int(vert_cap), ctypes.addressof(n_loops), ctypes.addressof(n_verts), int(device_id))))
    except _lib.MncError as e:
        e.needed = (int(n_loops.value), int(n_verts.value))
        raise
    return loop_ptr, vert_ptr, area, xy, int(n_loops.value), int(n_verts.value)


def contours(pm, connectivity=8, device_id=None):
    """contours_numpy on the GPU (mnc_mask_contours): the same Contours field by field.  One call with room for 256 + 32 n loops
    and 32 times as many vertices (a voted instance at image resolution has a dozen or two loops, most of them pinholes), a second
    one when the masks have more.  Invalid arguments raise ValueError, invalid sets
    _lib.MncError (MNC_ERR_INVALID), before anything is launched.  A device-resident PackedMasks is fetched to the host first."""
    connectivity = _check("contours", connectivity)
    pm = pm.fetch()
    dev = _device_id(device_id)
    loop_cap = 256 + 32 * len(pm)
    vert_cap = 32 * loop_cap
    try:
        out = contours_call(pm, connectivity, loop_cap, vert_cap, dev)
    except _lib.MncError as e:
        if e.code != INVALID or (e.needed[0] <= loop_cap and e.needed[1] <= vert_cap):
            raise
        out = contours_call(pm, connectivity, max(e.needed[0], 1), max(e.needed[1], 1), dev)
    loop_ptr, vert_ptr, area, xy, L, V = out
    if L == 0:
        vert_ptr[0] = 0                                # (nothing past the reported sizes is written: not even the end of no loops)
    return Contours(loop_ptr, vert_ptr[:L + 1].copy(), area[:L].copy(), xy[:V].copy())


def polygons(pm, connectivity=8, device_id=None, epsilon=0.0):
    """One COCO `segmentation` per instance: its outer loops as flat float lists, the holes dropped (PackedMasks.polygons).
    epsilon > 0: the loops simplified to that many pixels (simplify); epsilon == 0 is the exact outline, without that call."""
    q = _quantise("polygons", epsilon)
    c = contours(pm, connectivity, device_id)
    if q > 0:
        c = simplify(c, epsilon, device_id)
    return [c.polygons(i) for i in range(len(c))]


def timing(on):
    """mnc_mask_contours_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_contours_timing", on)


# ---- the simplification (n14) ----

def _quantise(who, epsilon):
    """epsilon in pixels -> q in sixteenths: Python's round-half-even of the double."""
    e = float(epsilon)
    if not e >= 0.0:
        raise ValueError("%s: epsilon=%r is negative or not a number" % (who, epsilon))
    if e * 16 > MAX_Q + 1:
        raise ValueError("%s: epsilon=%r is more than %d sixteenths of a pixel" % (who, epsilon, MAX_Q))
    q = int(round(e * 16))
    if q > MAX_Q:
        raise ValueError("%s: epsilon=%r is more than %d sixteenths of a pixel" % (who, epsilon, MAX_Q))
    return q


def _check_loops(who, vert_ptr, xy):
    """What mnc_contours_simplify refuses about the loops."""
    if len(vert_ptr) - 1 > MAX_LOOPS or len(xy) > MAX_VERTS:
        raise ValueError("%s: %d loops or %d vertices above %d and %d" % (who, len(vert_ptr) - 1, len(xy), MAX_LOOPS, MAX_VERTS))
    if len(vert_ptr) < 1 or vert_ptr[0] != 0 or vert_ptr[-1] != len(xy) or (np.diff(vert_ptr) < 0).any():
        raise ValueError("%s: vert_ptr does not run from 0 to %d without decreasing" % (who, len(xy)))
    if len(xy) and (xy.min() < -MAX_COORD or xy.max() > MAX_COORD):
        raise ValueError("%s: a coordinate outside [-%d, %d]" % (who, MAX_COORD, MAX_COORD))


def _best(pts, P, k, i, j):
    """The segment (i, j) of a loop of k vertices, j - i >= 2 -> (N, m*, D): the largest numerator among i < m < j, the lowest m
    that has it, and the segment's denominator.  pts holds the vertices as Python integers; P, where the loop is long enough to
    have one, as an array for the long segments -- int64 where every product fits (_simplify_loop), Python integers otherwise:
    the same integers either way."""
    (ax, ay), (bx, by) = pts[i], pts[j % k]
    abx, aby = bx - ax, by - ay
    L = abx * abx + aby * aby
    if P is None or j - i <= 24:
        N = []
        for px, py in pts[i + 1:j]:
            apx, apy = px - ax, py - ay
            t = apx * abx + apy * aby
            if L == 0:
                N.append(apx * apx + apy * apy)
            elif t <= 0:
                N.append((apx * apx + apy * apy) * L)
            elif t >= L:
                N.append(((px - bx) * (px - bx) + (py - by) * (py - by)) * L)
            else:
                N.append((abx * apy - aby * apx) ** 2)
    else:
        p = P[i + 1:j]
        apx, apy, bpx, bpy = p[:, 0] - ax, p[:, 1] - ay, p[:, 0] - bx, p[:, 1] - by
        near = apx * apx + apy * apy
        if L == 0:
            N = near
        else:
            t, cross = apx * abx + apy * aby, abx * apy - aby * apx
            N = np.where(t <= 0, near * L, np.where(t >= L, (bpx * bpx + bpy * bpy) * L, cross * cross))
        N = [int(v) for v in N.tolist()]
    top = max(N)
    return top, i + 1 + N.index(top), L or 1


def _simplify_loop(xy, q):
    """One loop int32 [k, 2] -> the kept indices in order."""
    k = len(xy)
    if k <= 3:
        return list(range(k))
    pts, P = [(int(x), int(y)) for x, y in xy.tolist()], None
    if k > 24:
        # |N| <= 4 R^4 for coordinates that span R: int64 holds it up to R = 2^15; beyond, Python integers (object arrays)
        P = xy.astype(np.int64) if int(xy.max()) - int(xy.min()) <= 2 ** 15 else xy.astype(object)
    x0, y0 = pts[0]
    far = [(x - x0) * (x - x0) + (y - y0) * (y - y0) for x, y in pts[1:]]
    B = 1 + far.index(max(far))
    kept = {0, B}
    chains = [(0, B), (B, k)]
    first = [_best(pts, P, k, i, j) if j - i >= 2 else None for i, j in chains]
    over = [f is not None and 256 * f[0] > q * q * f[2] for f in first]
    if not any(over):
        # the third anchor: the largest N of both chains (they share L), chain (0, B) -- the lower indices -- on ties
        over[0 if first[1] is None or (first[0] is not None and first[0][0] >= first[1][0]) else 1] = True
    open_ = []
    for (i, j), f, o in zip(chains, first, over):
        if o:
            kept.add(f[1])
            open_ += [(i, f[1]), (f[1], j)]
    while open_:                                       # split(i, j), without recursion: a comb is k / 2 deep
        i, j = open_.pop()
        if j - i < 2:
            continue
        N, m, D = _best(pts, P, k, i, j)
        if 256 * N > q * q * D:
            kept.add(m)
            open_ += [(i, m), (m, j)]
    return sorted(kept)


def _simplify_arrays(vert_ptr, xy, q):
    """-> (out_vert_ptr int64 [L + 1], index int64 [V']) of the rule."""
    out_ptr, index = np.zeros(len(vert_ptr), np.int64), []
    for l in range(len(vert_ptr) - 1):
        v0, v1 = int(vert_ptr[l]), int(vert_ptr[l + 1])
        index.extend(v0 + m for m in _simplify_loop(xy[v0:v1], q))
        out_ptr[l + 1] = len(index)
    return out_ptr, np.array(index, np.int64)


def simplify_numpy(c, epsilon):
    """The loops of a Contours simplified to epsilon pixels, sequentially in Python integers -- the specification
    csrc/contour_simplify.hip is tested against -> SimplifiedContours.  Raises ValueError for a negative or NaN epsilon, one of
    more than 2^20 sixteenths, and for what mnc_contours_simplify refuses about the loops."""
    q = _quantise("simplify_numpy", epsilon)
    _check_loops("simplify_numpy", c.vert_ptr, c.xy)
    out_ptr, index = _simplify_arrays(c.vert_ptr, c.xy, q)
    return SimplifiedContours(c.loop_ptr.copy(), out_ptr, c.area.copy(), c.xy[index], index)


def simplify_call(vert_ptr, xy, q, device_id=0):
    """mnc_contours_simplify as it is: vert_ptr int64 [L + 1], xy int32 [V, 2], q in sixteenths of a pixel -> (out_vert_ptr
    [L + 1], out_xy [V, 2], out_index [V], V'), the outputs with the input's room and zero past what was written.  What the entry
    refuses raises _lib.MncError (MNC_ERR_INVALID)."""
    vert_ptr = np.ascontiguousarray(vert_ptr, np.int64).reshape(-1)
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    L, V = len(vert_ptr) - 1, len(xy)
    out_ptr, out_xy, out_index = np.zeros(L + 1, np.int64), np.zeros((V, 2), np.int32), np.zeros(V, np.int64)
    kept = ctypes.c_size_t(0)
    _lib.call("mnc_contours_simplify", _lib.ptr(vert_ptr), _lib.ptr(xy), L, V, int(q), _lib.ptr(out_ptr), _lib.ptr(out_xy),
              _lib.ptr(out_index), ctypes.addressof(kept), int(device_id))
    return out_ptr, out_xy, out_index, int(kept.value)


def simplify(c, epsilon, device_id=None):
    """simplify_numpy on the GPU (mnc_contours_simplify): the same SimplifiedContours field by field, in one call.  Invalid
    arguments raise ValueError before the library is looked for."""
    q = _quantise("simplify", epsilon)
    _check_loops("simplify", c.vert_ptr, c.xy)
    out_ptr, out_xy, out_index, kept = simplify_call(c.vert_ptr, c.xy, q, _device_id(device_id))
    return SimplifiedContours(c.loop_ptr.copy(), out_ptr, c.area.copy(), out_xy[:kept].copy(), out_index[:kept].copy())


def simplify_timing(on):
    """mnc_contours_simplify_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0:
    none)."""
    return _lib.timing("mnc_contours_simplify_timing", on)
