"""The numpy statements of mnc_amd.shape (moments_numpy, hull_numpy, oriented_numpy and the host methods of Moments, Hulls and
OrientedBoxes) pinned to facts that do not come from them: closed forms, scipy.spatial.ConvexHull of the pixel corners, integer
invariants of a convex polygon, exact fractions, a sweep over 20 001 directions, all-pairs distances and plain sums in Python
integers.  No GPU: tests/test_gpu_mask_shape.py pins the kernels to these statements."""
import fractions
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_shape_inputs as SI  # noqa: E402
from mnc_amd import shape as SH  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

CHECKED = ("sizes", "shapes", "discs", "many130", "real", "tall")


def _one(m, x0=0, y0=0):
    h, w = m.shape
    return SI._place([m], bounds=[[x0, y0, x0 + w - 1, y0 + h - 1]])


def _verts(hulls, i):
    return [tuple(p) for p in hulls.vertices(i).tolist()]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


# ---- closed forms ----

def test_one_pixel():
    pm = _one(np.ones((1, 1), bool), -4, 9)
    hulls, boxes, mom = SH.hull_numpy(pm), SH.oriented_numpy(pm), SH.moments_numpy(pm)
    assert _verts(hulls, 0) == [(-4, 9), (-3, 9), (-3, 10), (-4, 10)] and hulls.area2.tolist() == [2]
    assert boxes.area().tolist() == [1.0] and boxes.diameter.tolist() == [[2, 0, 2]]
    assert mom.m.tolist() == [[1, 0, 0, 0, 0, 0]] and mom.centroid().tolist() == [[-4.0, 9.0]]
    assert mom.axes().tolist() == [[0.0, 0.0]] and hulls.solidity(pm.areas).tolist() == [1.0]
    assert hulls.polygon(0) == [-4.0, 9.0, -3.0, 9.0, -3.0, 10.0, -4.0, 10.0]


@pytest.mark.parametrize("w,h", [(37, 11), (1, 90), (64, 64), (130, 2)])
def test_a_rectangle(w, h):
    pm = _one(np.ones((h, w), bool), 20, -30)
    hulls, boxes, mom = SH.hull_numpy(pm), SH.oriented_numpy(pm), SH.moments_numpy(pm)
    assert _verts(hulls, 0) == [(20, -30), (20 + w, -30), (20 + w, -30 + h), (20, -30 + h)]
    assert hulls.area2.tolist() == [2 * w * h] and hulls.solidity(pm.areas).tolist() == [1.0]
    assert boxes.box.tolist() == [[0, 20, -30, w, 0, 0, w * w, w * h]] and boxes.diameter[0, 0] == w * w + h * h
    assert boxes.corners()[0].tolist() == [[20.0, -30.0], [20.0 + w, -30.0], [20.0 + w, -30.0 + h], [20.0, -30.0 + h]]
    assert boxes.rbox()[0].tolist() == [20 + w / 2, -30 + h / 2, w, h, 0.0]
    mu = mom.central()[0]
    assert mu[0] / (w * h) == pytest.approx((w * w - 1) / 12, rel=1e-12) and mu[2] / (w * h) == pytest.approx((h * h - 1) / 12, rel=1e-12)
    assert mu[1] == 0 and mom.centroid()[0].tolist() == [20 + (w - 1) / 2, -30 + (h - 1) / 2]
    if w != h:
        assert mom.orientation()[0] == (0.0 if w > h else math.pi / 2)
        assert mom.axes()[0].tolist() == pytest.approx([4 * math.sqrt((max(w, h) ** 2 - 1) / 12), 4 * math.sqrt((min(w, h) ** 2 - 1) / 12)])


@pytest.mark.parametrize("steps", [2, 3, SI.STAIR, 200])
def test_a_diagonal_staircase_has_six_vertices(steps):
    hulls = SH.hull_numpy(_one(SI.staircase(steps)))
    assert _verts(hulls, 0) == [(0, 0), (1, 0), (steps, steps - 1), (steps, steps), (steps - 1, steps), (0, 1)]
    assert hulls.area2.tolist() == [2 * (2 * steps - 1)]


def test_empty_instances_and_empty_rows():
    pm = SI.get("shapes")
    hulls, boxes, mom = (SI.reference("shapes", what) for what in ("hull", "oriented", "moments"))
    for i in (7, 8):                                                             # rows and no pixel; no rows
        assert hulls.vert_ptr[i] == hulls.vert_ptr[i + 1] and hulls.area2[i] == 0 and hulls.polygon(i) == []
        assert not boxes.box[i].any() and not boxes.diameter[i].any() and not mom.m[i].any()
        assert np.isnan(mom.centroid()[i]).all() and np.isnan(mom.orientation()[i]) and np.isnan(boxes.rbox()[i]).all()
    assert hulls.solidity(pm.areas)[7:9].tolist() == [0.0, 0.0] and boxes.area()[7:9].tolist() == [0.0, 0.0]
    gaps = SI.gaps()
    filled = {Y for y in np.flatnonzero(gaps.any(axis=1)) for Y in (int(y), int(y) + 1)}
    rows = set((hulls.vertices(5)[:, 1] - pm.bounds[5, 1]).tolist())
    assert rows <= filled and min(rows) == 3 and max(rows) == 14
    none = SI.get("empty")
    assert SH.hull_numpy(none).vert_ptr.tolist() == [0] and SH.moments_numpy(none).m.shape == (0, 6)
    assert SH.oriented_numpy(none).box.shape == (0, 8)


# ---- the hull ----

@pytest.mark.parametrize("name", CHECKED)
def test_hull_is_scipys_hull_of_the_pixel_corners(name):
    scipy_spatial = pytest.importorskip("scipy.spatial")
    pm, hulls = SI.get(name), SI.reference(name, "hull")
    seen = 0
    for i in range(len(pm)):
        d = pm.dense(i)
        if not d.any():
            assert hulls.vert_ptr[i] == hulls.vert_ptr[i + 1]
            continue
        if d.sum() > 20000:      # a large mask: the first and the last set pixel of every row, between which the others lie
            ends = np.zeros_like(d)
            rows = np.flatnonzero(d.any(axis=1))
            ends[rows, d[rows].argmax(axis=1)] = ends[rows, d.shape[1] - 1 - d[rows, ::-1].argmax(axis=1)] = True
            d = ends
        pts = SI.corners_of(d) + pm.bounds[i, :2].astype(np.int64)
        v = _verts(hulls, i)
        ch = scipy_spatial.ConvexHull(pts)
        ring = pts[ch.vertices].tolist()                                         # (counterclockwise for points in the plane)
        assert set(v) == set(map(tuple, ring)) and len(set(v)) == len(v)
        # scipy's own area is a sum of rounded doubles (115.00000000000014 for 115): area2 equals the shoelace sum of scipy's ring
        # in Python integers exactly, and scipy's figure to its rounding
        exact = abs(sum(ring[k][0] * ring[(k + 1) % len(ring)][1] - ring[(k + 1) % len(ring)][0] * ring[k][1] for k in range(len(ring))))
        assert exact == hulls.area2[i] and abs(2 * ch.volume - exact) <= 1e-9 * exact
        seen += 1
    assert seen > 0


@pytest.mark.parametrize("name", CHECKED + ("wide",))
def test_hull_invariants(name):
    hulls = SI.reference(name, "hull")
    for i in range(len(hulls.area2)):
        v = _verts(hulls, i)
        if not v:
            continue
        m = len(v)
        assert m >= 4 and v[0] == min(v, key=lambda p: (p[1], p[0]))
        # strictly convex and clockwise on screen: every turn has a positive cross product (y points down)
        assert all(_cross(v[k], v[(k + 1) % m], v[(k + 2) % m]) > 0 for k in range(m))
        assert hulls.area2[i] == sum(v[k][0] * v[(k + 1) % m][1] - v[(k + 1) % m][0] * v[k][1] for k in range(m)) > 0


# ---- the rectangle of least area and the diameter ----

@pytest.mark.parametrize("name", CHECKED + ("wide",))
def test_chosen_edge_is_the_least_in_exact_fractions_and_holds_every_vertex(name):
    hulls, boxes = SI.reference(name, "hull"), SI.reference(name, "oriented")
    for i in range(len(hulls.area2)):
        v = _verts(hulls, i)
        if not v:
            continue
        m = len(v)
        areas = []
        for k in range(m):
            (ax, ay), (bx, by) = v[k], v[(k + 1) % m]
            ex, ey = bx - ax, by - ay
            t = [(px - ax) * ex + (py - ay) * ey for px, py in v]
            s = [ex * (py - ay) - ey * (px - ax) for px, py in v]
            assert min(s) == 0
            A, D = (max(t) - min(t)) * max(s), ex * ex + ey * ey
            assert A < 2 ** 64 and D < 2 ** 32
            areas.append(fractions.Fraction(A, D))
        k, ax, ay, ex, ey, tmin, tmax, smax = boxes.box[i].tolist()
        assert areas[k] == min(areas) == fractions.Fraction((tmax - tmin) * smax, ex * ex + ey * ey) and areas.index(min(areas)) == k
        assert (ax, ay) == v[k] and (ax + ex, ay + ey) == v[(k + 1) % m]
        for px, py in v:
            assert tmin <= (px - ax) * ex + (py - ay) * ey <= tmax and 0 <= ex * (py - ay) - ey * (px - ax) <= smax
        d2, a, b = boxes.diameter[i].tolist()
        pairs = [((v[p][0] - v[q][0]) ** 2 + (v[p][1] - v[q][1]) ** 2, -p, -q) for p in range(m) for q in range(p + 1, m)]
        assert (d2, -a, -b) == max(pairs)


@pytest.mark.parametrize("name", ("shapes", "discs", "many130"))
def test_no_direction_of_a_sweep_gives_a_smaller_rectangle(name):
    hulls, boxes = SI.reference(name, "hull"), SI.reference(name, "oriented")
    theta = np.linspace(0.0, math.pi / 2, 20001)
    c, s = np.cos(theta)[:, None], np.sin(theta)[:, None]
    area = boxes.area()
    for i in range(len(area)):
        if hulls.area2[i]:
            p = (hulls.vertices(i) - hulls.vertices(i)[0]).astype(np.float64)
            u, v = p[:, 0] * c + p[:, 1] * s, p[:, 1] * c - p[:, 0] * s
            swept = ((u.max(axis=1) - u.min(axis=1)) * (v.max(axis=1) - v.min(axis=1))).min()
            assert area[i] <= swept + 1e-9 and 2 * area[i] >= hulls.area2[i]


@pytest.mark.parametrize("name", ("sizes", "shapes", "real", "wide"))
def test_corners_and_rbox_agree(name):
    boxes, hulls = SI.reference(name, "oriented"), SI.reference(name, "hull")
    corners, rbox = boxes.corners(), boxes.rbox()
    for i in range(len(rbox)):
        if not hulls.area2[i]:
            continue
        cx, cy, w, h, angle = rbox[i]
        scale = max(1.0, np.abs(corners[i]).max())
        assert np.abs(corners[i].mean(axis=0) - (cx, cy)).max() <= 1e-9 * scale
        assert abs(np.linalg.norm(corners[i, 1] - corners[i, 0]) - w) <= 1e-9 * scale
        assert abs(np.linalg.norm(corners[i, 2] - corners[i, 1]) - h) <= 1e-9 * scale
        assert w * h == pytest.approx(boxes.area()[i], rel=1e-12) and -180.0 < angle <= 180.0
        d = math.radians(angle)
        ux, uy = math.cos(d), math.sin(d)
        want = [(cx + a * w / 2 * ux - b * h / 2 * uy, cy + a * w / 2 * uy + b * h / 2 * ux) for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        assert np.abs(corners[i] - np.array(want)).max() <= 1e-9 * scale
        # every hull vertex lies in the rectangle of the corners
        p = hulls.vertices(i).astype(np.float64) - (cx, cy)
        assert (np.abs(p[:, 0] * ux + p[:, 1] * uy) <= w / 2 + 1e-9 * scale).all()
        assert (np.abs(p[:, 1] * ux - p[:, 0] * uy) <= h / 2 + 1e-9 * scale).all()


# ---- the moments ----

@pytest.mark.parametrize("name", CHECKED + ("wide",))
def test_moments_are_the_plain_sums(name):
    pm, mom = SI.get(name), SI.reference(name, "moments")
    assert mom.m.dtype == np.int64 and np.array_equal(mom.origin, pm.bounds[:, :2])
    central, centroid = mom.central(), mom.centroid()
    for i in range(len(pm)):
        ys, xs = (v.tolist() for v in np.nonzero(pm.dense(i)))
        want = [len(xs), sum(xs), sum(ys), sum(x * x for x in xs), sum(x * y for x, y in zip(xs, ys)), sum(y * y for y in ys)]
        assert mom.m[i].tolist() == want and all(v < 2 ** 56 for v in want)
        if xs:
            x, y = np.array(xs, np.float64), np.array(ys, np.float64)
            mx, my = x.mean(), y.mean()
            assert centroid[i].tolist() == pytest.approx([pm.bounds[i, 0] + mx, pm.bounds[i, 1] + my], rel=1e-12)
            sums = [((x - mx) ** 2).sum(), ((x - mx) * (y - my)).sum(), ((y - my) ** 2).sum()]
            scale = max(sums[0], sums[2], 1.0)
            assert np.abs(central[i] - sums).max() <= 1e-9 * scale


def test_the_wide_row_reaches_the_stated_widths():
    pm, mom = SI.get("wide"), SI.reference("wide", "moments")
    assert pm.size(0) == (2, 32768) and pm.bounds[0, 0] == -2 ** 24 + 1
    assert mom.m[0, 3] > 2 ** 42 and mom.centroid()[0, 0] < -2 ** 24 + 32768
    hulls = SI.reference("wide", "hull")
    assert _verts(hulls, 0)[0] == (-2 ** 24 + 1, 2 ** 24 - 3) and hulls.area2.tolist() == [4 * 32768]


def test_orientation_and_axes_of_a_slanted_bar():
    m = np.zeros((60, 60), bool)
    for k in range(60):
        m[k, max(k - 2, 0):k + 3] = True                                          # a bar along the +x +y diagonal
    mom = SH.moments_numpy(_one(m))
    assert mom.orientation()[0] == pytest.approx(math.pi / 4, abs=1e-3)
    major, minor = mom.axes()[0]
    assert major > 10 * minor > 0


# ---- refusals ----

def test_bounds_beyond_the_limits_are_refused():
    wide = PackedMasks([[0, 0, 32768, 0]], [0], [0], None, None, np.zeros(513, np.uint64))
    high = PackedMasks([[0, 0, 0, 32768]], [0], [0], None, None, np.zeros(32769, np.uint64))
    far = PackedMasks([[2 ** 24, 0, 2 ** 24 + 1, 0]], [0], [0], None, None, np.zeros(1, np.uint64))
    many = np.zeros((2049, 4), np.int32)
    many[:, 2:] = -1
    many = PackedMasks(many, np.zeros(2049, np.int64), np.zeros(2049, np.int64), None, None, np.zeros(0, np.uint64))
    for bad in (wide, high, far, many):
        for what in (SH.moments_numpy, SH.hull_numpy, SH.oriented_numpy):
            with pytest.raises(ValueError):
                what(bad)
    ok = PackedMasks([[0, 0, 32767, 0]], [0], [1], None, None, np.array([1] + [0] * 511, np.uint64))
    assert SH.hull_numpy(ok).area2.tolist() == [2] and SH.moments_numpy(ok).m[0, 0] == 1
