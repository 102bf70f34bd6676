"""The statement of the simplification rule (mnc_amd/contours.py:simplify_numpy, include/mnc_hip.h n14) without a GPU, pinned to
facts that do not come from it: the identity at epsilon 0, the subsequence structure, the tolerance by brute force in Python
integers against the kept neighbours, the vertex counts, closed forms (rectangles, the staircase triangle, the single pixel, the
loop that needs 128 bits), the rasterised result against scipy's distance transform, and what is refused -- nothing here may open a
device."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import contour_simplify_inputs as SI  # noqa: E402
import mask_contours_inputs as TI  # noqa: E402
import mask_overlap_inputs as MI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import components as CC  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402
from mnc_amd import polygons as PG  # noqa: E402

OTHER = {4: 8, 8: 4}
SETS = list(TI.SETS)


def one(m, x=0, y=0):
    m = np.asarray(m, bool)
    h, w = m.shape
    return CT.contours_numpy(MI.pack([[x, y, x + w - 1, y + h - 1]], [m], dirty=True), 8)


def loops_of(c):
    return [(int(c.vert_ptr[l]), int(c.vert_ptr[l + 1])) for l in range(len(c.area))]


# ---- structure ----

@pytest.mark.parametrize("connectivity", SI.CONNECTIVITIES)
@pytest.mark.parametrize("name", SETS)
def test_epsilon_0_is_the_identity_on_outlines(name, connectivity):
    """No three consecutive vertices of an outline are collinear, so no vertex lies on the segment of its neighbours."""
    c, s = TI.reference(name, connectivity), SI.reference(name, connectivity, 0)
    assert TI.same_contours(s, c) and SI.same_array(s.index, np.arange(len(c.xy), dtype=np.int64))
    assert isinstance(s, CT.SimplifiedContours) and s.FIELDS == ("loop_ptr", "vert_ptr", "area", "xy", "index")


@pytest.mark.parametrize("connectivity", SI.CONNECTIVITIES)
@pytest.mark.parametrize("name", SETS)
def test_the_result_is_a_subsequence_of_every_loop_that_starts_at_its_first_vertex(name, connectivity):
    c = TI.reference(name, connectivity)
    for q in SI.QS:
        s = SI.reference(name, connectivity, q)
        assert SI.same_array(s.loop_ptr, c.loop_ptr) and SI.same_array(s.area, c.area) and len(s.vert_ptr) == len(c.vert_ptr)
        assert s.index.dtype == np.int64 and s.xy.dtype == np.int32 and SI.same_array(s.xy, c.xy[s.index])
        assert (np.diff(s.index) > 0).all()                                  # strictly increasing over the whole set, so in every loop
        heads = s.vert_ptr[:-1][np.diff(s.vert_ptr) > 0]
        assert s.index[heads].tolist() == c.vert_ptr[:-1][np.diff(c.vert_ptr) > 0].tolist()
        # every kept vertex lies in its own loop
        assert (np.searchsorted(c.vert_ptr, s.index, side="right") - 1).tolist() == np.repeat(np.arange(len(s.area)), np.diff(s.vert_ptr)).tolist()


def within_tolerance(c, s, q):
    """Every dropped vertex against the segment of its kept neighbours: 256 N <= q^2 D, in Python integers."""
    for l, (v0, v1) in enumerate(loops_of(c)):
        kept = s.index[int(s.vert_ptr[l]):int(s.vert_ptr[l + 1])].tolist()
        if len(kept) == v1 - v0:
            continue
        pts = c.xy[v0:v1].tolist()
        ends = kept + [v1]
        for i, j in zip(ends[:-1], ends[1:]):
            a, b = pts[i - v0], pts[(j - v0) % (v1 - v0)]
            for m in range(i + 1, j):
                N, D = SI.deviation(a, b, pts[m - v0])
                if 256 * N > q * q * D:
                    return "loop %d: vertex %d is %d / %d from (%d, %d)" % (l, m, N, D, i, j)
    return None


@pytest.mark.parametrize("connectivity", SI.CONNECTIVITIES)
@pytest.mark.parametrize("name", SETS)
def test_every_dropped_vertex_is_within_the_tolerance_of_its_kept_neighbours(name, connectivity):
    """Without an exception for the third anchor: a forced vertex is an extra one, and what is dropped beside it was dropped by a
    split that stayed under the tolerance.  A loop that comes out with three vertices has three distinct ones."""
    c = TI.reference(name, connectivity)
    for q in SI.QS:
        s = SI.reference(name, connectivity, q)
        assert within_tolerance(c, s, q) is None
        for l in np.nonzero(np.diff(s.vert_ptr) == 3)[0]:
            assert len(set(s.index[int(s.vert_ptr[l]):int(s.vert_ptr[l + 1])].tolist())) == 3


@pytest.mark.parametrize("q", (0, 8, 16, 24))
def test_loops_of_ties_and_repeated_vertices_are_within_the_tolerance(q):
    c, s = SI.general("ties"), SI.general_reference("ties", q)
    assert within_tolerance(c, s, q) is None
    assert (np.diff(s.vert_ptr) >= 3).all() and SI.same_array(s.xy, c.xy[s.index])


@pytest.mark.parametrize("connectivity", SI.CONNECTIVITIES)
@pytest.mark.parametrize("name", SETS)
def test_no_loop_falls_below_three_vertices_and_the_count_does_not_rise_with_epsilon(name, connectivity):
    c = TI.reference(name, connectivity)
    totals = []
    for q in SI.QS:
        s = SI.reference(name, connectivity, q)
        assert (np.diff(s.vert_ptr) >= np.minimum(np.diff(c.vert_ptr), 3)).all()
        totals.append(len(s.xy))
    assert totals == sorted(totals, reverse=True) and totals[0] == len(c.xy)


def test_the_counts_of_the_two_large_sets():
    """The outer loops' vertices at 1 px and at 2.5 px, connectivity 8."""
    for name, before, counts in (("many", 54358, (20128, 12706)), ("real", 416, (109, 50))):
        c = TI.reference(name, 8)
        outer = np.repeat(c.area > 0, np.diff(c.vert_ptr))
        assert int(outer.sum()) == before
        assert tuple(int(outer[SI.reference(name, 8, q).index].sum()) for q in (16, 40)) == counts


# ---- closed forms ----

def test_a_rectangle_keeps_its_corners_up_to_a_bound_and_is_a_triangle_beyond():
    """The anchors are two opposite corners (the diagonal is longer than a side).  Each of the other two is w h / sqrt(w^2 + h^2)
    from the diagonal: N = (w h)^2, D = w^2 + h^2, so both are kept exactly while 256 (w h)^2 > q^2 (w^2 + h^2).  Beyond, neither
    is, and the third anchor puts the first of them back."""
    for x, y, w, h in ((0, 0, 2, 2), (3, 5, 7, 2), (-4, -9, 64, 3), (10, 0, 5, 40), (0, 0, 1, 1)):
        c = one(np.ones((h, w), bool), x, y)
        corners = [[x, y], [x + w, y], [x + w, y + h], [x, y + h]]
        assert c.xy.tolist() == corners
        bound = math.isqrt((256 * w * w * h * h - 1) // (w * w + h * h))          # the largest q with q^2 (w^2 + h^2) < 256 (w h)^2
        assert 256 * w * w * h * h > bound ** 2 * (w * w + h * h) and 256 * w * w * h * h <= (bound + 1) ** 2 * (w * w + h * h)
        for q in (0, 1, bound - 1, bound):
            assert CT.simplify_numpy(c, q / 16.0).xy.tolist() == corners, (w, h, q)
        for q in (bound + 1, bound + 2, 16 * max(w, h), 2 ** 20):
            s = CT.simplify_numpy(c, q / 16.0)
            assert s.xy.tolist() == corners[:3] and s.index.tolist() == [0, 1, 2] and s.area.tolist() == [w * h], (w, h, q)


def test_the_single_pixel_becomes_a_triangle_at_one_pixel():
    c = one([[1]], 4, 6)
    assert CT.simplify_numpy(c, 11 / 16.0).xy.tolist() == [[4, 6], [5, 6], [5, 7], [4, 7]]        # 256 > 2 * 121
    assert CT.simplify_numpy(c, 1.0).xy.tolist() == [[4, 6], [5, 6], [5, 7]]                      # 256 <= 2 * 256


def test_the_staircase_triangle_becomes_the_triangle_at_q_12_and_keeps_a_fourth_vertex_at_q_11():
    """m[y, :y + 1] of side 12: the outer corners of the staircase lie 1 / sqrt(2) off the hypotenuse (N / D = 1 / 2), and
    256 > 2 * 121 but 256 <= 2 * 144."""
    x0, y0 = 5, 7
    c = one(np.tril(np.ones((12, 12), bool)), x0, y0)
    assert c.vert_ptr.tolist() == [0, 26]
    s = CT.simplify_numpy(c, 12 / 16.0)
    assert s.xy.tolist() == [[x0, y0], [x0 + 12, y0 + 12], [x0, y0 + 12]] and s.vert_ptr.tolist() == [0, 3] and s.area.tolist() == [78]
    assert len(CT.simplify_numpy(c, 11 / 16.0).xy) == 4


def test_the_loop_that_needs_128_bits():
    """(-2^24, 0), (0, 8), (2^24, 0), (0, -8): the off-axis vertices are 8 from the axis, N = (2^25 * 8)^2 = 2^56, D = 2^50:
    256 N = 2^64 = 128^2 D exactly.  At q = 128 both are dropped and the third anchor puts the first back; at q = 127 both stay."""
    c = SI.general("wide")
    assert SI.deviation(SI.WIDE[0], SI.WIDE[2], SI.WIDE[1]) == (2 ** 56, 2 ** 50)
    assert SI.general_reference("wide", 128).index.tolist() == [0, 1, 2]
    assert SI.general_reference("wide", 127).index.tolist() == [0, 1, 2, 3]
    assert CT.simplify_numpy(c, 0.0).index.tolist() == [0, 1, 2, 3]


def test_short_loops_are_unchanged_and_equal_vertices_come_out_as_three():
    c = SI.general("short")
    for q in (0, 16, 2 ** 20):
        s = SI.general_reference("short", q)
        assert s.vert_ptr.tolist() == [0, 0, 1, 3, 6, 9, 9, 13 if q == 0 else 12]      # (the 7 x 1 rectangle: 256 * 49 <= 256 * 50)
        assert s.index[:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8] and SI.same_array(s.xy, c.xy[s.index])


def test_the_comb_is_hundreds_of_splits_deep():
    """Every tooth is longer than the one after it, so a split takes off one tooth and leaves the rest to the next.  The depth is
    counted here by replaying the splits with their level (this says what the input is, not what the rule gives)."""
    c, s = SI.general("comb"), SI.general_reference("comb", 16)
    assert len(c.area) == 1 and c.area.tolist() == [600 * 601 // 2 + 600]
    pts, P, k = [tuple(v) for v in c.xy.tolist()], c.xy.astype(np.int64), len(c.xy)
    far = [(x - pts[0][0]) ** 2 + (y - pts[0][1]) ** 2 for x, y in pts[1:]]
    B = 1 + far.index(max(far))
    open_, deepest = [(0, B, 1), (B, k, 1)], 0
    while open_:
        i, j, level = open_.pop()
        if j - i >= 2:
            N, m, D = CT._best(pts, P, k, i, j)
            if 256 * N > 256 * D:
                deepest = max(deepest, level)
                open_ += [(i, m, level + 1), (m, j, level + 1)]
    assert deepest >= 300
    assert within_tolerance(c, s, 16) is None


# ---- the rasterised result ----

@pytest.mark.parametrize("connectivity", SI.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["holes", "seam", "lines", "many", "real"])
def test_the_rasterised_polygons_stay_within_the_tolerance_of_the_mask(name, connectivity):
    """masks_from_polygons_numpy of the simplified outer loops against fill_holes_numpy of the complementary connectivity: every
    differing pixel has chessboard distance at most ceil(epsilon) + 1 (the + 1: the rasteriser's half pixel) from a pixel of the
    other value in the original.  Every instance is moved into a frame of its own: its bounds grown by that distance on every
    side, at the least (the vertices of a simplified loop are vertices of the outline, so the polygons stay inside the bounds)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    pm = TI.get(name)
    want = CC.fill_holes_numpy(pm, OTHER[connectivity])
    rows = [i for i in range(len(pm)) if min(pm.size(i)) > 0]
    for q in SI.QS[1:]:
        s = SI.reference(name, connectivity, q)
        reach = int(math.ceil(q / 16.0)) + 1
        assert all(s.polygons(i) == [] for i in range(len(pm)) if i not in rows)
        # one call of the rasteriser for the set: every frame has the size of the largest
        H, W = max(pm.size(i)[0] for i in rows) + 2 * reach, max(pm.size(i)[1] for i in rows) + 2 * reach
        local = [[(np.array(poly).reshape(-1, 2) - (pm.bounds[i][:2] - reach)).reshape(-1).tolist() for poly in s.polygons(i)] for i in rows]
        back = PG.masks_from_polygons_numpy(local, H, W)
        for n, i in enumerate(rows):
            h, w = pm.size(i)
            got = back.full(n, H, W).astype(bool)
            mask = np.pad(want.dense(i), ((reach, H - h - reach), (reach, W - w - reach)))
            differ = got != mask
            if not differ.any():
                continue
            inside, outside = ndimage.distance_transform_cdt(mask, "chessboard"), ndimage.distance_transform_cdt(~mask, "chessboard")
            assert int(np.where(mask, inside, outside)[differ].max()) <= reach, (i, q)


# ---- what is refused ----

def gone(*args, **kw):
    """Stands in for the library: touching it fails the test."""
    raise AssertionError("the library was looked for")


@pytest.mark.parametrize("epsilon", [-0.5, -1e-9, float("nan"), float("inf"), (2 ** 20 + 1) / 16.0, 1e300])
def test_invalid_tolerances_raise_before_the_library_is_looked_for(monkeypatch, epsilon):
    monkeypatch.setattr(_lib, "call", gone)
    monkeypatch.setattr(_lib, "load", gone)
    c, pm = TI.reference("seam", 8), TI.get("seam")
    from transform import mask_transform as MT
    for call in (lambda: CT.simplify_numpy(c, epsilon), lambda: CT.simplify(c, epsilon), lambda: c.simplify(epsilon),
                 lambda: pm.polygons(8, epsilon=epsilon), lambda: CT.polygons(pm, epsilon=epsilon),
                 lambda: MT.mask_polygons(pm, epsilon=epsilon)):
        with pytest.raises(ValueError, match="epsilon="):
            call()


def test_the_largest_tolerance_and_loops_out_of_range():
    c = SI.general("short")
    assert len(CT.simplify_numpy(c, 2 ** 20 / 16.0).xy) == 12
    far = CT.Contours([0, 1], [0, 4], [0], [[0, 0], [2 ** 24 + 1, 0], [5, 5], [0, 5]])
    with pytest.raises(ValueError, match=r"simplify_numpy: a coordinate outside \[-16777216, 16777216\]"):
        CT.simplify_numpy(far, 1.0)
    with pytest.raises(ValueError, match="index has 3 entries for 4 vertices"):
        CT.SimplifiedContours([0, 1], [0, 4], [0], np.zeros((4, 2)), [0, 1, 2])


def test_n14_is_declared():
    decls = _lib.parse_header()
    assert decls["mnc_contours_simplify"][2] == ["vert_ptr", "xy", "n_loops", "n_verts", "q", "out_vert_ptr", "out_xy", "out_index",
                                                 "out_verts", "device_id"]
    assert decls["mnc_contours_simplify_timing"][2] == ["on", "last_ms"]
