"""The numpy statements of the surface distances (mnc_amd.surface: surface_numpy, surface_stats_numpy, surface_distances_numpy)
pinned to facts that do not come from them -- scipy.ndimage's erosion and Euclidean distance transform, a brute force over all
point pairs, scipy.spatial's directed Hausdorff distance, closed forms, and the dilation of mnc_amd.distance -- and the host
methods of the result classes.  No GPU: tests/test_gpu_surface_dist.py holds the kernels to these statements."""
import math
import os
import sys

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial.distance import directed_hausdorff

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import surface_dist_inputs as SI  # noqa: E402
from mnc_amd import distance as DS  # noqa: E402
from mnc_amd import surface as SF  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

CASES = ["word_edges", "sectors", "far", "empty_rows", "ring", "ties", "hollow"]


def _one(x1, y1, m):
    return SI._pack([(x1, y1, np.asarray(m, bool))])


def _frame(a, b):
    """The hull of all bounds with rows -> (x0, y0, H, W)."""
    boxes = [pm.bounds[i] for pm in (a, b) for i in range(len(pm)) if min(pm.size(i))]
    x0, y0 = min(int(q[0]) for q in boxes), min(int(q[1]) for q in boxes)
    return x0, y0, max(int(q[3]) for q in boxes) - y0 + 1, max(int(q[2]) for q in boxes) - x0 + 1


def _shifted(pm, x0, y0):
    return PackedMasks(pm.bounds - np.array([x0, y0, x0, y0], np.int32), pm.offsets, pm.areas, pm.classes, pm.scores, pm.bits)


# ---- the surface ----

@pytest.mark.parametrize("name", CASES + ["large", "many130"])
def test_surface_is_the_mask_less_its_erosion_by_the_cross(name):
    cross = ndimage.generate_binary_structure(2, 1)
    for pm in SI.get(name)[:2]:
        got = SF.surface_numpy(pm)
        assert np.array_equal(got.bounds, pm.bounds) and np.array_equal(got.classes, pm.classes) and np.array_equal(got.scores, pm.scores)
        at = 0
        for i in range(len(pm)):
            assert got.offsets[i] == at
            at += 8 * got.size(i)[0] * ((got.size(i)[1] + 63) // 64) if min(got.size(i)) else 0
            if not min(pm.size(i)):
                assert got.areas[i] == 0
                continue
            m = pm.dense(i)
            want = m ^ ndimage.binary_erosion(np.pad(m, 1), cross)[1:-1, 1:-1]
            assert np.array_equal(got.dense(i), want) and got.areas[i] == want.sum()
        assert got.bits.size * 8 == at


def test_a_solid_5x5_has_16_surface_pixels_and_its_centre_is_4_away():
    box = _one(0, 0, np.ones((5, 5)))
    s = SF.surface_numpy(box)
    assert s.areas[0] == 16 and not s.dense(0)[1:4, 1:4].any()
    d = SF.surface_distances_numpy(_one(2, 2, [[1]]), box)
    assert d.slot(0, 0).tolist() == [4] and d.slot(0, 1).max() == 8 and d.slot(0, 1).min() == 4
    st = SF.surface_stats_numpy(_one(2, 2, [[1]]), box, tau2=[3, 4])
    assert st.within[0, 0].tolist() == [0, 1] and st.count.tolist() == [[1, 16]]


# ---- the distances ----

@pytest.mark.parametrize("name", CASES)
def test_d2_is_the_offset_to_the_nearest_surface_pixel_of_the_distance_transform(name):
    a, b, pairs = SI.get(name)
    x0, y0, H, W = _frame(a, b)
    sa, sb = _shifted(SF.surface_numpy(a), x0, y0), _shifted(SF.surface_numpy(b), x0, y0)
    got = SI.dist_ref(name)
    pairs = SF._check_pairs("test", a, b, pairs)
    edt = {}
    for k, (i, j) in enumerate(pairs.tolist()):
        for d, (src, s, dst, t) in enumerate(((sa, i, sb, j), (sb, j, sa, i))):
            key = (d, t)                                              # the nearest surface pixel of dst[t], for every pixel of the frame
            if key not in edt:
                full_dst = dst.full(t, H, W)
                edt[key] = ndimage.distance_transform_edt(~full_dst, return_indices=True)[1] if full_dst.any() else None
            ys, xs = np.nonzero(src.full(s, H, W))
            mine = got.slot(k, d)
            assert mine.dtype == np.uint32 and len(mine) == len(ys)
            if edt[key] is None:
                assert (mine == SF.NONE).all()
                continue
            ny, nx = edt[key][0][ys, xs], edt[key][1][ys, xs]
            assert np.array_equal(mine, (ny - ys) ** 2 + (nx - xs) ** 2)


@pytest.mark.parametrize("name", ["sectors", "far", "empty_rows", "ring", "ties", "hollow"])
def test_d2_is_the_brute_force_and_its_maximum_is_the_directed_hausdorff_distance(name):
    a, b, pairs = SI.get(name)
    got, st = SI.dist_ref(name), SI.stats_ref(name)
    pairs = SF._check_pairs("test", a, b, pairs)
    for k, (i, j) in enumerate(pairs.tolist()):
        pa, pb = np.stack(SF.surface_points(a, i), 1), np.stack(SF.surface_points(b, j), 1)
        for d, (src, dst) in enumerate(((pa, pb), (pb, pa))):
            assert st.count[k, d] == len(src)
            if not len(src) or not len(dst):
                assert st.max_d2[k, d] == -1 and (st.argmax[k, d] == -1).all() and st.sum_d2[k, d] == 0 and not st.within[k, d].any()
                assert (got.slot(k, d) == SF.NONE).all() and len(got.slot(k, d)) == len(src)
                continue
            want = np.array([min((int(p[0]) - int(q[0])) ** 2 + (int(p[1]) - int(q[1])) ** 2 for q in dst) for p in src])
            assert np.array_equal(got.slot(k, d), want)
            assert st.max_d2[k, d] == want.max() and st.sum_d2[k, d] == want.sum()
            assert tuple(st.argmax[k, d]) == tuple(src[int(np.argmax(want))])            # raster order: the lowest (y, x)
            assert math.isclose(directed_hausdorff(src, dst)[0], math.sqrt(st.max_d2[k, d]), rel_tol=1e-12)
            assert st.within[k, d].tolist() == [int((want <= t).sum()) for t in SI.TAU2]


def test_single_pixels_give_dx2_plus_dy2_also_at_the_ends_of_the_span():
    one = [[1]]
    for (ax, ay), (bx, by) in [((0, 0), (3, 4)), ((-7, 9), (5, -2)), ((4, 4), (4, 4))]:
        st = SF.surface_stats_numpy(_one(ax, ay, one), _one(bx, by, one))
        want = (ax - bx) ** 2 + (ay - by) ** 2
        assert st.max_d2.tolist() == [[want, want]] and st.sum_d2.tolist() == [[want, want]]
        assert st.argmax.tolist() == [[[ax, ay], [bx, by]]]
    a, b = SI.extreme_sets(16000)
    assert SF.surface_stats_numpy(a, b).max_d2.tolist() == [[2 * 32000 ** 2] * 2]
    a, b = SI.extreme_sets(16383)                                       # a span of 32767 pixels: the largest permitted
    far = SF.surface_distances_numpy(a, b)
    assert far.d2.tolist() == [2 * 32766 ** 2] * 2 and 2 * 32766 ** 2 < 2 ** 31


def test_a_rectangle_against_its_translate():
    """An h x w outline moved by (tx, 0) with 0 < tx < w: a pixel of the left side is tx from the translate's left side unless the
    top or bottom edge of the translate passes nearer; the pixels of the top edge from column tx on lie on the translate's."""
    h, w, tx = 9, 20, 6
    box = np.ones((h, w), bool)
    st = SF.surface_stats_numpy(_one(0, 0, box), _one(tx, 0, box), tau2=[0])
    assert st.count.tolist() == [[2 * (h + w) - 4] * 2]
    assert st.max_d2.tolist() == [[tx * tx, tx * tx]]
    assert st.argmax.tolist() == [[[0, 0], [w + tx - 1, 0]]]             # the first of the ties in raster order
    assert st.within[0, :, 0].tolist() == [2 * (w - tx)] * 2             # the parts of the top and bottom edges both outlines share
    d = SF.surface_distances_numpy(_one(0, 0, box), _one(tx, 0, box))
    assert d.slot(0, 0)[:w].tolist() == [(tx - x) ** 2 for x in range(tx)] + [0] * (w - tx)       # the top edge, raster order


@pytest.mark.parametrize("name", ["word_edges", "empty_rows", "many130"])
def test_a_set_against_itself_is_all_zeros(name):
    a = SI.get(name)[0]
    pairs = np.stack([np.arange(len(a))] * 2, 1).astype(np.int32)
    st = SF.surface_stats_numpy(a, a, pairs, [0])
    assert not st.max_d2.any() and not st.sum_d2.any() and np.array_equal(st.within[:, :, 0], st.count) and st.count.all()
    assert not SF.surface_distances_numpy(a, a, pairs).d2.any()


@pytest.mark.parametrize("name", ["word_edges", "empty_rows", "ring", "hollow"])
def test_within_is_the_area_of_the_surface_inside_the_dilated_other_surface(name):
    a, b, pairs = SI.get(name)
    st = SI.stats_ref(name)
    x0, y0, H, W = _frame(a, b)
    sa, sb = _shifted(SF.surface_numpy(a), x0, y0), _shifted(SF.surface_numpy(b), x0, y0)
    for k, (i, j) in enumerate(SF._check_pairs("test", a, b, pairs).tolist()[:24]):
        for t, r2 in enumerate(SI.TAU2[:5]):
            rho = math.isqrt(r2)
            grown = DS.dilate_numpy(sb.full(j, H, W), r2)[rho:rho + H, rho:rho + W]
            assert st.within[k, 0, t] == (sa.full(i, H, W) & grown).sum()


# ---- the host methods ----

def test_hausdorff_f_measure_and_surface_dice_on_the_integers():
    a, b, _ = SI.get("hollow")
    st = SF.surface_stats_numpy(a, b, None, [4])
    hd, f, nsd = st.hausdorff(), st.boundary_f(0), st.nsd(0)
    for k, (i, j) in enumerate(np.ndindex(len(a), len(b))):
        ea, eb = st.count[k, 0] == 0, st.count[k, 1] == 0
        if ea and eb:
            assert math.isnan(hd[k]) and f[k] == 1.0 and math.isnan(nsd[k]) and st.precision(0)[k] == 1.0 and st.recall(0)[k] == 1.0
        elif ea or eb:
            assert math.isinf(hd[k]) and f[k] == 0.0 and nsd[k] == 0.0
            assert (st.precision(0)[k], st.recall(0)[k]) == ((1.0, 0.0) if ea else (0.0, 1.0))
        else:
            p, r = st.within[k, 0, 0] / st.count[k, 0], st.within[k, 1, 0] / st.count[k, 1]
            assert hd[k] == math.sqrt(st.max_d2[k].max()) and st.precision(0)[k] == p and st.recall(0)[k] == r
            assert f[k] == (2 * p * r / (p + r) if p + r else 0.0)
            assert nsd[k] == st.within[k, :, 0].sum() / st.count[k].sum()
    assert (st.count == 0).all(1).any() and ((st.count == 0).sum(1) == 1).any() and (st.count > 0).all(1).any()
    with pytest.raises(ValueError):
        st.nsd(1)


def test_hd95_and_assd_are_the_percentile_and_the_mean_of_the_roots_of_both_directions():
    a, b, _ = SI.get("empty_rows")
    d = SF.surface_distances_numpy(a, b)
    for k in range(len(a)):
        roots = np.sqrt(np.concatenate([d.slot(k, 0), d.slot(k, 1)]).astype(np.float64))
        assert d.hd95()[k] == np.percentile(roots, 95) and d.percentile(50)[k] == np.percentile(roots, 50)
        assert d.assd()[k] == math.fsum(roots) / len(roots)
    h = SF.surface_distances_numpy(*SI.get("hollow")[:2])
    assert np.isnan(h.hd95()).any() and np.isinf(h.hd95()).any() and np.isfinite(h.assd()).any()


def test_tolerance_sq_is_davis_bound():
    assert SF.tolerance_sq(480, 854) == 64 and SF.tolerance_sq(375, 500, 0.008) == 25 and SF.tolerance_sq(600, 1000) == 100
    assert SF.tolerance_sq(10, 10, 3) == 9 and SF.tolerance_sq(10, 10, 0) == 0
    with pytest.raises(ValueError):
        SF.tolerance_sq(0, 10)


# ---- the refusals ----

def test_refusals_raise_value_error_without_a_device():
    a, b = SI.sectors_sets()
    one = np.ones((1, 1), bool)
    for f in (SF.surface_stats_numpy, SF.surface_distances_numpy, SF.surface_stats, SF.surface_distances):
        for pairs in ([[0, 1]], [[9, 0]], [[-1, 0]], np.zeros((2, 3), np.int32), np.zeros((65537, 2), np.int32), [[0.5, 0]]):
            with pytest.raises(ValueError):
                f(a, b, pairs)
    for f in (SF.surface_stats_numpy, SF.surface_stats):
        for tau in ([-1], [2 ** 31], list(range(9))):
            with pytest.raises(ValueError):
                f(a, b, None, tau)
    far = PackedMasks([[2 ** 24, 0, 2 ** 24 + 3, 4]], [0], [0], None, None, np.zeros(8, np.uint64))
    wide_a, wide_b = SI.extreme_sets(16384)                              # a span of 32769 pixels
    edge_a, edge_b = SI._pack([(-16384, 0, one)]), SI._pack([(16383, 0, one)])        # 32768: one past the limit
    tall = SI._pack([(0, 0, one), (0, 32767, one)])
    many = PackedMasks(np.zeros((2049, 4), np.int32) + [0, 0, -1, -1], np.zeros(2049, np.int64), np.zeros(2049, np.int64), None, None,
                       np.zeros(0, np.uint64))
    for x, y in ((far, b), (a, far), (wide_a, wide_b), (edge_a, edge_b), (tall, b), (many, b)):
        with pytest.raises(ValueError):
            SF.surface_stats_numpy(x, y, [[0, 0]])
        with pytest.raises(ValueError):
            SF.surface_distances_numpy(x, y, [[0, 0]])
    for pm in (far, tall, many):
        with pytest.raises(ValueError):
            SF.surface_numpy(pm)
    with pytest.raises(ValueError):
        SF.surface_stats_numpy(SI.many_set(), SI.many_set(505))            # 130 x 505 pairs
    assert SF.surface_stats_numpy(*SI.extreme_sets(16383)).max_d2[0, 0] == 2 * 32766 ** 2


# ---- the tool ----

def _eval_coco(argv):
    import io
    from contextlib import redirect_stdout
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import eval_coco
    out = io.StringIO()
    with redirect_stdout(out):
        ev = eval_coco.main(argv)
    return ev, out.getvalue().splitlines()


def test_eval_coco_surface_adds_four_lines_and_leaves_the_twelve_alone(tmp_path):
    import json
    import mask_boundary_inputs as BI
    gt_path, dt_path, sets = BI.coco_files(tmp_path)
    plain, lines = _eval_coco(["--gt", gt_path, "--dt", dt_path, "--cpu", "--out", str(tmp_path / "plain.json")])
    ev, more = _eval_coco(["--gt", gt_path, "--dt", dt_path, "--cpu", "--surface", "--out", str(tmp_path / "surface.json")])
    assert len(lines) == 12 and more[:12] == lines and len(more) == 16 and plain.surface is None
    with open(str(tmp_path / "plain.json")) as f:
        assert "surface" not in json.load(f)
    with open(str(tmp_path / "surface.json")) as f:
        s = json.load(f)["surface"]
    assert s == ev.surface and s["ratio"] == 0.008 and s["pairs"] > 10
    # the same figures from the matches and the statements, pair by pair
    hd, f = [], []
    for c, H, W, _ in sets.values():
        from mnc_amd.coco_eval import match_numpy
        m = match_numpy(c.dt, c.gt, c.kw["iscrowd"], c.kw["ignore"])
        g = m.dt_match[0, 0]
        pairs = np.array([[d, g[d]] for d in range(len(g)) if g[d] >= 0 and not c.kw["iscrowd"][g[d]]], np.int32)
        st = SF.surface_stats_numpy(c.dt, c.gt, pairs, [SF.tolerance_sq(H, W)])
        hd += st.hausdorff().tolist()
        f += st.boundary_f(0).tolist()
    assert s["pairs"] == len(hd) and s["hausdorff"] == float(np.mean(hd)) and s["boundary_f"] == float(np.mean(f))
    assert s["hausdorff"] >= s["hd95"] >= s["assd"] > 0.0 and 0.0 < s["boundary_f"] <= 1.0
    wide, _ = _eval_coco(["--gt", gt_path, "--dt", dt_path, "--cpu", "--surface", "0.05"])
    assert wide.surface["boundary_f"] > s["boundary_f"] and wide.surface["hausdorff"] == s["hausdorff"]


def test_the_pixel_and_entry_limits_of_a_call_are_refused_before_any_distance_is_made():
    """Three bounds of 8192 x 8191 pixels over one block of zero words are 1.5 x 2^27 pixels of rows, two are within the limit;
    65536 pairs of one instance of about 4000 surface pixels with itself are more than 2^28 distances."""
    words = np.zeros(8191 * 128, np.uint64)
    sets = {k: PackedMasks([[0, 0, 8191, 8190]] * k, [0] * k, [0] * k, None, None, words) for k in (1, 2, 3)}
    b = SI.sectors_sets()[1]
    assert 2 * 8192 * 8191 <= SF.MAX_PIXELS < 3 * 8192 * 8191 and 8192 * 8191 <= 2 ** 26
    SF._check_sets("test", [("a", sets[2]), ("b", b)])
    for x, y in ((sets[3], b), (b, sets[3]), (sets[2], sets[1])):
        with pytest.raises(ValueError, match="pixels of rows"):
            SF.surface_stats_numpy(x, y, [[0, 0]])
        with pytest.raises(ValueError, match="pixels of rows"):
            SF.surface_distances_numpy(x, y, [[0, 0]])
    with pytest.raises(ValueError, match="pixels of rows"):
        SF.surface_numpy(sets[3])
    a = SI._pack([(0, 0, SI._random(np.random.default_rng(2206), 65, 129))])
    count = int(SF.surface_numpy(a).areas[0])
    pairs = np.zeros((65536, 2), np.int32)
    assert 2 * len(pairs) * count > SF.MAX_ENTRIES
    with pytest.raises(ValueError, match="distances"):
        SF.surface_distances_numpy(a, a, pairs)
