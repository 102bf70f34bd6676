"""The numpy statements of mnc_amd/distance.py (distance_numpy, inscribed_numpy, morph_numpy) -- which tests/test_gpu_mask_distance.py
holds csrc/mask_distance.hip to, exactly -- pinned to facts that do not come from them: scipy.ndimage's Euclidean distance transform
and binary morphology, a brute-force minimum over all unset pixels, the closed form on full rectangles, the algebra of opening and
closing, and the 3 x 3 erosion of mnc_amd.boundary.  No GPU.  Also the input conditions of the GPU test's word-boundary set (stated
of the statement alone), radius_sq, the argument errors, and the numpy path of tools/demo.py --smooth-radius."""
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import mask_distance_inputs as DI  # noqa: E402
from mnc_amd import boundary  # noqa: E402
from mnc_amd import distance as DT  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

BI, MI = DI.BI, DI.MI


def one(m, x=0, y=0, dirty=True):
    m = np.asarray(m, bool)
    h, w = m.shape
    return MI.pack([[x, y, x + w - 1, y + h - 1]], [m], dirty=dirty)


def blobs(seed, count, lo=1, hi=70):
    rng = np.random.default_rng(seed)
    return [BI.blob(rng, int(rng.integers(lo, hi)), int(rng.integers(lo, 2 * hi))) for _ in range(count)]


# ---- the inside distance ----

def test_distance_equals_the_squared_scipy_edt_of_the_padded_mask():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name in ("word", "bounds", "tall"):
        pm, maps = DI.get(name), DI.reference(name, "distance")
        assert maps.sq.dtype == np.uint32 and maps.dist_ptr.dtype == np.int64 and len(maps.dist_ptr) == len(pm) + 1
        for i in range(len(pm)):
            h, w = pm.size(i)
            if not (h and w):
                assert maps.dist_ptr[i + 1] == maps.dist_ptr[i]
                continue
            d = ndimage.distance_transform_edt(np.pad(pm.dense(i), 1))[1:-1, 1:-1]
            assert np.array_equal(maps.map(i), np.rint(d * d).astype(np.uint32)), (name, i)


def test_distance_equals_the_brute_force_minimum():
    for m in blobs(11, 12, 1, 14):
        h, w = m.shape
        p = np.pad(m, max(h, w))                                   # every unset pixel that can be the nearest
        qy, qx = np.nonzero(~p)
        want = np.zeros((h, w), np.int64)
        for y, x in zip(*np.nonzero(m)):
            want[y, x] = ((qy - (y + max(h, w))) ** 2 + (qx - (x + max(h, w))) ** 2).min()
        assert np.array_equal(DT.distance_numpy(one(m, -3, 4)).map(0), want.astype(np.uint32))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (2, 2), (7, 64), (33, 65), (40, 9), (260, 600)])
def test_full_rectangles_have_the_closed_form(h, w):
    pm = one(np.ones((h, w), bool), 5, -7)
    yy, xx = np.mgrid[0:h, 0:w]
    want = np.minimum(np.minimum(xx + 1, w - xx), np.minimum(yy + 1, h - yy)) ** 2
    assert np.array_equal(DT.distance_numpy(pm).map(0), want.astype(np.uint32))
    # the inscribed disc: r2 = ((min(h, w) + 1) // 2)^2 at the first such pixel in raster order
    r = (min(h, w) + 1) // 2
    xy, r2 = DT.inscribed_numpy(pm)
    assert xy.dtype == np.int32 and r2.dtype == np.int32 and r2.tolist() == [r * r]
    assert xy.tolist() == [[5 + r - 1, -7 + r - 1]]


def test_inscribed_of_nothing():
    pm = MI.pack([[3, 3, 2, 9], [0, 0, 9, 4], [4, 4, 4, 4]], [np.zeros((7, 0), bool), np.zeros((5, 10), bool), np.ones((1, 1), bool)])
    xy, r2 = DT.inscribed_numpy(pm)
    assert xy.tolist() == [[-1, -1], [-1, -1], [4, 4]] and r2.tolist() == [0, 0, 1]
    assert DT.distance_numpy(pm).dist_ptr.tolist() == [0, 0, 50, 51]


# ---- the morphology ----

@pytest.mark.parametrize("r2", DI.HOST_R2S)
def test_erode_and_dilate_equal_scipys_with_the_disc(r2):
    ndimage = pytest.importorskip("scipy.ndimage")
    s, rho = DI.disc(r2)
    assert rho == math.isqrt(r2)
    masks = blobs(21 + r2, 6) if r2 < 100 else blobs(21 + r2, 1, 8, 9)       # (scipy's 129 x 129 element is slow)
    pm = DI._place(masks, dirty=True, x0=-20)
    er, di = DT.morph_numpy(pm, "erode", r2), DT.morph_numpy(pm, "dilate", r2)
    for i, m in enumerate(masks):
        h, w = m.shape
        p = np.pad(m, rho)
        assert np.array_equal(er.dense(i), ndimage.binary_erosion(p, s, border_value=0)[rho:rho + h, rho:rho + w]), i
        assert np.array_equal(di.dense(i), ndimage.binary_dilation(p, s, border_value=0)), i
        assert di.bounds[i].tolist() == (pm.bounds[i] + [-rho, -rho, rho, rho]).tolist()
    assert np.array_equal(er.bounds, pm.bounds) and np.array_equal(er.offsets, pm.offsets)
    assert er.areas.tolist() == [int(er.dense(i).sum()) for i in range(len(pm))]


@pytest.mark.parametrize("r2", DI.HOST_R2S[:-1])
def test_opening_and_closing_algebra(r2):
    pm = DI._place(blobs(41 + r2, 6), dirty=True)
    op, cl = DT.morph_numpy(pm, "open", r2), DT.morph_numpy(pm, "close", r2)
    assert np.array_equal(op.bounds, pm.bounds) and np.array_equal(cl.bounds, pm.bounds)           # neither leaves the bounds
    assert np.array_equal(op.offsets, pm.offsets) and np.array_equal(cl.offsets, pm.offsets)
    for i in range(len(pm)):
        m, o, c = pm.dense(i), op.dense(i), cl.dense(i)
        assert (o <= m).all() and (m <= c).all(), i                # anti-extensive, extensive
    assert DI.same_masks(DT.morph_numpy(op, "open", r2), op) and DI.same_masks(DT.morph_numpy(cl, "close", r2), cl)    # idempotent
    # the closing is the true one of the infinite lattice cut to the bounds: a wider frame changes nothing
    for i in range(len(pm)):
        rho = math.isqrt(r2)
        wide = DT.close_numpy(np.pad(pm.dense(i), rho + 2), r2)
        assert not wide[:rho + 2].any() and not wide[:, :rho + 2].any() and not wide[-rho - 2:].any() and not wide[:, -rho - 2:].any()
        assert np.array_equal(wide[rho + 2:-rho - 2, rho + 2:-rho - 2], cl.dense(i))


def test_closing_does_not_eat_an_object_at_the_frames_edge():
    m = np.ones((9, 9), bool)
    assert DT.close_numpy(m, 9).all() and DT.morph_numpy(one(m), "close", 9).areas.tolist() == [81]


def test_the_3x3_erosion_is_the_boundary_at_d_1():
    H, W = 90, 500
    pm = DI._place(blobs(61, 8, 3, 40), dirty=True)
    assert pm.bounds.min() >= 0 and pm.bounds[:, 2].max() < W and pm.bounds[:, 3].max() < H
    er = DT.morph_numpy(pm, "erode", 2)
    band = PackedMasks.from_dense(pm.bounds, [pm.dense(i) & ~er.dense(i) for i in range(len(pm))], pm.classes, pm.scores)
    assert DI.same_masks(band, boundary.boundary_numpy(pm, H, W, 1))


def test_dilate_clipped_to_an_image():
    pm = DI.get("bounds")
    H, W = DI.BOUNDS_H, DI.BOUNDS_W
    free, cut = DT.morph_numpy(pm, "dilate", 25), DT.morph_numpy(pm, "dilate", 25, H, W)
    grown = pm.bounds + np.array([-5, -5, 5, 5], np.int32)
    rows = (pm.bounds[:, 2] >= pm.bounds[:, 0]) & (pm.bounds[:, 3] >= pm.bounds[:, 1])
    assert np.array_equal(free.bounds[rows], grown[rows]) and np.array_equal(free.bounds[~rows], pm.bounds[~rows])
    want = boundary.clipped_bounds(grown, H, W)
    want[~rows] = (0, 0, -1, -1)
    assert np.array_equal(cut.bounds, want) and (cut.bounds[[6, 9, 10]] == (0, 0, -1, -1)).all()
    for i in range(len(pm)):
        assert np.array_equal(cut.full(i, H, W), free.full(i, H, W)), i
    assert cut.offsets.tolist() == np.concatenate(([0], np.cumsum([8 * ((max(b[2] - b[0] + 1, 0) + 63) // 64) * max(b[3] - b[1] + 1, 0)
                                                                   for b in cut.bounds.tolist()])))[:-1].tolist()


# ---- the input conditions of the GPU test ----

@pytest.mark.parametrize("r2", DI.R2S)
def test_the_word_boundary_set_can_fail(r2):
    pm = DI.get("word")
    assert len(pm) == 3 * len(DI.WIDTHS) * len(DI.HEIGHTS)
    assert (DI.reference("word", "erode", r2, None, None).areas > 0).sum() * 4 >= len(pm)
    assert (DI.reference("word", "open", r2, None, None).areas != pm.areas).sum() * 4 >= len(pm) or r2 == 0
    if r2 == 0:                                                    # the disc of one pixel: erode, open and close are the identity
        for op in ("erode", "open", "close"):
            assert np.array_equal(DI.reference("word", op, 0, None, None).bits, pm.bits)


def test_the_reach_set_meets_the_unaligned_shift():
    pm = DI.get("reach")
    assert sorted(math.isqrt(r) % 64 for r in DI.WORD_R2S) == [0, 1, 63] and ((pm.bounds[:, 2] - pm.bounds[:, 0]) >= 128).all()


# ---- arguments ----

def test_radius_sq():
    assert [DT.radius_sq(r) for r in (0, 1, 1.5, 2, 2.5, 23, 1024)] == [0, 1, 2, 4, 6, 529, 1024 * 1024]
    assert math.sqrt(3) ** 2 < 3 and DT.radius_sq(math.sqrt(3)) == 2          # what the docstring warns of
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            DT.radius_sq(bad)


def test_argument_errors():
    pm = one(np.ones((4, 4), bool))
    for args in (("shrink", 1), (4, 1), (-1, 1), ("erode", -1), ("erode", 1024 * 1024 + 1), ("dilate", 1, 5, None), ("dilate", 1, None, 5),
                 ("dilate", 1, 0, 5), ("dilate", 1, 5, 32769)):
        with pytest.raises(ValueError):
            DT.morph_numpy(pm, *args)
    for kw in ({}, {"radius": 1, "r2": 1}, {"r2": -1}, {"radius": -1.0}, {"r2": 1, "H": 5}):
        with pytest.raises(ValueError):
            DT.morph(pm, "erode", **kw)
    edge = MI.pack([[2 ** 24 - 12, 0, 2 ** 24 - 3, 4]], [np.ones((5, 10), bool)])
    assert DT.morph_numpy(edge, "dilate", 4).bounds.tolist() == [[2 ** 24 - 14, -2, 2 ** 24 - 1, 6]]
    for op in ("dilate", "close"):
        with pytest.raises(ValueError):
            DT.morph_numpy(edge, op, 9)
    assert DT.morph_numpy(edge, "open", 9).areas.tolist() == [0]
    big = np.zeros((2049, 4), np.int32)
    big[:, 2:] = -1
    many = PackedMasks(big, np.zeros(2049, np.int64), np.zeros(2049, np.int64), None, None, np.zeros(0, np.uint64))
    for fn in (DT.distance_numpy, DT.inscribed_numpy, lambda p: DT.morph_numpy(p, "erode", 1)):
        with pytest.raises(ValueError):
            fn(many)
    wide = PackedMasks(np.array([[0, 0, 8190, 8190]], np.int32), [0], [0], None, None, np.zeros(0, np.uint64))   # the bounds alone
    with pytest.raises(ValueError):
        DT._check_set("dilate", wide, 1)
    DT._check_set("erode", wide, 0)


def test_demo_smooth_radius_on_the_numpy_statement():
    import demo
    args = demo.parse_args(["--smooth-radius", "2", "--cpu"])
    assert args.smooth_radius == 2.0 and demo.parse_args([]).smooth_radius == 0.0
    pm = DI.get("many65")
    want = DT.morph_numpy(DT.morph_numpy(pm, "open", 4), "close", 4)
    assert DI.same_masks(demo._smooth(pm, 2, cpu=True), want) and (want.areas != pm.areas).any()
