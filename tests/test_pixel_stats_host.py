"""CPU: the numpy statements of mnc_amd.pixels (pixel_stats_numpy, histogram_numpy) and the host methods of their results, pinned to
facts that do not come from them: scipy.ndimage's sum, minimum, maximum, minimum_position, maximum_position and histogram with
PackedMasks.full(i, H, W) as the label, np.bincount, a constant image, the closed forms on moments_numpy for ramp images, np.var of
the selected pixels in float64, and every refusal.  The sets and images are those of tests/pixel_stats_inputs.py."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import pixel_stats_inputs as PI  # noqa: E402
from mnc_amd import pixels as PX  # noqa: E402
from mnc_amd import shape as SH  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402


def _live(pm, h=PI.H, w=PI.W):
    return [i for i in range(len(pm)) if pm.full(i, h, w).any()]


@pytest.mark.parametrize("set_name,image_name", [("word_edges", "uint8_c3"), ("image_edges", "int16_c4"), ("many130", "int32_c1"),
                                                 ("image_edges", "uint16_c5")])
def test_stats_equal_scipy_ndimage_on_the_full_mask(set_name, image_name):
    pm, im = PI.get(set_name), PI.image(image_name)
    st = PI.stats_ref(set_name, image_name)
    C = im.shape[2]
    assert st.count.dtype == np.int64 and st.sum.shape == (len(pm), C) and st.argmin.shape == (len(pm), C, 2)
    assert st.min.dtype == st.max.dtype == st.argmin.dtype == st.argmax.dtype == np.int32
    assert np.array_equal(st.count, PI.frame_counts(pm))
    live = _live(pm)
    assert 0 < len(live) and (set_name != "image_edges" or len(live) < len(pm))
    for i in range(len(pm)):
        label = pm.full(i, PI.H, PI.W)
        for c in range(C):
            plane = im[:, :, c].astype(np.int64)
            if i not in live:
                assert st.count[i] == 0 and st.sum[i, c] == st.sumsq[i, c] == st.sum_xv[i, c] == st.sum_yv[i, c] == 0
                assert st.min[i, c] == st.max[i, c] == 0 and tuple(st.argmin[i, c]) == tuple(st.argmax[i, c]) == (-1, -1)
                continue
            assert st.sum[i, c] == int(ndimage.sum(plane, label, 1)) and st.sumsq[i, c] == int(ndimage.sum(plane * plane, label, 1))
            assert st.min[i, c] == int(ndimage.minimum(plane, label, 1)) and st.max[i, c] == int(ndimage.maximum(plane, label, 1))
            y, x = ndimage.minimum_position(plane, label, 1)
            assert tuple(st.argmin[i, c]) == (x, y)
            y, x = ndimage.maximum_position(plane, label, 1)
            assert tuple(st.argmax[i, c]) == (x, y)
            yy, xx = np.mgrid[0:PI.H, 0:PI.W]
            assert st.sum_xv[i, c] == int(ndimage.sum(plane * xx, label, 1)) and st.sum_yv[i, c] == int(ndimage.sum(plane * yy, label, 1))
    # center_of_mass is (y, x); the weighted centroid is (x, y)
    i = live[0]
    com = ndimage.center_of_mass(im[:, :, 0].astype(np.float64), pm.full(i, PI.H, PI.W), 1)
    if st.sum[i, 0]:
        assert np.allclose(st.weighted_centroid()[i, 0], com[::-1], rtol=1e-9)


@pytest.mark.parametrize("case", sorted(PI.HISTOGRAMS))
def test_histograms_equal_bincount_and_scipy(case):
    im_name, bins, lo, shift = PI.HISTOGRAMS[case]
    im = PI.image(im_name)
    for set_name in ("word_edges", "image_edges"):
        pm, hs = PI.get(set_name), PI.hist_ref(set_name, case)
        C = im.shape[2] if im.ndim == 3 else 1
        assert hs.hist.shape == (len(pm), C, bins) and hs.hist.dtype == hs.count.dtype == np.int64
        assert (hs.lo, hs.shift, hs.bins) == (lo, shift, bins) and np.array_equal(hs.count, PI.frame_counts(pm))
        for i in range(len(pm)):
            label = pm.full(i, PI.H, PI.W)
            for c in range(C):
                v = im.reshape(PI.H, PI.W, C)[:, :, c][label].astype(np.int64)
                inside = v[(v >= lo) & (v < lo + (bins << shift))]
                assert np.array_equal(hs.hist[i, c], np.bincount((inside - lo) >> shift, minlength=bins))
                if label.any():
                    plane = im.reshape(PI.H, PI.W, C)[:, :, c].astype(np.float64)
                    upper = lo + (bins << shift)           # (scipy's last bin is closed above: the edge itself is taken out)
                    want = ndimage.histogram(plane, lo, upper, bins, label & (plane != upper), 1)
                    assert np.array_equal(hs.hist[i, c], want)
        if case in ("i16_negative_lo", "u8_dropped"):
            assert (hs.hist.sum(-1) <= hs.count[:, None]).all() and (hs.count >= 60).any()
            assert (hs.hist.sum(-1) < hs.count[:, None])[hs.count >= 60].all()           # (half the values or more lie outside)
        if case == "constant":
            assert np.array_equal(hs.hist[:, :, 7], np.broadcast_to(hs.count[:, None], (len(pm), C))) and hs.hist.sum() == 3 * hs.count.sum()


def test_constant_image_gives_v_times_count_and_the_first_pixel():
    for set_name in ("word_edges", "image_edges"):
        pm, st = PI.get(set_name), PI.stats_ref(set_name, "const_u8")
        assert np.array_equal(st.sum, 7 * np.broadcast_to(st.count[:, None], st.sum.shape))
        assert np.array_equal(st.sumsq, 49 * np.broadcast_to(st.count[:, None], st.sum.shape))
        for i in range(len(pm)):
            y, x = np.nonzero(pm.full(i, PI.H, PI.W))
            first = (int(x[0]), int(y[0])) if y.size else (-1, -1)
            for c in range(3):
                assert tuple(st.argmin[i, c]) == tuple(st.argmax[i, c]) == first
                assert st.min[i, c] == st.max[i, c] == (7 if y.size else 0)


def test_planted_ties_resolve_to_the_lowest_y_x():
    st = PI.stats_ref("ties", "ties")
    assert st.count[0] == PI.TIE_W * PI.TIE_H
    for c in range(3):
        x, y = PI.TIE_SPOTS[c]
        assert st.min[0, c] == 5 and tuple(st.argmin[0, c]) == (x, y)
        assert st.max[0, c] == 200 and tuple(st.argmax[0, c]) == ((x + 1) % PI.TIE_W, y)


def test_ramp_images_give_the_closed_forms_on_the_moments():
    pm = PI.get("inside")
    m = SH.moments_numpy(pm).m
    x1, y1 = pm.bounds[:, 0].astype(np.int64), pm.bounds[:, 1].astype(np.int64)
    m00, m10, m01, m20, m11, m02 = (m[:, k] for k in range(6))
    sx, sy = PI.stats_ref("inside", "ramp_x"), PI.stats_ref("inside", "ramp_y")
    assert np.array_equal(sx.count, m00) and np.array_equal(sx.count, pm.areas)
    assert np.array_equal(sx.sum[:, 0], m10 + x1 * m00) and np.array_equal(sx.sumsq[:, 0], m20 + 2 * x1 * m10 + x1 * x1 * m00)
    assert np.array_equal(sy.sum[:, 0], m01 + y1 * m00) and np.array_equal(sy.sumsq[:, 0], m02 + 2 * y1 * m01 + y1 * y1 * m00)
    assert np.array_equal(sx.sum_xv[:, 0], sx.sumsq[:, 0]) and np.array_equal(sy.sum_yv[:, 0], sy.sumsq[:, 0])
    assert np.array_equal(sx.sum_yv[:, 0], m11 + x1 * m01 + y1 * m10 + x1 * y1 * m00) and np.array_equal(sx.sum_yv, sy.sum_xv)
    assert np.allclose(sx.mean()[:, 0], SH.moments_numpy(pm).centroid()[:, 0], rtol=1e-12)


def test_var_near_the_top_of_the_range_where_a_naive_evaluation_fails():
    """300 x 300 pixels of 2^18 - {0, 1, 2}: count * sumsq is about 2^69, and float64 E[v^2] - E[v]^2 cancels to nothing."""
    rng = np.random.default_rng(2105)
    im = (PX.MAX_VALUE - rng.integers(0, 3, (300, 300))).astype(np.int32)
    pm = PI.get("big")
    st = PX.pixel_stats_numpy(pm, im)
    v = im.astype(np.float64).reshape(-1)
    want = np.var(v)
    assert 0.5 < want < 1.0
    assert abs(st.var()[0, 0] - want) <= 1e-9 * want and abs(st.std()[0, 0] - np.std(v)) <= 1e-9 * np.std(v)
    assert abs(st.var(ddof=1)[0, 0] - np.var(v, ddof=1)) <= 1e-9 * want
    assert abs(st.mean()[0, 0] - v.mean()) <= 1e-12 * v.mean()
    assert int(st.count[0]) * int(st.sumsq[0, 0]) > 2 ** 63                                # (does not fit int64)
    naive = float(st.sumsq[0, 0]) / float(st.count[0]) - (float(st.sum[0, 0]) / float(st.count[0])) ** 2
    assert abs(naive - want) > 1e-6 * want
    empty = PX.pixel_stats_numpy(PI.get("image_edges"), PI.image("uint8_c1"))
    assert np.isnan(empty.mean()[5, 0]) and np.isnan(empty.var()[8, 0]) and np.isnan(empty.weighted_centroid()[9, 0]).all()


def test_percentile_median_and_mode():
    hist = np.zeros((2, 1, 8), np.int64)
    hist[0, 0] = [0, 2, 0, 5, 5, 0, 1, 0]                      # 13 values
    h = PX.MaskHistograms(hist, np.array([13, 0]), -4, 2, 8)
    assert h.edge(3) == 8 and h.mode()[0, 0] == 8 and h.mode().dtype == np.int64            # the lowest of the two fullest bins
    assert h.percentile(0)[0, 0] == 0                          # at least one value: the first occupied bin, bin 1
    assert h.median()[0, 0] == 8                               # ceil(6.5) = 7 values: bins 1 and 3 hold 7
    assert h.percentile(54)[0, 0] == 12                        # ceil(7.02) = 8
    assert h.percentile(100)[0, 0] == 20
    assert h.percentile(50)[1, 0] == h.edge(8) == 28           # nothing counted
    st = PI.hist_ref("word_edges", "u8_256")
    pm, im = PI.get("word_edges"), PI.image("uint8_c3")
    v = np.sort(im[:, :, 1][pm.full(4, PI.H, PI.W)])
    assert st.median()[4, 1] == v[(len(v) + 1) // 2 - 1] and st.percentile(100)[4, 1] == v[-1] and st.percentile(0)[4, 1] == v[0]
    assert st.mode()[4, 1] == np.argmax(np.bincount(v))


def test_quantise():
    a = np.array([[0.5, -0.25], [1.0 / 3.0, 4.0]])
    q = PX.quantise(a)
    assert q.dtype == np.int32 and q.flags["C_CONTIGUOUS"] and np.array_equal(q, [[32768, -16384], [21845, 262144]])
    assert np.array_equal(PX.quantise(a, 0), [[0, 0], [0, 4]])                                   # (rint: halves to even)
    assert np.array_equal(PX.quantise(np.array([[2.5, 3.5]]), 0), [[2, 4]])
    for bad, bits in ((np.array([[4.00001]]), 16), (np.array([[-4.1]]), 16), (np.array([[np.nan]]), 16), (np.array([[np.inf]]), 0),
                      (a, 31), (a, -1)):
        with pytest.raises(ValueError):
            PX.quantise(bad, bits)
    PX.pixel_stats_numpy(PI.get("inside"), PX.quantise(np.random.default_rng(1).uniform(-4, 4, (PI.H, PI.W))))


def test_refusals():
    pm = PI.get("inside")
    good = PI.image("uint8_c3")
    for fn in (PX.pixel_stats_numpy, PX.histogram_numpy):
        for bad in (good.astype(np.float32), good.astype(np.int64), good.astype(np.uint32), good.astype(np.int8), good[0, :, 0],
                    good[None, None], np.zeros((PI.H, PI.W, 0), np.uint8), np.zeros((PI.H, PI.W, 33), np.uint8),
                    np.zeros((0, 5), np.uint8), np.broadcast_to(np.uint8(0), (32769, 4)), np.broadcast_to(np.uint8(0), (8193, 8193))):
            with pytest.raises(ValueError):
                fn(pm, bad)
        for v in (PX.MAX_VALUE + 1, -PX.MAX_VALUE - 1):
            im = np.zeros((PI.H, PI.W), np.int32)
            im[PI.H - 1, PI.W - 1] = v                       # (under no instance: the range is the image's)
            with pytest.raises(ValueError):
                fn(pm, im)
        fn(pm, np.full((PI.H, PI.W), PX.MAX_VALUE, np.int32))
        big = np.zeros((2049, 4), np.int32)
        big[:, 2:] = -1
        with pytest.raises(ValueError):
            fn(PackedMasks(big, np.zeros(2049, np.int64), np.zeros(2049, np.int64), None, None, np.zeros(0, np.uint64)), good)
        with pytest.raises(ValueError):
            fn(PackedMasks([[2 ** 24, 0, 2 ** 24 + 3, 4]], [0], [0], None, None, np.zeros(8, np.uint64)), good)
    for kw in ({"bins": 0}, {"bins": 4097}, {"shift": -1}, {"shift": 32}, {"lo": 2 ** 31}):
        with pytest.raises(ValueError):
            PX.histogram_numpy(pm, good, **kw)
    with pytest.raises(ValueError):
        PX.histogram_numpy(PI.get("many130"), np.zeros((PI.H, PI.W, 32), np.uint8), bins=4096)   # 130 * 32 * 4096 > 2^24
    # a [H, W] image is one channel; a non-contiguous one is taken as it reads
    two = PX.pixel_stats_numpy(pm, good[:, :, 1])
    assert PI.same_fields(two, PX.pixel_stats_numpy(pm, np.ascontiguousarray(good[:, :, 1:2])))
