"""Pixel statistics and histograms of an image under packed instance masks on the GPU (csrc/mask_pixels.hip: mnc_mask_pixel_stats,
mnc_mask_histogram and the Python surfaces over them) against the numpy statements (mnc_amd.pixels.pixel_stats_numpy and
histogram_numpy, which tests/test_pixel_stats_host.py pins to scipy.ndimage, np.bincount and closed forms).  Every comparison is
exact, field by field, dtype and shape included, and every device call is made twice: the bytes are equal.  The sets and images are
those of tests/pixel_stats_inputs.py: the smallest at which a kernel can go wrong."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import pixel_stats_inputs as PI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import pixels as PX  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY32 = 0x55555555
CANARY64 = 0x5555555555555555


def _bytes(t):
    return [a.tobytes() if isinstance(a, np.ndarray) else a for a in t]


def _stats(pm, im, want):
    """pixel_stats twice, against the statement's result."""
    first = PX.pixel_stats(pm, im)
    assert PI.same_fields(first, want)
    assert _bytes(PX.pixel_stats(pm, im)) == _bytes(first)
    return first


def _hist(pm, im, want):
    first = PX.histogram(pm, im, want.bins, want.lo, want.shift)
    assert PI.same_fields(first, want)
    assert _bytes(PX.histogram(pm, im, want.bins, want.lo, want.shift)) == _bytes(first)
    return first


# ---- word edges ----

@pytest.mark.parametrize("dtype", [np.dtype(d).name for d in PI.DTYPES])
def test_word_edge_widths_heights_and_starts_with_dirty_padding(dtype):
    """Widths 1, 63, 64, 65, 127, 128, 129 by heights 1, 2, 65 at x1 = 0, 1, 63 modulo 64 on the 67 x 131 image, C = 1, 3, 4, 5:
    every channel tile alone and the tile of 4 with a rest."""
    pm = PI.get("word_edges")
    w, h = pm.bounds[:, 2] - pm.bounds[:, 0] + 1, pm.bounds[:, 3] - pm.bounds[:, 1] + 1
    assert set(w.tolist()) == set(PI.WIDTHS) and set(h.tolist()) == set(PI.HEIGHTS) and set((pm.bounds[:, 0] % 64).tolist()) == set(PI.STARTS)
    clean = PI.word_edges_set(dirty=False)
    assert not np.array_equal(clean.bits, pm.bits)                     # the padding bits of the set are ones
    for C in PI.CHANNELS:
        name = "%s_c%d" % (dtype, C)
        got = _stats(pm, PI.image(name), PI.stats_ref("word_edges", name))
        assert _bytes(PX.pixel_stats(clean, PI.image(name))) == _bytes(got)
    assert np.array_equal(got.count, PI.frame_counts(pm)) and (got.count < pm.areas).any()      # (some hang over the right edge)


def test_a_two_dimensional_image_is_one_channel_and_the_methods_and_wrappers_agree():
    pm, im = PI.get("word_edges"), PI.image("uint8_c3")
    plane = np.ascontiguousarray(im[:, :, 2])
    want = PX.pixel_stats_numpy(pm, plane)
    assert want.sum.shape == (len(pm), 1)
    _stats(pm, plane, want)
    assert PI.same_fields(PX.pixel_stats(pm, im[:, :, 2]), want)                               # (a strided view)
    assert PI.same_fields(pm.pixel_stats(im), PI.stats_ref("word_edges", "uint8_c3"))
    assert PI.same_fields(MT.mask_pixel_stats(pm, im), PI.stats_ref("word_edges", "uint8_c3"))
    assert PI.same_fields(pm.histogram(im, 16, 0, 4), PI.hist_ref("word_edges", "u8_shift4"))
    assert PI.same_fields(MT.mask_histogram(pm, im, 16, 0, 4), PI.hist_ref("word_edges", "u8_shift4"))


# ---- image edges ----

@pytest.mark.parametrize("image_name", ["uint8_c3", "int16_c4", "int32_c5", "uint16_c1"])
def test_instances_over_the_edges_outside_without_rows_and_without_bits(image_name):
    pm = PI.get("image_edges")
    got = _stats(pm, PI.image(image_name), PI.stats_ref("image_edges", image_name))
    counts = PI.frame_counts(pm)
    assert np.array_equal(got.count, counts) and (counts[[0, 1, 2, 3, 4, 10, 11]] > 0).all()
    assert (counts[[0, 1, 2, 3, 4, 10]] < pm.areas[[0, 1, 2, 3, 4, 10]]).all() and counts[11] == 1
    for i in (5, 6, 7, 8, 9):                                          # outside (right, below, left), no rows, no bit
        assert got.count[i] == 0 and not got.sum[i].any() and not got.sumsq[i].any() and not got.sum_xv[i].any()
        assert not got.min[i].any() and not got.max[i].any() and (got.argmin[i] == -1).all() and (got.argmax[i] == -1).all()
    assert _bytes(PX.pixel_stats(PI.image_edges_set(dirty=False), PI.image(image_name))) == _bytes(got)


def test_sets_without_a_pixel_in_the_image_and_no_instance():
    im = PI.image("uint8_c3")
    out = PI.get("image_edges").take([5, 6, 7, 8])
    got = _stats(out, im, PX.pixel_stats_numpy(out, im))
    assert not got.count.any() and (got.argmin == -1).all()
    _hist(out, im, PX.histogram_numpy(out, im))
    none = PI.get("empty")
    got = _stats(none, im, PX.pixel_stats_numpy(none, im))
    assert got.count.shape == (0,) and got.sum.shape == (0, 3) and got.argmax.shape == (0, 3, 2)
    assert _hist(none, im, PX.histogram_numpy(none, im, 16, 0, 4)).hist.shape == (0, 3, 16)


# ---- ties and signs ----

def test_equal_extremes_in_other_waves_and_workgroups_go_to_the_lowest_y_x():
    got = _stats(PI.get("ties"), PI.image("ties"), PI.stats_ref("ties", "ties"))
    for c in range(3):
        x, y = PI.TIE_SPOTS[c]
        assert got.min[0, c] == 5 and tuple(got.argmin[0, c]) == (x, y)
        assert got.max[0, c] == 200 and tuple(got.argmax[0, c]) == ((x + 1) % PI.TIE_W, y)


@pytest.mark.parametrize("set_name", ["word_edges", "image_edges"])
def test_constant_image(set_name):
    pm = PI.get(set_name)
    got = _stats(pm, PI.image("const_u8"), PI.stats_ref(set_name, "const_u8"))
    assert np.array_equal(got.sum, 7 * np.broadcast_to(got.count[:, None], got.sum.shape))
    for i in np.nonzero(got.count)[0]:
        y, x = np.nonzero(pm.full(i, PI.H, PI.W))
        assert (got.argmin[i] == (x[0], y[0])).all() and (got.argmax[i] == (x[0], y[0])).all()


def test_both_signs_the_top_of_uint16_and_the_ends_of_int32():
    got = _stats(PI.get("word_edges"), PI.image("signs_i16"), PI.stats_ref("word_edges", "signs_i16"))
    assert (got.min < 0).any() and (got.max > 0).any() and (got.sum < 0).any() and (got.sum_xv < 0).any()
    big = _stats(PI.get("big"), PI.image("top_u16"), PI.stats_ref("big", "top_u16"))
    assert big.sum[0, 0] == 65535 * 90000 > 2 ** 32 and big.sumsq[0, 0] == 65535 ** 2 * 90000
    assert big.sum_xv[0, 0] == 65535 * 300 * (299 * 300 // 2) and tuple(big.argmax[0, 0]) == (0, 0)
    ends = _stats(PI.get("image_edges"), PI.image("ends_i32"), PI.stats_ref("image_edges", "ends_i32"))
    assert ends.min.min() == -PX.MAX_VALUE and ends.max.max() == PX.MAX_VALUE
    assert np.array_equal(ends.sumsq[:, 0], ends.count * PX.MAX_VALUE ** 2)


# ---- the grid ----

def test_130_instances_and_21_channels():
    pm = PI.get("many130")
    assert len(pm) == 130
    _stats(pm, PI.image("int32_c3"), PI.stats_ref("many130", "int32_c3"))
    got = _stats(pm, PI.image("c21_u8"), PI.stats_ref("many130", "c21_u8"))              # five tiles of 4 and one of 1
    assert got.sum.shape == (130, 21)
    im = PI.image("c21_u8")
    _hist(pm, im, PX.histogram_numpy(pm, im, 256, 0, 0))
    for C in (2, 6, 7):                                                                  # rests of 2 and of 3
        part = np.ascontiguousarray(im[:, :, :C])
        _stats(pm, part, PX.pixel_stats_numpy(pm, part))


# ---- the histogram ----

@pytest.mark.parametrize("case", sorted(PI.HISTOGRAMS))
def test_histograms(case):
    """uint8 with 256 bins; shift 4 with 16 bins; int16 with a negative lo; uint16 with shift 4 and 4096 bins; values below and
    above the range; the constant image (one hot cell per channel); 5 x 4096 cells (two channel groups)."""
    im = PI.image(PI.HISTOGRAMS[case][0])
    for set_name in ("word_edges", "image_edges"):
        pm = PI.get(set_name)
        got = _hist(pm, im, PI.hist_ref(set_name, case))
        assert np.array_equal(got.count, PI.frame_counts(pm))
        if case in ("i16_negative_lo", "u8_dropped"):
            assert (got.hist.sum(-1) < got.count[:, None])[got.count >= 60].all()
        elif case == "constant":
            assert np.array_equal(got.hist[:, :, 7], np.broadcast_to(got.count[:, None], got.hist.shape[:2]))
        else:
            assert np.array_equal(got.hist.sum(-1), np.broadcast_to(got.count[:, None], got.hist.shape[:2]))


def test_histogram_of_int32_and_its_percentiles():
    pm, im = PI.get("image_edges"), PI.image("int32_c1")
    got = _hist(pm, im, PX.histogram_numpy(pm, im, 1024, -PX.MAX_VALUE, 9))
    v = np.sort(im[:, :, 0][pm.full(10, PI.H, PI.W)])
    assert v[-1] == PX.MAX_VALUE and got.hist[10, 0].sum() == got.count[10] - 1          # (2^18 itself is one past the last bin)
    v = v[:-1]
    assert got.median()[10, 0] == -PX.MAX_VALUE + ((int(v[(len(v) + 1) // 2 - 1]) + PX.MAX_VALUE) >> 9 << 9)


# ---- against existing kernels ----

def test_ramp_images_against_the_moments_kernel():
    pm = PI.get("inside")
    m = pm.moments().m
    x1, y1 = pm.bounds[:, 0].astype(np.int64), pm.bounds[:, 1].astype(np.int64)
    m00, m10, m01, m20, m11, m02 = (m[:, k] for k in range(6))
    sx, sy = PX.pixel_stats(pm, PI.image("ramp_x")), PX.pixel_stats(pm, PI.image("ramp_y"))
    assert np.array_equal(sx.count, m00) and np.array_equal(sy.count, m00)
    assert np.array_equal(sx.sum[:, 0], m10 + x1 * m00) and np.array_equal(sx.sumsq[:, 0], m20 + 2 * x1 * m10 + x1 * x1 * m00)
    assert np.array_equal(sy.sum[:, 0], m01 + y1 * m00) and np.array_equal(sy.sumsq[:, 0], m02 + 2 * y1 * m01 + y1 * y1 * m00)
    assert np.array_equal(sx.sum_yv[:, 0], m11 + x1 * m01 + y1 * m10 + x1 * y1 * m00) and np.array_equal(sx.sum_yv, sy.sum_xv)


def test_a_mask_as_the_image_against_the_overlap_kernel():
    pm = PI.get("many130")
    clipped = pm.crop(0, 0, PI.W - 1, PI.H - 1)                           # (overlaps counts outside the image too)
    inter = clipped.overlaps()[0]
    for j in (0, 17, 129):
        got = PX.pixel_stats(pm, pm.full(j, PI.H, PI.W).astype(np.uint8))
        assert np.array_equal(got.sum[:, 0], inter[:, j]) and got.sum[j, 0] == got.count[j]


def test_the_label_map_as_the_image_against_the_layers():
    pm = PI.get("many130")
    n = len(pm)
    label = pm.to_labels(PI.H, PI.W)
    got = PX.histogram(pm, label, bins=n + 1)
    layers = pm.layered().crop(0, 0, PI.W - 1, PI.H - 1)
    inter = pm.crop(0, 0, PI.W - 1, PI.H - 1).overlaps(layers)[0]
    assert np.array_equal(got.hist[:, 0, 1:], inter) and not got.hist[:, 0, 0].any()
    assert np.array_equal(got.hist.sum(-1)[:, 0], got.count)


# ---- refusals ----

def _raw(pm, im, dtype=None, H=None, W=None, C=None, n=None, image_ptr=True, outputs=(True, True, True), hist=None):
    """One raw call with canaries in every output -> (status, the outputs)."""
    from mnc_amd.masks import _set_args
    im3 = im.reshape(im.shape[0], im.shape[1], -1)
    n_out, c_out = max(len(pm), 1), im3.shape[2]
    count = np.full(n_out, CANARY64, np.int64)
    args = list(_set_args(pm, areas=False))
    if n is not None:
        args[-1] = n
    args += [_lib.ptr(im3) if image_ptr else None, PX.DTYPES.index(im.dtype) if dtype is None else dtype,
             im3.shape[0] if H is None else H, im3.shape[1] if W is None else W, c_out if C is None else C]
    lib = _lib.load()
    if hist is None:
        sums, ext = np.full((n_out, c_out, 4), CANARY64, np.int64), np.full((n_out, c_out, 6), CANARY32, np.int32)
        outs = (count, sums, ext)
        args += [_lib.ptr(a) if keep else None for a, keep in zip(outs, outputs)] + [0]
        return lib.mnc_mask_pixel_stats(*args), outs
    bins, lo, shift = hist
    table = np.full((n_out, c_out, max(min(bins, 4096), 1)), CANARY64, np.int64)
    outs = (count, table)
    args += [lo, shift, bins] + [_lib.ptr(a) if keep else None for a, keep in zip(outs, outputs)] + [0]
    return lib.mnc_mask_histogram(*args), outs


def _intact(outs):
    return all((a == (CANARY32 if a.dtype == np.int32 else CANARY64)).all() for a in outs)


def test_an_int32_value_outside_the_range_is_refused_on_the_device_with_nothing_written():
    pm = PI.get("inside")
    for v in (PX.MAX_VALUE + 1, -PX.MAX_VALUE - 1):
        im = PI.image("int32_c3").copy()
        im[PI.H - 1, PI.W - 1, 2] = v                                   # (under no instance: the range is the image's)
        for hist in (None, (256, 0, 10)):
            rc, outs = _raw(pm, im, hist=hist)
            assert rc == INVALID and _intact(outs)
            assert b"int32 image value" in _lib.load().mnc_last_error()
        with pytest.raises(ValueError):
            PX.pixel_stats(pm, im)
        with pytest.raises(ValueError):
            pm.histogram(im, 256, 0, 10)
    rc, outs = _raw(pm, PI.image("int32_c3"))
    assert rc == 0 and not _intact(outs)


def test_bad_arguments_are_refused_before_anything_is_launched():
    pm, im = PI.get("inside"), PI.image("uint8_c3")
    bad = [dict(dtype=4), dict(dtype=-1), dict(H=0), dict(W=0), dict(H=32769), dict(W=32769), dict(H=8193, W=8193), dict(C=0), dict(C=33),
           dict(image_ptr=False), dict(n=-1), dict(n=2049), dict(outputs=(False, True, True)), dict(outputs=(True, False, True))]
    for kw in bad:
        for hist in (None, (256, 0, 0)):
            rc, outs = _raw(pm, im, hist=hist, **kw)
            assert rc == INVALID and _intact(outs), kw
    rc, outs = _raw(pm, im, outputs=(True, True, False))
    assert rc == INVALID and _intact(outs)
    for hist in ((0, 0, 0), (4097, 0, 0), (256, 0, -1), (256, 0, 32)):
        rc, outs = _raw(pm, im, hist=hist)
        assert rc == INVALID and _intact(outs), hist
    rc, outs = _raw(PI.get("many130"), np.zeros((PI.H, PI.W, 32), np.uint8), hist=(4096, 0, 0))      # 130 * 32 * 4096 > 2^24
    assert rc == INVALID and _intact(outs)
    far = PackedMasks([[2 ** 24, 0, 2 ** 24 + 3, 4]], [0], [0], None, None, np.zeros(8, np.uint64))
    odd = PackedMasks(pm.bounds, pm.offsets + 4, pm.areas, None, None, pm.bits)
    short = PackedMasks(pm.bounds, pm.offsets, pm.areas, None, None, pm.bits[:-1])
    for s in (far, odd, short):
        for hist in (None, (256, 0, 0)):
            rc, outs = _raw(s, im, hist=hist)
            assert rc == INVALID and _intact(outs)
    # the Python surface: ValueError
    for image in (im.astype(np.float32), im.astype(np.int64), np.zeros((PI.H, PI.W, 33), np.uint8), np.zeros((0, 4), np.uint8),
                  np.broadcast_to(np.uint8(0), (8193, 8193))):
        with pytest.raises(ValueError):
            pm.pixel_stats(image)
        with pytest.raises(ValueError):
            pm.histogram(image)
    for kw in (dict(bins=0), dict(bins=4097), dict(shift=32), dict(shift=-1), dict(lo=2 ** 31)):
        with pytest.raises(ValueError):
            pm.histogram(im, **kw)
    with pytest.raises(ValueError):
        far.pixel_stats(im)
    with pytest.raises(ValueError):
        PI.get("many130").histogram(np.zeros((PI.H, PI.W, 32), np.uint8), bins=4096)


# ---- the demo ----

def test_demo_pixel_stats_writes_mean_and_std_color(tmp_path):
    import glob
    import io
    import json
    from contextlib import redirect_stdout

    import demo
    from mnc_amd import models
    jpg = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "demo", "*.jpg")))[0]
    proto = models.write_mnc_5stage_test_prototxt(width_div=8)
    name = os.path.splitext(os.path.basename(jpg))[0]
    got, raw, saved = {}, {}, {}
    for key, flags in (("plain", []), ("stats", ["--pixel-stats"]), ("stats_cpu", ["--pixel-stats", "--cpu"])):
        out = str(tmp_path / (key + ".json"))
        os.makedirs(str(tmp_path / key))
        with redirect_stdout(io.StringIO()):
            demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-annotations", out, "--save-masks", str(tmp_path / key),
                       "--vis-thresh", "0.0"] + flags)
        with open(out) as f:
            raw[key] = f.read()
        got[key] = json.loads(raw[key])
        saved[key] = PackedMasks.load(str(tmp_path / key / (name + "_masks.npz")))
    pm, ann = saved["stats"], got["stats"]["annotations"]
    assert len(pm) == len(ann) == len(got["plain"]["annotations"]) > 0
    assert not any("mean_color" in a or "std_color" in a for a in got["plain"]["annotations"])
    st = PX.pixel_stats_numpy(pm, demo._read_image_bgr(jpg))
    assert st.count.any()
    for i, a in enumerate(ann):
        assert a["mean_color"] == ([float(v) for v in st.mean()[i, ::-1]] if st.count[i] else None)
        assert a["std_color"] == ([float(v) for v in st.std()[i, ::-1]] if st.count[i] else None)
    assert [a["mean_color"] for a in got["stats_cpu"]["annotations"]] == [a["mean_color"] for a in ann]
    # without the flag the file is, byte for byte, the file with the flag less the two keys
    less = dict(got["stats"], annotations=[{k: v for k, v in a.items() if k not in ("mean_color", "std_color")} for a in ann])
    assert json.dumps(less) == raw["plain"]
