"""The numpy statements of the geometric transforms of packed masks (mnc_amd.warp.isometry_numpy, warp_numpy and the host helpers)
pinned to facts that do not come from them: numpy's own flips, transpose and rot90 on full(i, H, W), the group laws, np.kron and
strided slicing for the integer resizes, Pillow's NEAREST on integer upscales, a per-pixel brute force in Python integers, and the
closed form of an integer shear.  tests/test_gpu_mask_warp.py holds csrc/mask_warp.hip to these statements."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import mask_warp_inputs as WI  # noqa: E402
from mnc_amd import algebra as AL  # noqa: E402
from mnc_amd import warp as WP  # noqa: E402
from mnc_amd.masks import PackedMasks, mask_overlaps_numpy  # noqa: E402


def _fulls(pm, H, W):
    return [pm.full(i, H, W) for i in range(len(pm))]


def _same_fulls(got, arrays, H, W):
    assert len(got) == len(arrays) and WI.canonical(got)
    for i, m in enumerate(arrays):
        assert np.array_equal(got.full(i, H, W), m), i
    return True


# ---- the isometries against numpy ----

@pytest.mark.parametrize("name,H,W", [("image0",) + WI.IMAGES[0], ("image1",) + WI.IMAGES[1]])
def test_isometries_are_numpys_flips_transpose_and_rotations(name, H, W):
    pm = WI.get(name)
    fulls = _fulls(pm, H, W)
    assert H % 64 and W % 64 and sum(m.any() for m in fulls) >= 7
    table = [(np.fliplr, (2, W - 1, 0), (H, W)), (np.flipud, (4, 0, H - 1), (H, W)), (np.transpose, (1, 0, 0), (W, H)),
             (lambda m: np.rot90(m, 1), (5, 0, W - 1), (W, H)), (lambda m: np.rot90(m, 2), (6, W - 1, H - 1), (H, W)),
             (lambda m: np.rot90(m, 3), (3, H - 1, 0), (W, H))]
    for fn, args, (H2, W2) in table:
        assert _same_fulls(WP.isometry_numpy(pm, *args), [fn(m) for m in fulls], H2, W2), args
    for k in range(-1, 5):
        H2, W2 = (W, H) if k % 2 else (H, W)
        assert _same_fulls(WP.isometry_numpy(pm, *WP.rot90_code(k, H, W)), [np.rot90(m, k) for m in fulls], H2, W2), k
    # the instances inside the image keep all their pixels; the set as a whole keeps them under every code
    for code in WI.CODES:
        got = WP.isometry_numpy(pm, code, 5, -3)
        assert np.array_equal(got.areas, AL.combine_numpy(pm, None, "copy").areas)
        assert np.array_equal(got.classes, pm.classes) and np.array_equal(got.scores, pm.scores)


def test_group_laws():
    H, W = WI.IMAGES[0]
    pm = WI.get("image0")
    tight = AL.combine_numpy(pm, None, "copy")
    iso = WP.isometry_numpy
    assert WI.same_masks(iso(iso(pm, 2, W - 1, 0), 2, W - 1, 0), tight)
    assert WI.same_masks(iso(iso(pm, 4, 0, H - 1), 4, 0, H - 1), tight)
    assert WI.same_masks(iso(iso(pm, 1), 1), tight)
    turned, h, w = pm, H, W
    for _ in range(4):
        turned = iso(turned, *WP.rot90_code(1, h, w))
        h, w = w, h
    assert WI.same_masks(turned, tight)
    assert WI.same_masks(iso(iso(pm, 2, W - 1, 0), 1), iso(pm, *WP.rot90_code(1, H, W)))          # transpose after fliplr
    assert WI.same_masks(iso(pm, 0), tight)
    moved = WP.translate(pm, -100, 33)
    assert WI.same_masks(WP.translate(moved, 100, -33), pm) and moved.bits is not None
    assert np.array_equal(moved.bounds[1], pm.bounds[1] + [-100, 33, -100, 33]) and tuple(moved.bounds[6]) == (0, 0, -1, -1)
    assert WI.same_masks(iso(pm, 0, -100, 33), AL.combine_numpy(moved, None, "copy"))


@pytest.mark.parametrize("code", WI.CODES)
def test_overlaps_are_those_of_the_images(code):
    a, b = WI.get("image0"), WI.get("negative")
    both = lambda pm: WP.isometry_numpy(pm, code, 17, -9)    # noqa: E731
    want = mask_overlaps_numpy(a.take([0, 3, 5]), a.take([1, 3, 4, 7]))
    got = mask_overlaps_numpy(both(a).take([0, 3, 5]), both(a).take([1, 3, 4, 7]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0].any()
    assert np.array_equal(mask_overlaps_numpy(both(b))[0], mask_overlaps_numpy(b)[0])


# ---- the gather against the isometries ----

@pytest.mark.parametrize("code", WI.CODES)
def test_the_gather_through_an_isometry_map_is_the_isometry(code):
    for name in ("word", "negative"):
        pm = WI.get(name)
        for tx, ty in ((0, 0), WI.SHIFTS[code]):
            want = WI.isometry_ref(name, code, tx, ty)
            coef, den = WP.isometry_map(code, tx, ty)
            assert den == 1
            assert WI.same_masks(WP.warp_numpy(pm, coef, den, (-2000, -2000, 2000, 2000)), want), (name, code)
            # the loose frame of an isometry map is the image of the bounds
            for i in range(len(pm)):
                if AL._rows(pm, i):
                    assert WP.warp_frame(AL._box(pm, i), coef, den, (-2000, -2000, 2000, 2000)) == \
                        WP.isometry_frame(AL._box(pm, i), code, tx, ty)
    # ... and so the extent of a brute force over full rectangles
    full = WI.get("rectangle")
    coef, den = WP.isometry_map(code, *WI.SHIFTS[code])
    for i in range(len(full)):
        f = WP.isometry_frame(AL._box(full, i), code, *WI.SHIFTS[code])
        window = (f[0] - 2, f[1] - 2, f[2] + 2, f[3] + 2)
        pixels = WI.brute_force(full.take([i]), coef, den, window)[0]
        xs, ys = [x for x, _ in pixels], [y for _, y in pixels]
        assert (min(xs), min(ys), max(xs), max(ys)) == WP.warp_frame(AL._box(full, i), coef, den, window) == f, (code, i)
    crossed = WI.isometry_ref("word", code, *WI.SHIFTS[code])
    b = crossed.bounds[crossed.areas > 0]                    # results lie across zero in x, and in y
    assert ((b[:, 0] < 0) & (b[:, 2] > 0)).any() and ((b[:, 1] < 0) & (b[:, 3] > 0)).any()


# ---- the resize ----

@pytest.mark.parametrize("name,H,W", [("image0",) + WI.IMAGES[0], ("image1",) + WI.IMAGES[1]])
def test_resize_closed_forms(name, H, W):
    pm = WI.get(name)
    fulls = _fulls(pm, H, W)
    resized = lambda H2, W2: WP.warp_numpy(pm, *WP.resize_map(H, W, H2, W2), window=(0, 0, W2 - 1, H2 - 1))   # noqa: E731
    for k in (2, 3):
        assert _same_fulls(resized(k * H, k * W), [np.kron(m, np.ones((k, k), bool)) for m in fulls], k * H, k * W), k
    for k in (3, 5):
        if H % k == 0 and W % k == 0:
            assert _same_fulls(resized(H // k, W // k), [m[k // 2::k, k // 2::k] for m in fulls], H // k, W // k), k
    assert _same_fulls(resized(H, W), fulls, H, W)
    coef, den = WP.resize_map(H, W, H, W)
    assert all((coef[0] * x + coef[2]) // den == x for x in range(-5, 80)) and coef[1] == coef[3] == 0
    # the stated formula, whatever the common factor that was divided out
    coef, den = WP.resize_map(H, W, 50, 61)
    for x in range(61):
        assert (coef[0] * x + coef[2]) // den == ((2 * x + 1) * W) // (2 * 61)
    for y in range(50):
        assert (coef[4] * y + coef[5]) // den == ((2 * y + 1) * H) // (2 * 50)


def test_odd_downscales_take_the_centre_pixel():
    # 37 x 70 has no odd divisor in common: an image of 45 x 75 for the factors 3 and 5
    rng = np.random.default_rng(5)
    H, W = 45, 75
    full = rng.random((H, W)) < 0.5
    pm = PackedMasks.from_dense([[0, 0, W - 1, H - 1]], [full])
    for k in (3, 5):
        got = WP.warp_numpy(pm, *WP.resize_map(H, W, H // k, W // k), window=(0, 0, W // k - 1, H // k - 1))
        assert np.array_equal(got.full(0, H // k, W // k), full[k // 2::k, k // 2::k])


def test_pillow_nearest_agrees_on_integer_upscales():
    from PIL import Image
    nearest = getattr(Image, "Resampling", Image).NEAREST
    H, W = WI.IMAGES[0]
    pm = WI.get("image0")
    for k in (2, 3):
        got = WP.warp_numpy(pm, *WP.resize_map(H, W, k * H, k * W), window=(0, 0, k * W - 1, k * H - 1))
        for i in (0, 3, 5):
            pil = np.asarray(Image.fromarray(pm.full(i, H, W).astype(np.uint8) * 255).resize((k * W, k * H), nearest)) > 0
            assert np.array_equal(got.full(i, k * H, k * W), pil), (k, i)


# ---- the gather against a brute force ----

@pytest.mark.parametrize("key", sorted(WI.maps()))
def test_the_gather_is_the_per_pixel_rule_in_python_integers(key):
    name, coef, den = WI.maps()[key]
    pm = WI.get(name)
    window = (-40, -30, 130, 80)
    want = WI.brute_force(pm, coef, den, window)
    got = WI.warp_ref(name, coef, den, window)
    assert WI.canonical(got) and sum(len(p) for p in want) > 500
    assert WI.pixels_of(got) == want
    # the loose frame holds every pixel of the brute force
    for i, pixels in enumerate(want):
        if pixels:
            f = WP.warp_frame(AL._box(pm, i), coef, den, window)
            assert all(f[0] <= x <= f[2] and f[1] <= y <= f[3] for x, y in pixels), i


def test_the_maps_are_what_they_are_called():
    coef, den = WP.affine_map(WI.ROTATION, 16)
    assert den == 65536 and abs(coef[0] / den - np.cos(np.pi / 6)) < 1e-4 and abs(coef[1] / den + 0.5) < 1e-4
    # the forward matrix takes the centre to itself; so does the inverse map, to the rounding
    assert (coef[0] * 34 + coef[1] * 17 + coef[2]) // den in (33, 34) and (coef[3] * 34 + coef[4] * 18 + coef[5]) // den in (17, 18)
    inv = np.concatenate((np.linalg.inv(WI.SHEAR[:, :2]), -np.linalg.inv(WI.SHEAR[:, :2]).dot(WI.SHEAR[:, 2:])), axis=1)
    assert WP.affine_map(inv, 10, inverse=True) == WP.affine_map(WI.SHEAR, 10)
    assert WP.affine_map(np.array([[1.0, 0, 0], [0, 1.0, 0]]), 16) == ((65536, 0, 32768, 0, 65536, 32768), 65536)
    name, coef, den = WI.maps()["negative"]
    assert min(coef) < 0 and den & (den - 1) and (WI.get(name).bounds[:, :2] < 0).all()


def test_an_integer_shear_shifts_each_row_of_a_rectangle():
    pm = WI.get("rectangle")
    coef, den = WI.INTEGER_SHEAR
    window = (-400, -10, 400, 70)
    got = WP.warp_numpy(pm, coef, den, window)
    for i in range(len(pm)):
        x1, y1, x2, y2 = (int(v) for v in pm.bounds[i])
        want = {(x, y) for y in range(y1, y2 + 1) for x in range(x1 - 2 * y, x2 - 2 * y + 1)}
        assert WI.pixels_of(got)[i] == want
        assert tuple(got.bounds[i]) == (x1 - 2 * y2, y1, x2 - 2 * y1, y2)


def test_windows_and_an_empty_result():
    name, coef, den = WI.maps()["rotation16"]
    pm = WI.get(name)
    whole = WI.pixels_of(WI.warp_ref(name, coef, den, WI.WINDOWS[0]))
    for window in WI.WINDOWS[1:]:
        cut = [{(x, y) for x, y in p if window[0] <= x <= window[2] and window[1] <= y <= window[3]} for p in whole]
        assert WI.pixels_of(WI.warp_ref(name, coef, den, window)) == cut, window
    far = WP.warp_numpy(pm, coef, den, WI.FAR_WINDOW)
    assert not far.areas.any() and far.bits.size == 0 and (far.bounds == (0, 0, -1, -1)).all()
    e = WI.get("empty")
    assert len(WP.warp_numpy(e, coef, den, WI.WINDOWS[0])) == 0 and len(WP.isometry_numpy(e, 3)) == 0


# ---- the limits ----

def test_every_limit_raises_value_error():
    pm = WI.get("rectangle")
    ident, win = (1, 0, 0, 0, 1, 0), (0, 0, 9, 9)
    for args in ((8, 0, 0), (-1, 0, 0), (2, 1 << 24, 0), (4, 0, -(1 << 24)), (2, (1 << 24) - 1, 0), (1, 0, (1 << 24) - 100)):
        with pytest.raises(ValueError):
            WP.isometry_numpy(pm, *args)
        with pytest.raises(ValueError):
            WP.isometry(pm, *args)                           # refused before the library is asked
    for coef, den, window in ((ident, 0, win), (ident, (1 << 32) + 1, win), (ident, 1, (0, 0, 1 << 24, 5)), (ident, 1, (5, 5, 4, 9)),
                              (ident, 1, (5, 5, 9, 4)), (ident, 1, None), ((1, 2, 0, 2, 4, 0), 1, win), ((0, 0, 0, 0, 0, 0), 1, win),
                              (((1 << 32) + 1, 0, 0, 0, 1, 0), 1, win), ((1, -(1 << 32) - 1, 0, 0, 1, 0), 1, win),
                              ((1, 0, 0, (1 << 32) + 1, 1, 0), 1, win), ((1, 0, 0, 0, -(1 << 32) - 1, 0), 1, win),
                              ((1, 0, (1 << 60) + 1, 0, 1, 0), 1, win), ((1, 0, 0, 0, 1, -(1 << 60) - 1), 1, win),
                              ((1, 0, 0, 0, 1), 1, win)):
        with pytest.raises(ValueError):
            WP.warp_numpy(pm, coef, den, window)
        with pytest.raises(ValueError):
            WP.warp(pm, coef, den, window)
    # at the limits themselves the statement answers
    assert WP.warp_numpy(pm, (1 << 32, 0, 0, 0, 1 << 32, 0), 1 << 32, (0, 0, 30, 30)).areas.tolist() == [16 * 7, 31 * 3, 0]
    assert WP.warp_numpy(pm, (1, 0, -(1 << 60), 0, 1, 1 << 60), 1, win).areas.tolist() == [0, 0, 0]
    # more than 2^27 pixels of loose-frame rows: three instances blown up 3000 times each way
    big = PackedMasks(np.array([[0, 0, 9, 9]] * 3, np.int32), [0, 80, 160], [0, 0, 0], None, None, np.zeros(30, np.uint64))
    with pytest.raises(ValueError):
        WP.warp_numpy(big, (1, 0, 0, 0, 1, 0), 3000, (0, 0, 40000, 40000))
    with pytest.raises(ValueError):
        WP.isometry_numpy(PackedMasks(np.zeros((2049, 4), np.int32) + [0, 0, -1, -1], np.zeros(2049), np.zeros(2049), None, None,
                                      np.zeros(0, np.uint64)), 1)
    with pytest.raises(ValueError):
        WP.translate(pm, 1 << 24, 0)
    with pytest.raises(ValueError):
        WP.resize_map(0, 5, 5, 5)
    with pytest.raises(ValueError):
        WP.affine_map(np.array([[1.0, 2.0, 0], [2.0, 4.0, 0]]))                                    # singular
    with pytest.raises(ValueError):
        WP.affine_map(np.full((2, 3), np.nan), inverse=True)


def test_the_size_bound_needs_no_gpu():
    """out_bits == NULL: *bits_bound from the bounds alone, on the host -- the statement's loose frames."""
    import ctypes
    from mnc_amd import _lib
    from mnc_amd.masks import _set_args
    for key, (name, coef, den) in sorted(WI.maps().items()):
        pm = WI.get(name)
        for window in WI.WINDOWS[:3]:
            bound, used = ctypes.c_size_t(12345), ctypes.c_size_t(54321)
            c, win = np.array(coef, np.int64), np.array(window, np.int32)
            _lib.call("mnc_mask_warp", *(_set_args(pm, areas=False) + (_lib.ptr(c), den, _lib.ptr(win), None, None, None, None, 0,
                                                                        ctypes.addressof(bound), ctypes.addressof(used), 0)))
            frames = [WP.warp_frame(AL._box(pm, i), coef, den, window) for i in range(len(pm)) if AL._rows(pm, i)]
            assert bound.value == WI.bound_bytes(frames) and used.value == 54321, (key, window)


# ---- the demo's helper ----

def test_flip_tta_helper_on_the_host():
    import demo
    a, b, W = WI.tta_sets()
    mirror = WP.isometry_numpy(a, 2, W - 1, 0)               # what the mirrored run would give for the same instances
    got = demo._flip_tta(a, mirror, W, 0.5, cpu=True)
    assert WI.same_masks(got, a)                             # exactly the input's instances: the duplicates lose on equal scores
    far = WP.isometry_numpy(b, 2, W - 1, 0)
    got = demo._flip_tta(a, far, W, 0.5, cpu=True)
    tight_b = AL.combine_numpy(b, None, "copy")
    assert len(got) == len(a) + len(b) and WI.same_masks(got.take(range(len(a))), a)
    assert WI.same_masks(got.take(range(len(a), len(got))), tight_b)
