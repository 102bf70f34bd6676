"""Inputs shared by tests/test_pixel_stats_host.py and tests/test_gpu_pixel_stats.py: packed mask sets and images placed where
csrc/mask_pixels.hip can go wrong -- widths around the 64-column word crossed with heights 1, 2 and 65 at x1 = 0, 1 and 63 modulo
64 (padding bits set) on a 67 x 131 image, which is no multiple of 4 or 64 either way; instances that hang over each edge of the
image, lie outside it, have no rows or no bit; one instance of more than one workgroup of words with equal extremes planted in
different waves and workgroups; 130 small instances; no instance.  Every set and image is seeded; every reference (the numpy
statements of mnc_amd.pixels) is computed once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_overlap_inputs as MI  # noqa: E402  (pack; sets up the reference-shaped import paths)
from mnc_amd import pixels as PX  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

H, W = 67, 131
WIDTHS = [1, 63, 64, 65, 127, 128, 129]
HEIGHTS = [1, 2, 65]
STARTS = [0, 1, 63]                                 # x1 modulo 64
CHANNELS = [1, 3, 4, 5]
DTYPES = [np.uint8, np.uint16, np.int16, np.int32]
MAX_VALUE = 2 ** 18
TIE_W, TIE_H = 129, 65                              # 3 words a row, 195 words: four workgroups of 64 words, waves of 16


def _random(rng, h, w):
    m = rng.random((h, w)) < 0.5
    m[0, 0] = m[-1, -1] = True
    return m


def word_edges_set(dirty=True):
    """WIDTHS x HEIGHTS x STARTS random masks; x1 is 0, 1, 63 or those plus 64 where the width still ends inside the image, y1 is 0
    .. 2.  The wider ones hang over the right edge."""
    rng = np.random.default_rng(2100)
    bounds, dense = [], []
    for w in WIDTHS:
        for h in HEIGHTS:
            for s in STARTS:
                x1 = s + 64 if s + 64 + w <= W and (w + h) % 2 else s
                y1 = (w + s) % 3                                  # (65 rows from row 2 on end on the last row)
                bounds.append([x1, y1, x1 + w - 1, y1 + h - 1])
                dense.append(_random(rng, h, w))
    return MI.pack(bounds, dense, None, None, dirty)


def image_edges_set(dirty=True):
    """Over the left, top, right and bottom edge; negative x1 and y1; wholly outside (right of, below, left of by more than a word);
    no rows; rows and no set bit; larger than the image on every side, its first word column left of the image."""
    rng = np.random.default_rng(2101)
    bounds = [[-10, 20, 29, 30], [40, -5, 110, 3], [100, 10, 170, 40], [5, 60, 80, 75], [-70, -6, 20, 9], [200, 5, 240, 9],
              [3, 67, 40, 70], [-200, 3, -65, 8], [0, 0, -1, -1], [10, 10, 80, 14], [-70, -3, 229, 76], [130, 66, 131, 67]]
    dense = []
    for k, (x1, y1, x2, y2) in enumerate(bounds):
        h, w = max(y2 - y1 + 1, 0), max(x2 - x1 + 1, 0)
        dense.append(np.zeros((h, w), bool) if k in (8, 9) else _random(rng, h, w))
    return MI.pack(bounds, dense, None, None, dirty)


def tie_set():
    """One full instance of TIE_W x TIE_H at the origin."""
    return MI.pack([[0, 0, TIE_W - 1, TIE_H - 1]], [np.ones((TIE_H, TIE_W), bool)], None, None, True)


# (x, y) of the planted extremes: word 3 y + x // 64 of the instance -- wave 0 and wave 1 of workgroup 0, workgroup 1, workgroup 3
TIE_SPOTS = [(10, 2), (70, 8), (5, 40), (128, 64)]


def tie_image():
    """uint8 [H, W, 3] of 100s.  Channel c has the least value 5 and the greatest 200 planted at TIE_SPOTS[c:]: the first of them
    in (y, x) order must win, and it lies in another wave or workgroup for every channel."""
    im = np.full((H, W, 3), 100, np.uint8)
    for c in range(3):
        for x, y in TIE_SPOTS[c:]:
            im[y, x, c] = 5
            im[y, (x + 1) % TIE_W, c] = 200
    return im


def many_set(n=130):
    rng = np.random.default_rng(2102)
    bounds, dense = [], []
    for _ in range(n):
        h, w = int(rng.integers(1, 30)), int(rng.integers(1, 70))
        x1, y1 = int(rng.integers(-5, W - 3)), int(rng.integers(-5, H - 3))
        bounds.append([x1, y1, x1 + w - 1, y1 + h - 1])
        dense.append(_random(rng, h, w))
    return MI.pack(bounds, dense, None, None, True)


def inside_set():
    """Instances wholly inside the image, for the closed forms on the moments: widths around the word, negative nowhere."""
    rng = np.random.default_rng(2103)
    bounds = [[0, 0, 63, 9], [1, 3, 65, 66], [63, 0, 130, 1], [2, 2, 130, 66], [64, 30, 64, 30], [7, 5, 70, 40]]
    return MI.pack(bounds, [_random(rng, b[3] - b[1] + 1, b[2] - b[0] + 1) for b in bounds], None, None, True)


def empty_set():
    return PackedMasks(np.zeros((0, 4), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), None, None, np.zeros(0, np.uint64))


def big_set():
    """One full 300 x 300 instance."""
    return MI.pack([[0, 0, 299, 299]], [np.ones((300, 300), bool)])


SETS = {"word_edges": word_edges_set, "image_edges": image_edges_set, "ties": tie_set, "many130": many_set, "inside": inside_set,
        "empty": empty_set, "big": big_set}


def random_image(dtype, C, seed=0, h=H, w=W):
    """[h, w, C] ([h, w] for C = 0) over the whole range of the dtype; int32 over [-2^18, 2^18] with both ends present."""
    rng = np.random.default_rng(2200 + seed)
    shape = (h, w, C) if C else (h, w)
    if np.dtype(dtype) == np.int32:
        im = rng.integers(-MAX_VALUE, MAX_VALUE + 1, shape).astype(np.int32)
        im.reshape(-1)[:2] = (-MAX_VALUE, MAX_VALUE)
        return im
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max + 1, shape).astype(dtype)


def ramp_images():
    """-> (x, y): uint8 [H, W] images whose value is the pixel's column resp. row."""
    yy, xx = np.mgrid[0:H, 0:W]
    return xx.astype(np.uint8), yy.astype(np.uint8)


IMAGES = {"ties": tie_image,
          "const_u8": lambda: np.full((H, W, 3), 7, np.uint8),
          "signs_i16": lambda: random_image(np.int16, 3, 1),
          "top_u16": lambda: np.full((300, 300), 65535, np.uint16),
          "ends_i32": lambda: np.where(np.random.default_rng(2104).random((H, W, 2)) < 0.5, -MAX_VALUE, MAX_VALUE).astype(np.int32),
          "c21_u8": lambda: random_image(np.uint8, 21, 2),
          "ramp_x": lambda: ramp_images()[0], "ramp_y": lambda: ramp_images()[1]}
for _d in DTYPES:
    for _c in CHANNELS:
        IMAGES["%s_c%d" % (np.dtype(_d).name, _c)] = (lambda d=_d, c=_c: random_image(d, c))

# name -> (image, bins, lo, shift): the histogram cases
HISTOGRAMS = {"u8_256": ("uint8_c3", 256, 0, 0),
              "u8_shift4": ("uint8_c3", 16, 0, 4),
              "i16_negative_lo": ("int16_c3", 128, -20000, 8),           # covers -20000 .. 12767: values below and above are dropped
              "u16_shift4_4096": ("uint16_c1", 4096, 0, 4),
              "u8_dropped": ("uint8_c4", 100, 50, 0),                    # covers 50 .. 149
              "constant": ("const_u8", 256, 0, 0),
              "groups": ("uint16_c5", 4096, 0, 4)}                       # 5 x 4096 cells: two channel groups

_SETS, _IMAGES, _REFERENCE = {}, {}, {}


def get(name):
    if name not in _SETS:
        _SETS[name] = SETS[name]()
    return _SETS[name]


def image(name):
    if name not in _IMAGES:
        _IMAGES[name] = IMAGES[name]()
        _IMAGES[name].setflags(write=False)
    return _IMAGES[name]


def stats_ref(set_name, image_name):
    key = ("stats", set_name, image_name)
    if key not in _REFERENCE:
        _REFERENCE[key] = PX.pixel_stats_numpy(get(set_name), image(image_name))
    return _REFERENCE[key]


def hist_ref(set_name, case):
    key = ("hist", set_name, case)
    if key not in _REFERENCE:
        im, bins, lo, shift = HISTOGRAMS[case]
        _REFERENCE[key] = PX.histogram_numpy(get(set_name), image(im), bins, lo, shift)
    return _REFERENCE[key]


def same_fields(got, want):
    """Two PixelStats or two MaskHistograms: the same type, and every field the same dtype, shape and values."""
    assert type(got) is type(want) and len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, np.ndarray):
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), got._fields[k]
        else:
            assert a == b, got._fields[k]
    return True


def frame_counts(pm, h=H, w=W):
    """int64 [n]: the popcount of every instance ANDed with the image frame, from the words."""
    out = np.zeros(len(pm), np.int64)
    for i in range(len(pm)):
        hh, ww = pm.size(i)
        if hh == 0 or ww == 0:
            continue
        x1, y1 = int(pm.bounds[i][0]), int(pm.bounds[i][1])
        yy, xx = np.mgrid[0:hh, 0:ww]
        frame = (yy + y1 >= 0) & (yy + y1 < h) & (xx + x1 >= 0) & (xx + x1 < w)
        out[i] = int((pm.dense(i) & frame).sum())
    return out
