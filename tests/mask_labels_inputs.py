"""Inputs shared by tests/test_mask_labels_host.py and tests/test_gpu_mask_labels.py: label maps placed where csrc/mask_labels.hip
can go wrong -- widths around the 64-pixel strip of a wave and heights of one, two and more rows than a strip has pixels, boxes that
start at columns 0, 1, 63, 64 and 65 (a shift of 0 and of 63 into two destination words), runs of length one, a run that fills a row,
single pixels, ids in one bitmap word, in neighbouring words, past the first scan tile of bitmap words and at the top of the range,
maps without an instance, exactly and one more than 2048 labels, class maps -- and the sets of tests/mask_algebra_inputs.py and
tests/mask_warp_inputs.py for the way back.  Every map is seeded; every reference (the numpy statements of mnc_amd.labels) is
computed once per key and left unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_algebra_inputs as AI  # noqa: E402  (sets up the reference-shaped import paths)
import mask_warp_inputs as WI  # noqa: E402
from mnc_amd import labels as LB  # noqa: E402

WIDTHS = [1, 63, 64, 65, 130]
HEIGHTS = [1, 2, 65]
BOX_STARTS = [0, 1, 63, 64, 65]
TOP_ID = 2 ** 24 - 1
BLOBS_SIZE = (299, 599)            # the blobs of mask_algebra_inputs lie between -50 .. 748 and -20 .. 319: cut on every side
EDGE_SIZE = (29, 199)              # the 1025 small instances of its edge set: -30 .. 235 and -5 .. 32
SURVIVORS = {"blobs": 245, "edge": 467}    # instances that keep a pixel inside those images once layered


def patches(H, W, n_labels, seed, first=1):
    """int32 [H, W]: random rectangles of labels first .. first + n_labels - 1 painted over a background of 0 (some labels may end
    up covered: the statement finds what is there)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((H, W), np.int32)
    for k in range(n_labels):
        h, w = int(rng.integers(1, max(H // 2, 1) + 1)), int(rng.integers(1, max(W // 2, 1) + 1))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        out[y:y + h, x:x + w] = first + k
    return out


def box_edges():
    """int32 [12, 200]: per start column s of BOX_STARTS an instance of two ragged rows from s on, 71 and 130 columns wide, so that
    its rows take two resp. three words and its pixels come from two to four strips."""
    out = np.zeros((12, 200), np.int32)
    for k, s in enumerate(BOX_STARTS):
        out[2 * k, s:s + 71] = k + 1
        out[2 * k + 1, s + 3:s + 130] = k + 1
        out[2 * k + 1, s + 40] = 0                               # a hole
    out[10, 199] = 9                                             # the last column alone
    out[11, 0] = 8
    return out


def checkerboard():
    yy, xx = np.mgrid[0:5, 0:130]
    return ((yy + xx) % 2 + 1).astype(np.int32)


def full_row():
    out = patches(4, 130, 3, 41)
    out[2] = 7
    return out


def single_pixels():
    out = np.zeros((65, 130), np.int32)
    rng = np.random.default_rng(42)
    flat = rng.choice(65 * 130, 40, replace=False)
    out.reshape(-1)[flat] = np.arange(1, 41)
    out[0, 0], out[64, 129], out[0, 63], out[0, 64] = 50, 51, 52, 53
    return out


def with_ids(ids, seed=43):
    """A patches map whose labels 1 .. len(ids) are renamed to `ids`."""
    base = patches(20, 90, len(ids), seed)
    table = np.zeros(len(ids) + 1, np.int32)
    table[1:] = ids
    return table[base]


def labels_2048():
    """int32 [64, 64]: exactly 2048 labels, 1 .. 2048, of two pixels each."""
    return (np.arange(64 * 64).reshape(64, 64) // 2 + 1).astype(np.int32)


def labels_2049():
    """The same with one pixel renamed: 2049 labels."""
    out = labels_2048()
    out[63, 63] = 5000
    return out


def class_maps():
    """(inst, cls): an SBD-shaped pair -- every instance of one class, class ids 1 .. 20, background 0 in both."""
    inst = patches(40, 70, 9, 44)
    cls = np.zeros_like(inst)
    for i in np.unique(inst)[1:]:
        cls[inst == i] = (int(i) * 7) % 20 + 1
    return inst, cls


def mixed_class_maps():
    """(inst, cls, the smallest id of mixed class): two instances have one pixel of another class."""
    inst, cls = class_maps()
    ids = np.unique(inst)[1:]
    cls = cls.copy()
    for i in (ids[-1], ids[2]):
        ys, xs = np.nonzero(inst == i)
        cls[ys[-1], xs[-1]] += 1
    return inst, cls, int(ids[2])


def superpixel_image():
    """The engineered superpixel image of tests/mcg_inputs.py, int32 [420, 460]: 18795 labels -- nine times the 2048 a set may
    hold, so the whole image is a map that from_labels must refuse with its count."""
    import mcg_inputs as MC
    return MC.engineered_image(0)["superpixels"].astype(np.int32)


SUPERPIXEL_LABELS = 18795


def superpixel_part():
    """A 70 x 130 window of it: 1659 labels with ids up to 18895, most of them a handful of pixels."""
    return np.ascontiguousarray(superpixel_image()[200:270, 100:230])


REFUSED_MAPS = {"superpixels": superpixel_image, "labels_2049": labels_2049}
MAPS = {
    "box_edges": box_edges, "checkerboard": checkerboard, "full_row": full_row, "single_pixels": single_pixels,
    "one_word": lambda: with_ids([31, 30, 29]), "word_edge": lambda: with_ids([31, 32, 33]),
    "scan_tile": lambda: with_ids([32767, 32768, 40000]), "top_id": lambda: with_ids([5, TOP_ID]),
    "labels_2048": labels_2048, "class_inst": lambda: class_maps()[0], "superpixels_part": superpixel_part,
    "blobs": lambda: LB.to_labels_numpy(AI.get("blobs"), *BLOBS_SIZE),
}
for _w in WIDTHS:
    for _h in HEIGHTS:
        MAPS["size_%dx%d" % (_h, _w)] = (lambda h, w: lambda: patches(h, w, 6, 100 + 7 * h + w))(_h, _w)
SIZE_MAPS = sorted(k for k in MAPS if k.startswith("size_"))
_MAPS, _REFERENCE = {}, {}


def get(name):
    if name not in _MAPS:
        _MAPS[name] = (MAPS[name] if name in MAPS else REFUSED_MAPS[name])()
        _MAPS[name].setflags(write=False)
    return _MAPS[name]


def reference(key, make):
    """make() computed once per key and left unchanged."""
    if key not in _REFERENCE:
        _REFERENCE[key] = make()
    return _REFERENCE[key]


def from_ref(name, background=0):
    """from_labels_numpy of the map of that name -> (PackedMasks, ids)."""
    return reference((name, "from", background), lambda: LB.from_labels_numpy(get(name), None, background))


def to_ref(name, pm, H, W, values=None, order=None, background=0):
    key = (name, "to", H, W, None if values is None else tuple(int(v) for v in values),
           None if order is None else tuple(int(v) for v in order), background)
    return reference(key, lambda: LB.to_labels_numpy(pm, H, W, values, order, background))


def sets():
    """name -> (PackedMasks, H, W) for to_labels: equal scores, nested stacks, 1025 small instances, no instance, dirty padding,
    negative bounds."""
    return {"equal": (AI.get("equal"), AI.IMAGE_H, AI.IMAGE_W), "nested_up": (AI.get("nested_up"), AI.IMAGE_H, AI.IMAGE_W),
            "nested_down": (AI.get("nested_down"), AI.IMAGE_H, AI.IMAGE_W), "edge": (AI.get("edge")[0],) + EDGE_SIZE,
            "empty": (AI.get("empty"), 7, 70), "word_dirty": (WI.get("word_dirty"), 37, 70), "negative": (WI.get("negative"), 37, 70)}


def paint(pm, H, W, values, order, background):
    """The backward painting loop written out, independent of mnc_amd.labels: pixels inside the image, bit by bit from dense()."""
    out = np.full((H, W), background, np.int64)
    for i in list(order)[::-1]:
        h, w = pm.size(i)
        if h == 0 or w == 0:
            continue
        x1, y1 = int(pm.bounds[i][0]), int(pm.bounds[i][1])
        ys, xs = np.nonzero(pm.dense(i))
        ys, xs = ys + y1, xs + x1
        ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
        out[ys[ok], xs[ok]] = values[i]
    return out


def disjoint_ref(pm, H, W):
    """What round trip 2 must give: the layered set cropped to the image, its empty instances dropped -> (PackedMasks, kept)."""
    def make():
        cut = AI.AL.combine_numpy(AI.AL.layer_numpy(pm), None, "copy", (0, 0, W - 1, H - 1))
        kept = np.nonzero(cut.areas > 0)[0]
        return cut.take(kept), kept
    return reference(("disjoint", id(pm), H, W), make)
