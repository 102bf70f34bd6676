"""Label maps in and out of packed instance masks (include/mnc_hip.h n19, csrc/mask_labels.hip) on mnc_amd.masks.PackedMasks: the
format SBD's inst / cls arrays, Cityscapes' instanceIds, COCO panoptic PNGs and superpixel maps come in, and the one a panoptic
result goes out in.

    from_labels_numpy(label, cls=None, background=0, classes=None)   -> (PackedMasks, ids int32 [n]): the CPU statement
    to_labels_numpy(pm, H, W, values=None, order=None, background=0) -> int32 [H, W]: the CPU statement
    from_labels / to_labels                                          the same through mnc_label_table + mnc_label_masks resp.
                                                                     mnc_mask_to_labels (the GPU); PackedMasks.from_labels /
                                                                     .to_labels are the methods
    id_to_rgb(ids) / rgb_to_id(rgb)                                  the published panoptic id rule, id = R + 256 G + 65536 B
    segments_info(pm, ids)                                           [{"id", "category_id", "area", "bbox", "iscrowd"}]

The rules.  A label map is an integer array [H, W] with values in [0, 2^24), H and W in [1, 32768], H * W <= 2^26.

    from_labels   background is one value, a sequence of at most 8 values, or None (every value is an instance; VOC's object PNGs
                  want (0, 255)).  The instances are the distinct values that are not background, ascending -- np.unique's order
                  and utils.voc_eval.parse_inst's.  Instance k has ids[k] as its value, the tight box of its pixels, its pixel
                  count and its bits, offsets in order without gaps, padding bits 0: what PackedMasks.from_dense gives for the
                  same boxes and arrays.  Scores are 0.  Classes: with cls, a map of the same shape, the value of cls on the
                  instance's pixels (values that differ raise ValueError naming the smallest such id: the reference's assert);
                  with classes, a dict or an array looked up by id on the host (a missing id raises ValueError); else 0.  More
                  than 2048 instances raise ValueError.
    to_labels     a pixel gets values[i] (None: i + 1; any int32, pm.classes gives the semantic map) of the first instance i in
                  `order` that has it set, `background` where none has: the painting loop run over the order backwards.  order
                  None is algebra.score_order(pm.scores), layered()'s; an explicit one is a permutation.  A mask is empty outside
                  its bounds, bounds may be negative or unclipped and what lies outside the image is dropped, padding bits are not
                  trusted, an instance without rows paints nothing, no instance gives a map of background.

There is no fallback: without the library or a GPU the device functions raise.  They read host arrays: a device-resident
PackedMasks (engine results) is fetched to the host first."""
import ctypes

import numpy as np

from . import _lib
from .algebra import _check_order
from .masks import MAX_SIDE, PackedMasks, _device_id, _set_args

MAX_N = 2048
MAX_ID = 2 ** 24
MAX_PIXELS = 2 ** 26
MAX_SKIP = 8
_EMPTY = (0, 0, -1, -1)


def _check_image(who, H, W):
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("%s: image %d x %d not in [1, %d]" % (who, H, W, MAX_SIDE))
    if H * W > MAX_PIXELS:
        raise ValueError("%s: %d pixels (limit %d)" % (who, H * W, MAX_PIXELS))
    return H, W


def _check_map(who, label, name="label"):
    """-> the map as it was given, checked: two-dimensional, an integer type, inside the size limits."""
    label = np.asarray(label)
    if label.ndim != 2 or label.dtype.kind not in "iub":
        raise ValueError("%s: %s is not an integer array [H, W] (shape %s, dtype %s)" % (who, name, label.shape, label.dtype))
    _check_image(who, *label.shape)
    return label


def _check_range(who, label):
    lo, hi = int(label.min()), int(label.max())
    if lo < 0 or hi >= MAX_ID:
        raise ValueError("%s: label value %d not in [0, %d)" % (who, lo if lo < 0 else hi, MAX_ID))


def _skip(who, background):
    """-> int32 [n_skip]: the background values, those the map cannot hold dropped."""
    if background is None:
        return np.zeros(0, np.int32)
    skip = [int(v) for v in np.asarray(background).reshape(-1)]
    if len(skip) > MAX_SKIP:
        raise ValueError("%s: %d background values (limit %d)" % (who, len(skip), MAX_SKIP))
    return np.array([v for v in skip if 0 <= v < MAX_ID], np.int32)


def _lookup_classes(who, classes, ids):
    out = np.zeros(len(ids), np.int32)
    table = None if isinstance(classes, dict) else np.asarray(classes).reshape(-1)
    for k, i in enumerate(int(v) for v in ids):
        if table is None:
            if i not in classes:
                raise ValueError("%s: classes has no entry for id %d" % (who, i))
            out[k] = classes[i]
        else:
            if i >= table.size:
                raise ValueError("%s: classes has no entry for id %d" % (who, i))
            out[k] = table[i]
    return out


def _classes_of(who, ids, cls_lo, cls_hi, cls, classes):
    if cls is not None:
        mixed = np.nonzero(cls_lo != cls_hi)[0]
        if mixed.size:
            raise ValueError("%s: instance %d has pixels of more than one class" % (who, int(ids[mixed[0]])))
        return np.asarray(cls_lo, np.int32)
    if classes is not None:
        return _lookup_classes(who, classes, ids)
    return np.zeros(len(ids), np.int32)


def _check_cls(who, label, cls, classes):
    if cls is None:
        return None
    if classes is not None:
        raise ValueError("%s: both cls and classes given" % who)
    cls = _check_map(who, cls, "cls")
    if cls.shape != label.shape:
        raise ValueError("%s: cls %s does not have the shape of label %s" % (who, cls.shape, label.shape))
    if cls.size and (int(cls.min()) < -2 ** 31 or int(cls.max()) >= 2 ** 31):
        raise ValueError("%s: cls does not fit int32" % who)
    return cls


# ---- the statements ----

def from_labels_numpy(label, cls=None, background=0, classes=None):
    """The instances of a label map as plain numpy on the host -- the specification csrc/mask_labels.hip is tested against.
    -> (PackedMasks, ids int32 [n]).  Raises ValueError where from_labels does."""
    who = "from_labels_numpy"
    label = _check_map(who, label)
    cls = _check_cls(who, label, cls, classes)
    _check_range(who, label)
    skip = _skip(who, background)
    ids = np.setdiff1d(np.unique(label), skip).astype(np.int32)
    if ids.size > MAX_N:
        raise ValueError("%s: the map has %d instances (limit %d)" % (who, ids.size, MAX_N))
    bounds, dense = np.zeros((ids.size, 4), np.int32), []
    cls_lo, cls_hi = np.zeros(ids.size, np.int64), np.zeros(ids.size, np.int64)
    for k, i in enumerate(ids):
        m = label == i
        ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
        bounds[k] = (xs[0], ys[0], xs[-1], ys[-1])
        dense.append(m[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1])
        if cls is not None:
            cls_lo[k], cls_hi[k] = cls[m].min(), cls[m].max()
    return PackedMasks.from_dense(bounds, dense, _classes_of(who, ids, cls_lo, cls_hi, cls, classes), None), ids


def _values(who, pm, values):
    if values is None:
        return np.arange(1, len(pm) + 1, dtype=np.int32)
    v = np.asarray(values).reshape(-1)
    if v.size != len(pm) or v.dtype.kind not in "iub":
        raise ValueError("%s: values is not an integer array of %d entries" % (who, len(pm)))
    if v.size and (int(v.min()) < -2 ** 31 or int(v.max()) >= 2 ** 31):
        raise ValueError("%s: a value does not fit int32" % who)
    return np.ascontiguousarray(v, np.int32)


def _int32(who, name, v):
    v = int(v)
    if not -2 ** 31 <= v < 2 ** 31:
        raise ValueError("%s: %s=%d does not fit int32" % (who, name, v))
    return v


def to_labels_numpy(pm, H, W, values=None, order=None, background=0):
    """The label map of a set as plain numpy on the host -- the specification csrc/mask_labels.hip is tested against: the
    instances painted over one another, the order run backwards so that its first instance ends on top.  -> int32 [H, W]."""
    who = "to_labels_numpy"
    H, W = _check_image(who, H, W)
    if len(pm) > MAX_N:
        raise ValueError("%s: n=%d not in [0, %d]" % (who, len(pm), MAX_N))
    values = _values(who, pm, values)
    order = _check_order(who, pm, order)
    out = np.full((H, W), _int32(who, "background", background), np.int32)
    for i in (int(v) for v in order[::-1]):
        out[pm.full(i, H, W)] = values[i]
    return out


# ---- the device ----

def label_table(label, cls=None, skip=(), cap=MAX_N, device_id=None):
    """mnc_label_table as it is: label (and cls) int32 [H, W], C-contiguous -> (n, ids, bounds, areas, cls_lo, cls_hi, bits_bytes)
    with the arrays cut to n.  More than cap instances raise ValueError naming their number."""
    H, W = label.shape
    skip = np.ascontiguousarray(skip, np.int32).reshape(-1)
    cap = int(cap)
    room = max(cap, 1)
    ids, bounds, areas = np.zeros(room, np.int32), np.zeros((room, 4), np.int32), np.zeros(room, np.int64)
    cls_lo, cls_hi = np.zeros(room, np.int32), np.zeros(room, np.int32)
    n, need = ctypes.c_int(-1), ctypes.c_size_t(0)
    try:
        _lib.call("mnc_label_table", _lib.ptr(label), _lib.ptr(cls), int(H), int(W), _lib.ptr(skip) if skip.size else None,
                  int(skip.size), cap, ctypes.addressof(n), _lib.ptr(ids), _lib.ptr(bounds), _lib.ptr(areas), _lib.ptr(cls_lo),
                  _lib.ptr(cls_hi), ctypes.addressof(need), _device_id(device_id))
    except _lib.MncError as e:
        if n.value > min(cap, MAX_N):
            raise ValueError("label_table: the map has %d instances (limit %d)" % (n.value, min(cap, MAX_N)))
        raise e
    k = n.value
    return k, ids[:k].copy(), bounds[:k].copy(), areas[:k].copy(), cls_lo[:k].copy(), cls_hi[:k].copy(), int(need.value)


def label_masks(label, ids, bounds, bits_bytes, device_id=None):
    """mnc_label_masks as it is -> bits uint64 [bits_bytes / 8]."""
    H, W = label.shape
    bits = np.zeros(max(bits_bytes // 8, 1), np.uint64)
    used = ctypes.c_size_t(0)
    _lib.call("mnc_label_masks", _lib.ptr(label), int(H), int(W), _lib.ptr(ids), _lib.ptr(bounds), len(ids), _lib.ptr(bits),
              int(bits_bytes), ctypes.addressof(used), _device_id(device_id))
    return bits[:used.value // 8]


def from_labels(label, cls=None, background=0, classes=None, device_id=None):
    """from_labels_numpy on the GPU (mnc_label_table, then mnc_label_masks with the table): the same (PackedMasks, ids) field by
    field.  What the rule refuses raises ValueError; the map is uploaded by each of the two calls."""
    who = "from_labels"
    label = _check_map(who, label)
    cls = _check_cls(who, label, cls, classes)
    if label.dtype != np.int32:
        _check_range(who, label)                              # (before the cast, which would wrap a value past int32)
    label = np.ascontiguousarray(label, np.int32)
    if cls is not None:
        cls = np.ascontiguousarray(cls, np.int32)
    skip = _skip(who, background)
    try:
        n, ids, bounds, areas, cls_lo, cls_hi, need = label_table(label, cls, skip, MAX_N, device_id)
    except _lib.MncError as e:
        if e.code == 1 and "not in [0," in str(e) and "label[" in str(e):
            raise ValueError(str(e))
        raise
    classes = _classes_of(who, ids, cls_lo, cls_hi, cls, classes)
    bits = label_masks(label, ids, bounds, need, device_id) if n else np.zeros(0, np.uint64)
    offsets = np.zeros(n, np.int64)
    if n:
        rows = (bounds[:, 3] - bounds[:, 1] + 1).astype(np.int64) * ((bounds[:, 2] - bounds[:, 0] + 64) // 64) * 8
        offsets[1:] = np.cumsum(rows)[:-1]
    return PackedMasks(bounds, offsets, areas, classes, None, bits), ids


def to_labels(pm, H, W, values=None, order=None, background=0, device_id=None):
    """to_labels_numpy on the GPU (mnc_mask_to_labels): the same int32 [H, W].  The order by scores is made by the library.  A
    device-resident set is fetched to the host first."""
    who = "to_labels"
    H, W = _check_image(who, H, W)
    pm = pm.fetch()
    n = len(pm)
    values = _values(who, pm, values)
    if order is not None:
        order = np.ascontiguousarray(order, np.int32).reshape(-1)
        if order.size != n:
            raise ValueError("%s: order has %d entries for %d instances" % (who, order.size, n))
        if n == 0:
            order = None
    scores = pm.scores if n else np.zeros(1, np.float32)
    out = np.zeros((H, W), np.int32)
    _lib.call("mnc_mask_to_labels", *(_set_args(pm, areas=False) + (_lib.ptr(scores), _lib.ptr(order),
                                                                    _lib.ptr(values) if n else None,
                                                                    _int32(who, "background", background), H, W, _lib.ptr(out),
                                                                    _device_id(device_id))))
    return out


def timing(on):
    """mnc_mask_labels_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_labels_timing", on)


# ---- the panoptic format ----

def id_to_rgb(ids):
    """Segment ids in [0, 2^24) -> uint8 [..., 3]: id = R + 256 G + 65536 B, the published panoptic rule."""
    ids = np.asarray(ids)
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= MAX_ID):
        raise ValueError("id_to_rgb: id not in [0, %d)" % MAX_ID)
    ids = ids.astype(np.int64)
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


def rgb_to_id(rgb):
    """uint8 [..., 3] -> int32 [...]: R + 256 G + 65536 B."""
    rgb = np.asarray(rgb).astype(np.int32)
    return rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]


def segments_info(pm, ids):
    """The `segments_info` list of a panoptic annotation for the instances of from_labels (or any set with its ids): per instance
    id, category_id (its class), area, bbox = [x, y, w, h] of its bounds, iscrowd 0."""
    ids = np.asarray(ids).reshape(-1)
    if ids.size != len(pm):
        raise ValueError("segments_info: %d ids for %d instances" % (ids.size, len(pm)))
    out = []
    for k in range(len(pm)):
        x1, y1, x2, y2 = (int(v) for v in pm.bounds[k])
        out.append({"id": int(ids[k]), "category_id": int(pm.classes[k]), "area": int(pm.areas[k]),
                    "bbox": [x1, y1, max(x2 - x1 + 1, 0), max(y2 - y1 + 1, 0)], "iscrowd": 0})
    return out
