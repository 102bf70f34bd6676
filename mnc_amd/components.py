"""Connected components of packed instance masks, and what is built on them (include/mnc_hip.h n12, csrc/mask_components.hip) on
mnc_amd.masks.PackedMasks: the component table, the selection by area, the filling of holes, one instance per region.

    label_numpy(m, connectivity=8)                 bool [h, w] -> (labels int32 [h, w], count): the rule on one dense mask
    components_numpy(pm, connectivity=8)           -> Components(comp_ptr, area, bbox, anchor)
    select_numpy(pm, connectivity=8, min_area=1, keep=0)   -> PackedMasks: the components that stay
    fill_holes_numpy(pm, connectivity=4)           -> PackedMasks: the masks OR their holes
    split_numpy(pm, connectivity=8)                -> (PackedMasks, source): one instance per component
    components / select / fill_holes / split       the same through mnc_mask_components / _select / _fill_holes / _split (the GPU);
                                                   PackedMasks.components / .select / .fill_holes / .split are the methods

The rule.  A component of instance i is a maximal set of its set pixels connected under `connectivity` 4 (edge neighbours) or 8
(edge and corner neighbours).  Padding bits of the input are not trusted; pixels outside the instance's bounds are background; an
instance without rows has no components.  The components of an instance are numbered by their first pixel in row-major order
(lowest y, then lowest x), which is also scipy.ndimage.label's numbering; the components of a set are those of instance 0, then of
instance 1, ...: instance i has the components comp_ptr[i] .. comp_ptr[i + 1] - 1.

    Components   comp_ptr int64 [n + 1]; area int64 [C]; bbox int32 [C, 4] (x1, y1, x2, y2 in image coordinates, inclusive and
                 tight); anchor int32 [C, 2] (x, y of the first pixel)
    select       a component stays when its area is >= min_area and, with keep > 0, it is among the `keep` largest of its instance
                 (larger area first, equal areas to the lower number).  The result has the input's bounds (not tightened) and
                 offsets, its areas are the true bit counts, its padding bits are 0 (as is every word of the bits outside the rows),
                 classes and scores are carried over.  select(min_area=1, keep=0) is the input with its padding cleared.  The rows
                 of the input must stand in order without overlap.
    fill_holes   `connectivity` is that of the BACKGROUND.  A hole is a background component of the instance's box that is not
                 connected to the outside of the box: pad the complement with a frame of one background pixel and drop the component
                 that holds the frame.  The result is the mask OR its holes, in the layout of select
                 (scipy.ndimage.binary_fill_holes with the 4- or 8-neighbour structure).
    split        every component becomes an instance with tight bounds, in component order, offsets in order without gaps; class and
                 score are those of the instance it came from, source int32 [C] is that instance's index.

There is no fallback: without the library or a GPU the device functions raise.  They read host arrays: a device-resident
PackedMasks (engine results) is fetched to the host first."""
import collections
import ctypes

import numpy as np

from . import _lib
from .masks import PackedMasks, _device_id, _set_args, pack_rows, row_words

MAX_N = 2048
MAX_WORDS = 2 ** 25
INVALID = 1

Components = collections.namedtuple("Components", "comp_ptr area bbox anchor")


def _check(who, connectivity, min_area=0, keep=0):
    connectivity, min_area, keep = int(connectivity), int(min_area), int(keep)
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity=%d is not 4 or 8" % (who, connectivity))
    if min_area < 0 or keep < 0:
        raise ValueError("%s: min_area=%d or keep=%d is negative" % (who, min_area, keep))
    return connectivity, min(min_area, 2 ** 31 - 1), min(keep, 2 ** 31 - 1)


def _check_set(who, pm, frame=0, ordered=False):
    """What the library refuses about the set beyond HostMaskSet::check: the count, the words, and (ordered) rows out of order."""
    n = len(pm)
    if n > MAX_N:
        raise ValueError("%s: n=%d not in [0, %d]" % (who, n, MAX_N))
    words, end = 0, 0
    for i in range(n):
        h, w = pm.size(i)
        if h == 0 or w == 0:
            continue
        words += row_words(h + 2 * frame, w + 2 * frame)
        if words > MAX_WORDS:
            raise ValueError("%s: more than %d words of rows in the set (at masks[%d])" % (who, MAX_WORDS, i))
        if ordered:
            if int(pm.offsets[i]) < end:
                raise ValueError("%s: the rows of masks[%d] (offset %d) begin before the end of the rows before (%d)"
                                 % (who, i, int(pm.offsets[i]), end))
            end = int(pm.offsets[i]) + row_words(h, w) * 8


def _runs(m):
    """The runs of a dense mask in raster order -> (y, x0, x1) int64 arrays, x1 inclusive."""
    h, w = m.shape
    p = np.zeros((h, w + 2), np.int8)
    p[:, 1:-1] = m
    d = np.diff(p, axis=1)
    y, x0 = np.nonzero(d == 1)
    _, x1 = np.nonzero(d == -1)
    return y.astype(np.int64), x0.astype(np.int64), x1.astype(np.int64) - 1


def _label_runs(y, x0, x1, connectivity):
    """-> (comp int64 [runs], count): the component of every run, numbered by the first run (= the first pixel) of each."""
    e = 1 if connectivity == 8 else 0
    n = len(y)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    row_lo = np.searchsorted(y, np.arange(int(y[-1]) + 2)) if n else np.zeros(1, np.int64)
    for r in range(1, len(row_lo) - 1):
        a, a_end, b, b_end = int(row_lo[r - 1]), int(row_lo[r]), int(row_lo[r]), int(row_lo[r + 1])
        while a < a_end and b < b_end:                            # runs of the row above against the runs of this row
            if x1[a] + e >= x0[b] and x0[a] - e <= x1[b]:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)             # the smaller id is the root: the component's first run
            if x1[a] < x1[b]:
                a += 1
            else:
                b += 1
    root = np.array([find(k) for k in range(n)], np.int64)
    is_root = root == np.arange(n)
    number = np.cumsum(is_root) - 1
    return number[root] if n else np.zeros(0, np.int64), int(is_root.sum())


def label_numpy(m, connectivity=8):
    """bool [h, w] -> (labels int32 [h, w] with 0 the background and 1 .. count the components in first-pixel order, count)."""
    connectivity = _check("label_numpy", connectivity)[0]
    m = np.asarray(m, bool)
    h, w = m.shape
    y, x0, x1 = _runs(m)
    comp, count = _label_runs(y, x0, x1, connectivity)
    d = np.zeros((h, w + 1), np.int64)
    np.add.at(d, (y, x0), comp + 1)
    np.add.at(d, (y, x1 + 1), -(comp + 1))
    return np.cumsum(d, axis=1)[:, :w].astype(np.int32), count


def _table(m, connectivity, x1, y1):
    """One dense mask at (x1, y1) -> (area, bbox, anchor) of its components."""
    y, a, b = _runs(m)
    comp, count = _label_runs(y, a, b, connectivity)
    area = np.bincount(comp, weights=None if not len(comp) else (b - a + 1), minlength=count).astype(np.int64)
    bbox = np.zeros((count, 4), np.int64)
    bbox[:, :2], bbox[:, 2:] = 2 ** 40, -2 ** 40
    np.minimum.at(bbox[:, 0], comp, a + x1)
    np.minimum.at(bbox[:, 1], comp, y + y1)
    np.maximum.at(bbox[:, 2], comp, b + x1)
    np.maximum.at(bbox[:, 3], comp, y + y1)
    first = np.unique(comp, return_index=True)[1] if count else np.zeros(0, np.int64)
    anchor = np.stack((a[first] + x1, y[first] + y1), axis=1) if count else np.zeros((0, 2), np.int64)
    return area, bbox.astype(np.int32), anchor.astype(np.int32)


def components_numpy(pm, connectivity=8):
    """The component table as a plain loop on the host -- the specification csrc/mask_components.hip is tested against."""
    connectivity = _check("components_numpy", connectivity)[0]
    _check_set("components_numpy", pm)
    n = len(pm)
    comp_ptr, areas, boxes, anchors = np.zeros(n + 1, np.int64), [], [], []
    for i in range(n):
        h, w = pm.size(i)
        if h and w:
            area, bbox, anchor = _table(pm.dense(i), connectivity, int(pm.bounds[i][0]), int(pm.bounds[i][1]))
            areas.append(area), boxes.append(bbox), anchors.append(anchor)
            comp_ptr[i + 1] = len(area)
    np.cumsum(comp_ptr, out=comp_ptr)
    return Components(comp_ptr, np.concatenate(areas) if areas else np.zeros(0, np.int64),
                      np.concatenate(boxes) if boxes else np.zeros((0, 4), np.int32),
                      np.concatenate(anchors) if anchors else np.zeros((0, 2), np.int32))


def _rewritten(pm, make):
    """The layout of select and fill_holes: make(dense mask) per instance with rows, written where the input's rows stand."""
    n = len(pm)
    bits, areas = np.zeros(pm.bits.size, np.uint64), np.zeros(n, np.int64)
    for i in range(n):
        h, w = pm.size(i)
        if h and w:
            b = make(pm.dense(i))
            words = pack_rows(b)
            lo = int(pm.offsets[i]) // 8
            bits[lo:lo + len(words)] = words
            areas[i] = int(b.sum())
    return PackedMasks(pm.bounds.copy(), pm.offsets.copy(), areas, pm.classes.copy(), pm.scores.copy(), bits)


def select_numpy(pm, connectivity=8, min_area=1, keep=0):
    """The selection as a plain loop on the host.  Raises ValueError where mnc_mask_select returns MNC_ERR_INVALID for its
    parameters, the instance count, the words or the order of the rows."""
    connectivity, min_area, keep = _check("select_numpy", connectivity, min_area, keep)
    _check_set("select_numpy", pm, ordered=True)

    def make(m):
        labels, count = label_numpy(m, connectivity)
        area = np.bincount(labels.reshape(-1), minlength=count + 1)[1:]
        stay = area >= min_area
        if keep > 0:
            order = np.argsort(-area, kind="stable")              # larger area first, equal areas to the lower number
            among = np.zeros(count, bool)
            among[order[:keep]] = True
            stay &= among
        return np.concatenate(([False], stay))[labels]

    return _rewritten(pm, make)


def fill_holes_numpy(pm, connectivity=4):
    """The filling of holes as a plain loop on the host; `connectivity` is the background's."""
    connectivity = _check("fill_holes_numpy", connectivity)[0]
    _check_set("fill_holes_numpy", pm, frame=1, ordered=True)

    def make(m):
        h, w = m.shape
        outside = np.ones((h + 2, w + 2), bool)
        outside[1:-1, 1:-1] = ~m
        labels, _ = label_numpy(outside, connectivity)
        return m | ((labels != labels[0, 0]) & outside)[1:-1, 1:-1]

    return _rewritten(pm, make)


def split_numpy(pm, connectivity=8):
    """One instance per component as a plain loop on the host -> (PackedMasks, source int32 [C])."""
    connectivity = _check("split_numpy", connectivity)[0]
    _check_set("split_numpy", pm)
    bounds, dense, source = [], [], []
    for i in range(len(pm)):
        h, w = pm.size(i)
        if not (h and w):
            continue
        m = pm.dense(i)
        labels, count = label_numpy(m, connectivity)
        ax, ay = int(pm.bounds[i][0]), int(pm.bounds[i][1])
        for c in range(1, count + 1):
            part = labels == c
            ys, xs = np.nonzero(part.any(axis=1))[0], np.nonzero(part.any(axis=0))[0]
            dense.append(part[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1])
            bounds.append([ax + xs[0], ay + ys[0], ax + xs[-1], ay + ys[-1]])
            source.append(i)
    source = np.array(source, np.int32)
    return PackedMasks.from_dense(np.array(bounds, np.int32).reshape(-1, 4), dense, pm.classes[source], pm.scores[source]), source


# ---- the device ----

def _host(pm):
    """A PackedMasks whose arrays are on the host (a device-resident result is fetched: there are no *_dev forms of n12)."""
    return pm.fetch()


def components_call(pm, connectivity, cap, device_id=0, sizes_only=False):
    """mnc_mask_components as it is, with room for `cap` components -> (Components with arrays of `cap` rows, C).  Too little room
    raises _lib.MncError (MNC_ERR_INVALID); sizes_only passes no table at all."""
    n = len(pm)
    comp_ptr = np.zeros(n + 1, np.int64)
    area, bbox, anchor = np.zeros(cap, np.int64), np.zeros((cap, 4), np.int32), np.zeros((cap, 2), np.int32)
    count = ctypes.c_size_t(0)
    try:
        _lib.call("mnc_mask_components", *(_set_args(pm, areas=False) + (
            int(connectivity), _lib.ptr(comp_ptr), None if sizes_only else _lib.ptr(area), _lib.ptr(bbox), _lib.ptr(anchor), int(cap),
            ctypes.addressof(count), int(device_id))))
    except _lib.MncError as e:
        e.needed = int(count.value)
        raise
    return Components(comp_ptr, area, bbox, anchor), int(count.value)


def components(pm, connectivity=8, device_id=None):
    """components_numpy on the GPU (mnc_mask_components): the same Components field by field.  One call with room for 64 + 16 n
    components, a second one when the masks have more.  Invalid arguments raise ValueError, invalid sets _lib.MncError
    (MNC_ERR_INVALID), before anything is launched.  A device-resident PackedMasks is fetched to the host first."""
    connectivity = _check("components", connectivity)[0]
    pm = _host(pm)
    dev = _device_id(device_id)
    cap = 64 + 16 * len(pm)
    try:
        t, C = components_call(pm, connectivity, cap, dev)
    except _lib.MncError as e:
        if e.code != INVALID or e.needed <= cap:
            raise
        t, C = components_call(pm, connectivity, e.needed, dev)
    return Components(t.comp_ptr, t.area[:C].copy(), t.bbox[:C].copy(), t.anchor[:C].copy())


def _rewrite(name, pm, head, device_id):
    pm = _host(pm)
    bits, areas = np.zeros(max(pm.bits.size, 1), np.uint64), np.zeros(len(pm), np.int64)
    _lib.call(name, *(_set_args(pm, areas=False) + head + (_lib.ptr(areas), _lib.ptr(bits), int(pm.bits.nbytes), _device_id(device_id))))
    return PackedMasks(pm.bounds.copy(), pm.offsets.copy(), areas, pm.classes.copy(), pm.scores.copy(), bits[:pm.bits.size])


def select(pm, connectivity=8, min_area=1, keep=0, device_id=None):
    """select_numpy on the GPU (mnc_mask_select): the same PackedMasks field by field.  Invalid arguments raise ValueError, invalid
    sets _lib.MncError (MNC_ERR_INVALID), before anything is launched.  A device-resident PackedMasks is fetched to the host first."""
    return _rewrite("mnc_mask_select", pm, _check("select", connectivity, min_area, keep), device_id)


def fill_holes(pm, connectivity=4, device_id=None):
    """fill_holes_numpy on the GPU (mnc_mask_fill_holes); see select."""
    return _rewrite("mnc_mask_fill_holes", pm, _check("fill_holes", connectivity)[:1], device_id)


def split_call(pm, connectivity, cap, bits, device_id=0):
    """mnc_mask_split as it is, with room for `cap` components and the words `bits` (None: the sizes only) -> (bounds, offsets,
    areas, source, C, bytes).  Too little room raises _lib.MncError (MNC_ERR_INVALID) with .needed = (C, bytes)."""
    bounds, offsets = np.zeros((cap, 4), np.int32), np.zeros(cap, np.int64)
    areas, source = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
    count, nbytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    try:
        _lib.call("mnc_mask_split", *(_set_args(pm, areas=False) + (
            int(connectivity), _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(source), int(cap), ctypes.addressof(count),
            _lib.ptr(bits), bits.nbytes if bits is not None else 0, ctypes.addressof(nbytes), int(device_id))))
    except _lib.MncError as e:
        e.needed = (int(count.value), int(nbytes.value))
        raise
    return bounds, offsets, areas, source, int(count.value), int(nbytes.value)


def split(pm, connectivity=8, device_id=None):
    """split_numpy on the GPU (mnc_mask_split): the same (PackedMasks, source) field by field.  One call with room for 64 + 16 n
    components and twice the input's words, a second one when the result is larger.  Invalid arguments raise ValueError, invalid sets
    _lib.MncError (MNC_ERR_INVALID), before anything is launched.  A device-resident PackedMasks is fetched to the host first."""
    connectivity = _check("split", connectivity)[0]
    pm = _host(pm)
    dev = _device_id(device_id)
    cap, bits = 64 + 16 * len(pm), np.zeros(2 * pm.bits.size + 64, np.uint64)
    try:
        out = split_call(pm, connectivity, cap, bits, dev)
    except _lib.MncError as e:
        if e.code != INVALID or (e.needed[0] <= cap and e.needed[1] <= bits.nbytes):
            raise
        cap, bits = max(e.needed[0], 1), np.zeros(e.needed[1] // 8 + 1, np.uint64)
        out = split_call(pm, connectivity, cap, bits, dev)
    bounds, offsets, areas, source, C, nbytes = out
    source = source[:C].copy()
    return PackedMasks(bounds[:C].copy(), offsets[:C].copy(), areas[:C].copy(), pm.classes[source], pm.scores[source],
                       bits[:nbytes // 8].copy()), source


def timing(on):
    """mnc_mask_components_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_components_timing", on)
