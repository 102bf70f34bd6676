"""The set algebra of packed instance masks: and, or, xor, minus, copy and complement of two sets instance by instance, the union
or intersection of groups of instances, and the layering of a set into disjoint instances (include/mnc_hip.h n17,
csrc/mask_algebra.hip) on mnc_amd.masks.PackedMasks.

    combine_numpy(a, b, op, window=None)                    -> PackedMasks: the CPU statement of a op b, instance by instance
    merge_numpy(pm, group_ptr, members, intersect=False)    -> PackedMasks: one instance per group, its members' union or intersection
    layer_numpy(pm, order=None)                             -> PackedMasks: instance i minus every instance before it in the order
    score_order(scores)                                     the order layer uses by default: descending score, lower index first
    class_groups(classes)                                   -> (distinct classes ascending, [indices of each]): merge(by="class")
    groups_csr(groups)                                      a list of index lists -> (group_ptr int64 [G + 1], members int32)
    combine / merge / layer                                 the same through mnc_mask_combine / _merge / _layer (the GPU);
                                                            PackedMasks.combine / & | ^ - / .tighten / .crop / .complement /
                                                            .merge / .layered are the methods

The rules.  All of it is frame-free integer set arithmetic on lattice pixels: a mask is the set of its pixels in image
coordinates, empty outside its bounds; bounds may be negative or unclipped; padding bits of the input are not trusted.

    combine   per instance: instance i of a with instance i of b (len(b) == len(a)) or with b's only instance (len(b) == 1).
              op "and", "or", "xor", "minus" (a & ~b); "copy": b is not looked at, the result is a (tightened, or cropped by the
              window); "not": b is not looked at, the result is the complement of a inside the window, which is required.
              window = (x1, y1, x2, y2), inclusive: the result is intersected with it.  Classes and scores are a's.
    merge     one instance per group: the union of the group's members, or their intersection with intersect.  members are indices
              into pm in any order, repeats allowed; an empty group gives an empty instance either way.  The class and score are
              the first member's, 0 and 0.0 for an empty group.
    layer     instance i minus the union of every instance before it in `order`; order None is score_order(pm.scores), the order
              mask_nms_numpy uses.  len(pm) instances in input index order, pairwise disjoint, their union unchanged.

Every result has the layout boundary() and the morphology give -- offsets in order, without gaps, multiples of 8; areas the true bit
counts; padding bits 0 -- and TIGHT bounds, the smallest box that holds the instance's set pixels, as from_rle gives; an instance
without a pixel gets (0, 0, -1, -1) and no rows.  There is no fallback: without the library or a GPU the device functions raise.
They read host arrays: a device-resident PackedMasks (engine results) is fetched to the host first."""
import ctypes

import numpy as np

from . import _lib
from .masks import MAX_COORD, PackedMasks, _device_id, _set_args

MAX_N = 2048
MAX_PIXELS = 2 ** 27
MAX_MEMBERS = 2 ** 20
OPS = ("and", "or", "xor", "minus", "copy", "not")
_EMPTY = (0, 0, -1, -1)


def _op(who, op):
    if isinstance(op, str):
        if op not in OPS:
            raise ValueError("%s: op=%r is not one of %s" % (who, op, ", ".join(OPS)))
        return OPS.index(op)
    op = int(op)
    if not 0 <= op < len(OPS):
        raise ValueError("%s: op=%d not in [0, %d]" % (who, op, len(OPS) - 1))
    return op


def _window(who, window, op):
    """-> None or a tuple of four ints; what mnc_mask_combine refuses about a window raises ValueError."""
    if window is None:
        if op == 5:
            raise ValueError("%s: op \"not\" needs a window" % who)
        return None
    w = tuple(int(v) for v in np.asarray(window).reshape(-1))
    if len(w) != 4:
        raise ValueError("%s: window %r is not (x1, y1, x2, y2)" % (who, window))
    if not all(-MAX_COORD < v < MAX_COORD for v in w):
        raise ValueError("%s: window %r leaves the coordinate range" % (who, w))
    if w[2] < w[0] or w[3] < w[1]:
        raise ValueError("%s: window %r is empty" % (who, w))
    return w


def _rows(pm, i):
    h, w = pm.size(i)
    return h > 0 and w > 0


def _box(pm, i):
    return tuple(int(v) for v in pm.bounds[i])


def _meet(p, q):
    return (max(p[0], q[0]), max(p[1], q[1]), min(p[2], q[2]), min(p[3], q[3]))


def _hull(p, q):
    return (min(p[0], q[0]), min(p[1], q[1]), max(p[2], q[2]), max(p[3], q[3]))


def _has(f):
    return f is not None and f[2] >= f[0] and f[3] >= f[1]


def _pixels(f):
    return (f[2] - f[0] + 1) * (f[3] - f[1] + 1) if _has(f) else 0


def _in_frame(pm, i, f):
    """bool [fh, fw]: the pixels of instance i inside the frame f (which has rows)."""
    out = np.zeros((f[3] - f[1] + 1, f[2] - f[0] + 1), bool)
    if not _rows(pm, i):
        return out
    b = _box(pm, i)
    m = _meet(b, f)
    if _has(m):
        out[m[1] - f[1]:m[3] - f[1] + 1, m[0] - f[0]:m[2] - f[0] + 1] = \
            pm.dense(i)[m[1] - b[1]:m[3] - b[1] + 1, m[0] - b[0]:m[2] - b[0] + 1]
    return out


def _tight(f, m):
    """A frame and its pixels -> (bounds, bool array or None): the smallest box of the set pixels."""
    if m is None or not m.any():
        return _EMPTY, None
    ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    y1, y2, x1, x2 = int(ys[0]), int(ys[-1]), int(xs[0]), int(xs[-1])
    return (f[0] + x1, f[1] + y1, f[0] + x2, f[1] + y2), m[y1:y2 + 1, x1:x2 + 1]


def _check_set(who, pm):
    if len(pm) > MAX_N:
        raise ValueError("%s: n=%d not in [0, %d]" % (who, len(pm), MAX_N))


def _check_frames(who, frames):
    if sum(_pixels(f) for f in frames) > MAX_PIXELS:
        raise ValueError("%s: more than %d pixels of loose-frame rows in the call" % (who, MAX_PIXELS))


def _packed(frames, dense, classes, scores):
    tight = [_tight(f, m) for f, m in zip(frames, dense)]
    return PackedMasks.from_dense(np.array([t[0] for t in tight], np.int32).reshape(len(tight), 4), [t[1] for t in tight],
                                  classes, scores)


def score_order(scores):
    """int64 [n]: descending score, the lower index first on equal scores (mask_nms_numpy's order).  A NaN raises ValueError."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    if np.isnan(scores).any():
        raise ValueError("score_order: NaN score")
    return np.argsort(-scores, kind="stable")


def class_groups(classes):
    """-> (the distinct classes ascending, int32 [K]; for each the indices that have it, ascending)."""
    classes = np.asarray(classes, np.int32).reshape(-1)
    distinct = np.unique(classes)
    return distinct, [np.nonzero(classes == c)[0] for c in distinct]


def groups_csr(groups):
    """A list of index lists -> (group_ptr int64 [G + 1], members int32 [group_ptr[G]])."""
    groups = [np.asarray(g, np.int64).reshape(-1) for g in groups]
    group_ptr = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(g) for g in groups], out=group_ptr[1:])
    members = np.concatenate(groups).astype(np.int32) if groups else np.zeros(0, np.int32)
    return group_ptr, np.ascontiguousarray(members, np.int32)


def _check_groups(who, n, group_ptr, members):
    group_ptr = np.ascontiguousarray(group_ptr, np.int64).reshape(-1)
    members = np.ascontiguousarray(members, np.int32).reshape(-1)
    if group_ptr.size < 1 or group_ptr[0] != 0 or (np.diff(group_ptr) < 0).any():
        raise ValueError("%s: group_ptr does not start at 0 or is not monotone" % who)
    if group_ptr.size - 1 > MAX_N:
        raise ValueError("%s: G=%d not in [0, %d]" % (who, group_ptr.size - 1, MAX_N))
    if group_ptr[-1] > MAX_MEMBERS or group_ptr[-1] > members.size:
        raise ValueError("%s: %d members (limit %d, given %d)" % (who, group_ptr[-1], MAX_MEMBERS, members.size))
    used = members[:int(group_ptr[-1])]
    if used.size and (used.min() < 0 or used.max() >= n):
        raise ValueError("%s: a member is outside [0, %d)" % (who, n))
    return group_ptr, members


def _check_order(who, pm, order):
    if order is None:
        return score_order(pm.scores)
    order = np.ascontiguousarray(order, np.int32).reshape(-1)
    if order.size != len(pm) or not np.array_equal(np.sort(order), np.arange(len(pm))):
        raise ValueError("%s: order is not a permutation of 0 .. %d" % (who, len(pm) - 1))
    return order


# ---- the statements ----

def combine_numpy(a, b, op, window=None):
    """a op b as a plain loop on the host -- the specification csrc/mask_algebra.hip is tested against.  -> PackedMasks.  Raises
    ValueError where mnc_mask_combine returns MNC_ERR_INVALID for op, the window, the counts or the pixels."""
    who = "combine_numpy"
    op = _op(who, op)
    window = _window(who, window, op)
    _check_set(who, a)
    n = len(a)
    nb = 0 if op >= 4 or b is None else len(b)
    if op < 4:
        if b is None and n:
            raise ValueError("%s: op %s needs a set b" % (who, OPS[op]))
        if nb not in (0, 1, n) or (nb == 0 and n):
            raise ValueError("%s: len(b)=%d is not 1 or len(a)=%d" % (who, nb, n))
        _check_set(who, b)
    frames, dense = [], []
    for i in range(n):
        k = 0 if nb == 1 else i
        fa = _box(a, i) if _rows(a, i) else None
        fb = _box(b, k) if op < 4 and _rows(b, k) else None
        if op == 0:
            f = _meet(fa, fb) if fa and fb else None
        elif op in (1, 2):
            f = _hull(fa, fb) if fa and fb else fa or fb
        elif op in (3, 4):
            f = fa
        else:
            f = window
        if f is not None and window is not None:
            f = _meet(f, window)
        frames.append(f)
    _check_frames(who, frames)
    for i, f in enumerate(frames):
        if not _has(f):
            dense.append(None)
            continue
        p = _in_frame(a, i, f)
        if op >= 4:
            dense.append(p if op == 4 else ~p)
            continue
        q = _in_frame(b, 0 if nb == 1 else i, f)
        dense.append((p & q, p | q, p ^ q, p & ~q)[op])
    return _packed(frames, dense, a.classes, a.scores)


def merge_numpy(pm, group_ptr, members, intersect=False):
    """The unions (intersections) of groups of instances as a plain loop on the host -> PackedMasks of len(group_ptr) - 1
    instances.  Raises ValueError where mnc_mask_merge returns MNC_ERR_INVALID for the groups, the count or the pixels."""
    who = "merge_numpy"
    _check_set(who, pm)
    group_ptr, members = _check_groups(who, len(pm), group_ptr, members)
    G = group_ptr.size - 1
    frames, dense = [], []
    classes, scores = np.zeros(G, np.int32), np.zeros(G, np.float32)
    for g in range(G):
        mem = [int(m) for m in members[int(group_ptr[g]):int(group_ptr[g + 1])]]
        if mem:
            classes[g], scores[g] = pm.classes[mem[0]], pm.scores[mem[0]]
        boxes = [_box(pm, m) for m in mem if _rows(pm, m)]
        f = None
        if boxes and (not intersect or len(boxes) == len(mem)):
            f = boxes[0]
            for q in boxes[1:]:
                f = _meet(f, q) if intersect else _hull(f, q)
        frames.append(f)
    _check_frames(who, frames)
    for g, f in enumerate(frames):
        if not _has(f):
            dense.append(None)
            continue
        mem = [int(m) for m in members[int(group_ptr[g]):int(group_ptr[g + 1])]]
        acc = _in_frame(pm, mem[0], f)
        for m in mem[1:]:
            acc = acc & _in_frame(pm, m, f) if intersect else acc | _in_frame(pm, m, f)
        dense.append(acc)
    return _packed(frames, dense, classes, scores)


def layer_numpy(pm, order=None):
    """Disjoint instances as a plain loop on the host: instance i minus the union of every instance before it in order (None:
    score_order(pm.scores)) -> PackedMasks in input index order.  Raises ValueError where mnc_mask_layer returns MNC_ERR_INVALID
    for the order, a NaN score, the count or the pixels."""
    who = "layer_numpy"
    _check_set(who, pm)
    order = _check_order(who, pm, order)
    n = len(pm)
    frames, dense, seen = [None] * n, [None] * n, []
    _check_frames(who, [_box(pm, i) for i in range(n) if _rows(pm, i)])
    for i in (int(v) for v in order):
        if not _rows(pm, i):
            continue
        f = frames[i] = _box(pm, i)
        m = _in_frame(pm, i, f)
        for k in seen:
            if _has(_meet(f, _box(pm, k))):
                m &= ~_in_frame(pm, k, f)
        dense[i] = m
        seen.append(i)
    return _packed(frames, dense, pm.classes, pm.scores)


# ---- the device ----

def _one_call(entry, args_before, n_out, device_id):
    """The two calls of an n17 entry: the bound of the result's bytes from the bounds alone (nothing is launched), then the one
    launching call with that much room -> (bounds, offsets, areas, bits) with bits cut to the bytes written."""
    bounds, offsets, areas = np.zeros((n_out, 4), np.int32), np.zeros(n_out, np.int64), np.zeros(n_out, np.int64)
    bound, used = ctypes.c_size_t(0), ctypes.c_size_t(0)

    def call(bits):
        _lib.call(entry, *(args_before + (_lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits),
                                          bits.nbytes if bits is not None else 0, ctypes.addressof(bound), ctypes.addressof(used),
                                          int(device_id))))
    call(None)
    bits = np.zeros(max(bound.value // 8, 1), np.uint64)
    call(bits)
    return bounds, offsets, areas, bits[:used.value // 8].copy() if used.value < bits.nbytes else bits


def combine(a, b, op, window=None, device_id=None):
    """combine_numpy on the GPU (mnc_mask_combine): the same PackedMasks field by field.  Invalid arguments raise ValueError,
    invalid sets _lib.MncError (MNC_ERR_INVALID), before anything is launched.  Device-resident sets are fetched to the host
    first."""
    who = "combine"
    op = _op(who, op)
    window = _window(who, window, op)
    a = a.fetch()
    b = None if op >= 4 or b is None else b.fetch()
    win = None if window is None else np.array(window, np.int32)
    args_b = (None, None, None, 0, 0) if b is None else _set_args(b, areas=False)
    bounds, offsets, areas, bits = _one_call("mnc_mask_combine", _set_args(a, areas=False) + args_b + (op, _lib.ptr(win)), len(a),
                                             _device_id(device_id))
    return PackedMasks(bounds, offsets, areas, a.classes, a.scores, bits)


def merge(pm, group_ptr, members, intersect=False, device_id=None):
    """merge_numpy on the GPU (mnc_mask_merge): the same PackedMasks field by field."""
    pm = pm.fetch()
    group_ptr = np.ascontiguousarray(group_ptr, np.int64).reshape(-1)
    members = np.ascontiguousarray(members, np.int32).reshape(-1)
    if group_ptr.size < 1:
        raise ValueError("merge: group_ptr is empty")
    G = group_ptr.size - 1
    mem = members if members.size else np.zeros(1, np.int32)
    bounds, offsets, areas, bits = _one_call("mnc_mask_merge", _set_args(pm, areas=False) + (
        _lib.ptr(group_ptr), _lib.ptr(mem), G, int(bool(intersect))), G, _device_id(device_id))
    classes, scores = np.zeros(G, np.int32), np.zeros(G, np.float32)
    first = np.nonzero(np.diff(group_ptr) > 0)[0]
    classes[first], scores[first] = pm.classes[members[group_ptr[first]]], pm.scores[members[group_ptr[first]]]
    return PackedMasks(bounds, offsets, areas, classes, scores, bits)


def layer(pm, order=None, device_id=None):
    """layer_numpy on the GPU (mnc_mask_layer): the same PackedMasks field by field.  The order by scores is made by the library."""
    pm = pm.fetch()
    n = len(pm)
    if order is not None:
        order = np.ascontiguousarray(order, np.int32).reshape(-1)
        if order.size != n:
            raise ValueError("layer: order has %d entries for %d instances" % (order.size, n))
        if n == 0:
            order = None
    scores = pm.scores if n else np.zeros(1, np.float32)
    bounds, offsets, areas, bits = _one_call("mnc_mask_layer", _set_args(pm, areas=False) + (_lib.ptr(scores), _lib.ptr(order)), n,
                                             _device_id(device_id))
    return PackedMasks(bounds, offsets, areas, pm.classes, pm.scores, bits)


def timing(on):
    """mnc_mask_algebra_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_algebra_timing", on)
