"""The contingency table of two integer label maps (include/mnc_hip.h n20, csrc/label_pairs.hip): for every pair of values (a, b)
that occurs at the same pixel, the number of such pixels.  It is what panoptic quality matches segments on (mnc_amd/panoptic.py),
the confusion matrix of a semantic result, and the answer to "which instance does each superpixel lie in".

    label_pairs_numpy(a, b)                                   -> LabelPairs: the CPU statement
    label_pairs(a, b, device_id=None)                         the same through mnc_label_pairs (the GPU), one call
    confusion(gt, pred, num_classes, ignore=255, device=True) -> int64 [C, C], rows gt, columns pred
    semantic_scores(conf)                                     -> pixel accuracy, mean accuracy, mIoU, frequency-weighted IoU

The rule.  a and b are integer arrays [H, W] of one shape with values in [0, 2^24), H and W in [1, 32768], H * W <= 2^26 -- the
limits of mnc_amd/labels.py.  No value is background: every value is a row (of a) or a column (of b).  The result equals
np.unique((a.astype(np.int64) << 24) | b, return_counts=True) split back into its fields:

    a_ids, b_ids   int32 [na], [nb]: the distinct values, ascending
    ia, ib         int32 [m]: the ranks into a_ids / b_ids of the m pairs that occur, sorted by (ia, ib) ascending
    count          int64 [m]: the pixels of each pair, always positive, summing to H * W

A map has at most 65536 distinct values and the table at most 2^22 cells (na * nb); beyond that ValueError names the numbers.

There is no fallback: without the library or a GPU the device functions raise."""
import ctypes

import numpy as np

from . import _lib
from .labels import MAX_ID, _check_map, _check_range
from .masks import _device_id

MAX_IDS = 65536
MAX_CELLS = 2 ** 22
LDS_CELLS = 16384         # csrc/label_pairs.hip kLpLdsCells: tables up to this size are counted per workgroup in LDS


class LabelPairs(object):
    """The table in compressed rows.  Everything here runs on the host."""
    FIELDS = ("a_ids", "b_ids", "ia", "ib", "count")

    def __init__(self, a_ids, b_ids, ia, ib, count):
        self.a_ids, self.b_ids = np.asarray(a_ids, np.int32), np.asarray(b_ids, np.int32)
        self.ia, self.ib, self.count = np.asarray(ia, np.int32), np.asarray(ib, np.int32), np.asarray(count, np.int64)

    def __len__(self):
        return int(self.count.size)

    @property
    def row_ptr(self):
        """int64 [na + 1]: the pairs of row r are row_ptr[r] .. row_ptr[r + 1]."""
        out = np.zeros(self.a_ids.size + 1, np.int64)
        np.cumsum(np.bincount(self.ia, minlength=self.a_ids.size), out=out[1:])
        return out

    @property
    def a_areas(self):
        """int64 [na]: the pixels of every value of a."""
        return _sums(self.ia, self.count, self.a_ids.size)

    @property
    def b_areas(self):
        return _sums(self.ib, self.count, self.b_ids.size)

    def dense(self):
        """int64 [na, nb]."""
        out = np.zeros((self.a_ids.size, self.b_ids.size), np.int64)
        out[self.ia, self.ib] = self.count
        return out

    def get(self, a_value, b_value):
        """The pixels where a == a_value and b == b_value; 0 for a pair, or a value, that does not occur."""
        r, c = _find(self.a_ids, a_value), _find(self.b_ids, b_value)
        if r < 0 or c < 0:
            return 0
        ptr = self.row_ptr
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        k = lo + int(np.searchsorted(self.ib[lo:hi], c))
        return int(self.count[k]) if k < hi and self.ib[k] == c else 0

    def without(self, a_values=(), b_values=()):
        """-> LabelPairs without the rows of a_values and the columns of b_values (values that do not occur change nothing); the
        ranks are renumbered."""
        keep_a = ~np.isin(self.a_ids, np.asarray(a_values, np.int64).reshape(-1))
        keep_b = ~np.isin(self.b_ids, np.asarray(b_values, np.int64).reshape(-1))
        new_a, new_b = np.cumsum(keep_a) - 1, np.cumsum(keep_b) - 1
        keep = keep_a[self.ia] & keep_b[self.ib]
        return LabelPairs(self.a_ids[keep_a], self.b_ids[keep_b], new_a[self.ia[keep]], new_b[self.ib[keep]], self.count[keep])


def _sums(idx, count, n):
    out = np.zeros(n, np.int64)
    np.add.at(out, idx, count)
    return out


def _find(ids, value):
    k = int(np.searchsorted(ids, value))
    return k if k < ids.size and int(ids[k]) == int(value) else -1


def _check_pair(who, a, b):
    a, b = _check_map(who, a, "a"), _check_map(who, b, "b")
    if a.shape != b.shape:
        raise ValueError("%s: b %s does not have the shape of a %s" % (who, b.shape, a.shape))
    return a, b


def _check_sizes(who, na, nb):
    if na > MAX_IDS or nb > MAX_IDS:
        raise ValueError("%s: the maps have %d and %d distinct values (limit %d)" % (who, na, nb, MAX_IDS))
    if na * nb > MAX_CELLS:
        raise ValueError("%s: %d x %d distinct values are %d cells (limit %d)" % (who, na, nb, na * nb, MAX_CELLS))


def label_pairs_numpy(a, b):
    """The pair table of two label maps as plain numpy on the host -- the specification csrc/label_pairs.hip is tested against.
    -> LabelPairs.  Raises ValueError where label_pairs does."""
    who = "label_pairs_numpy"
    a, b = _check_pair(who, a, b)
    _check_range(who, a)
    _check_range(who, b)
    key, count = np.unique((a.astype(np.int64).reshape(-1) << 24) | b.astype(np.int64).reshape(-1), return_counts=True)
    ka, kb = key >> 24, key & (MAX_ID - 1)
    a_ids, b_ids = np.unique(ka), np.unique(kb)
    _check_sizes(who, a_ids.size, b_ids.size)
    return LabelPairs(a_ids, b_ids, np.searchsorted(a_ids, ka), np.searchsorted(b_ids, kb), count)


def label_pairs(a, b, device_id=None):
    """label_pairs_numpy on the GPU (mnc_label_pairs, one call that uploads each map once): the same LabelPairs field by field.
    Other integer dtypes are accepted as from_labels accepts them; what the rule refuses raises ValueError."""
    who = "label_pairs"
    a, b = _check_pair(who, a, b)
    for m in (a, b):
        if m.dtype != np.int32:
            _check_range(who, m)                              # (before the cast, which would wrap a value past int32)
    a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    H, W = a.shape
    cap = min(MAX_CELLS, H * W)
    cap_ids = min(MAX_IDS, H * W)
    a_ids, b_ids = np.empty(cap_ids, np.int32), np.empty(cap_ids, np.int32)
    ia, ib, count = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int64)
    na, nb, m = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_longlong(-1)
    try:
        _lib.call("mnc_label_pairs", _lib.ptr(a), _lib.ptr(b), int(H), int(W), cap_ids, cap, ctypes.addressof(na), _lib.ptr(a_ids),
                  ctypes.addressof(nb), _lib.ptr(b_ids), ctypes.addressof(m), _lib.ptr(ia), _lib.ptr(ib), _lib.ptr(count),
                  _device_id(device_id))
    except _lib.MncError as e:
        if e.code == 1 and "not in [0," in str(e):
            raise ValueError(str(e))
        if e.code == 1 and na.value >= 0:
            _check_sizes(who, na.value, nb.value)
        raise
    return LabelPairs(a_ids[:na.value].copy(), b_ids[:nb.value].copy(), ia[:m.value].copy(), ib[:m.value].copy(),
                      count[:m.value].copy())


def plan(global_only):
    """mnc_label_pairs_plan: True counts every table in device memory from now on, False (the default) the small ones in LDS."""
    _lib.call("mnc_label_pairs_plan", int(bool(global_only)))


def timing(on):
    """mnc_label_pairs_timing: 0 off, 1 an event pair around the launches of a call, 2 around its counting launch alone -> the
    milliseconds of the last timed call (-1.0: none)."""
    last = ctypes.c_double(-1.0)
    _lib.call("mnc_label_pairs_timing", int(on), ctypes.addressof(last))
    return float(last.value)


# ---- the semantic scores ----

def confusion(gt, pred, num_classes, ignore=255, device=True, device_id=None):
    """The confusion matrix of a semantic result: int64 [C, C], conf[g, p] = the pixels of class g predicted as p.  Pixels whose gt
    equals `ignore` (None: none) are dropped; any other value of gt or pred outside [0, C) raises ValueError naming it.
    device=False never touches the GPU."""
    who = "confusion"
    C = int(num_classes)
    if C < 1:
        raise ValueError("%s: num_classes=%d" % (who, C))
    t = label_pairs(gt, pred, device_id) if device else label_pairs_numpy(gt, pred)
    if ignore is not None:
        t = t.without(a_values=(int(ignore),))
    for name, ids in (("gt", t.a_ids), ("pred", t.b_ids)):
        if ids.size and int(ids[-1]) >= C:
            raise ValueError("%s: %s value %d not in [0, %d)" % (who, name, int(ids[-1]), C))
    out = np.zeros((C, C), np.int64)
    out[t.a_ids[t.ia], t.b_ids[t.ib]] = t.count
    return out


def semantic_scores(conf):
    """FCN's four numbers from a confusion matrix (rows gt, columns pred), float64 on the host:
        pixel_acc = sum_i n_ii / sum_i t_i          mean_acc = mean_i n_ii / t_i
        miou      = mean_i n_ii / (t_i + sum_j n_ji - n_ii)
        fwiou     = sum_i t_i * iou_i / sum_i t_i
    with t_i the row sums.  Classes with an empty row are left out of the means (and add nothing to the sums).  An all-zero matrix
    gives nan."""
    conf = np.asarray(conf)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError("semantic_scores: conf %s is not square" % (conf.shape,))
    conf = conf.astype(np.float64)
    diag, rows, cols = np.diag(conf), conf.sum(axis=1), conf.sum(axis=0)
    has = rows > 0
    if not has.any():
        nan = float("nan")
        return {"pixel_acc": nan, "mean_acc": nan, "miou": nan, "fwiou": nan}
    iou = diag[has] / (rows[has] + cols[has] - diag[has])
    return {"pixel_acc": float(diag.sum() / rows.sum()), "mean_acc": float(np.mean(diag[has] / rows[has])),
            "miou": float(np.mean(iou)), "fwiou": float((rows[has] * iou).sum() / rows.sum())}
