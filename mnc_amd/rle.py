"""COCO run-length encoding of packed instance masks, and the way back (include/mnc_hip.h n7, csrc/mask_rle.hip): the rule of the
published maskApi.c.  An H x W mask is read column by column (pixel (x, y) stands at position x * H + y); its counts are the
lengths of the runs of 0 and of 1 in turn, beginning with a run of 0; the compressed string packs them five bits a character,
from the fourth count on as the difference to the count two places before.

    rle_counts_numpy(pm, H, W)              the CPU statement: PackedMasks.full(i, H, W) flattened in Fortran order, np.flatnonzero
                                            of its diff -> (run_ptr int64 [n + 1], runs uint32)
    masks_from_counts_numpy(run_ptr, runs, H, W)   the reverse through np.repeat -> PackedMasks with tight bounds
    rle_counts(pm, H, W)                    the same counts through mnc_mask_rle (the GPU)
    masks_from_counts(run_ptr, runs, H, W)  the same PackedMasks through mnc_mask_from_rle (the GPU)
    counts_to_string / string_to_counts     rleToString / rleFrString, numpy-vectorised
    mask_rle(pm, H, W)                      -> [{"size": [H, W], "counts": str}] of a PackedMasks (its .rle(H, W))
    masks_from_rle(rles)                    COCO RLEs of one image size -> PackedMasks (PackedMasks.from_rle)

There is no fallback: without the library or a GPU the device functions raise."""
import ctypes

import numpy as np

from . import _lib
from .masks import MAX_SIDE, PackedMasks, _device_id, _set_args, sized_then_filled

MAX_MASKS = 2048
FIRST_RUNS = 1 << 16            # room of the first mnc_mask_rle_dev of a device-resident result; one retry at the true total
RLE_HEAD = np.dtype({"names": ["kept", "total_runs"], "formats": ["<i4", "<i8"], "offsets": [0, 8], "itemsize": 256})


def _check_image(who, H, W):
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("%s: image %d x %d not in [1, %d]" % (who, H, W, MAX_SIDE))


def rle_counts_numpy(pm, H, W):
    """The rule as plain numpy on the host: per instance pm.full(i, H, W) flattened column by column, the positions where it
    changes, their differences.  -> (run_ptr int64 [n + 1], runs uint32 [run_ptr[n]])."""
    H, W = int(H), int(W)
    _check_image("rle_counts_numpy", H, W)
    run_ptr, runs = np.zeros(len(pm) + 1, np.int64), []
    for i in range(len(pm)):
        flat = pm.full(i, H, W).reshape(-1, order="F").astype(np.int8)
        t = np.flatnonzero(np.diff(flat, prepend=np.int8(0)))
        runs.append(np.diff(np.concatenate(([0], t, [H * W]))).astype(np.uint32))
        run_ptr[i + 1] = run_ptr[i] + len(runs[-1])
    return run_ptr, (np.concatenate(runs) if runs else np.zeros(0, np.uint32))


def _check_counts(who, run_ptr, runs, H, W):
    run_ptr = np.ascontiguousarray(run_ptr, np.int64).reshape(-1)
    runs = np.ascontiguousarray(runs, np.uint32).reshape(-1)
    _check_image(who, H, W)
    n = len(run_ptr) - 1
    if n < 0 or n > MAX_MASKS:
        raise ValueError("%s: %d masks not in [0, %d]" % (who, n, MAX_MASKS))
    if run_ptr[0] < 0 or (np.diff(run_ptr) < 0).any() or run_ptr[-1] > len(runs):
        raise ValueError("%s: run_ptr is negative, decreasing or reaches past the runs" % who)
    return run_ptr, runs, n


def masks_from_counts_numpy(run_ptr, runs, H, W, classes=None, scores=None):
    """The reverse as plain numpy on the host: per mask np.repeat of (0, 1, 0, ...) by its counts, reshaped column-major; the
    bounds are the tight box of the set pixels, an empty mask gets (0, 0, -1, -1) and no rows.  Runs of length 0 are accepted.
    Raises ValueError where mnc_mask_from_rle returns MNC_ERR_INVALID."""
    H, W = int(H), int(W)
    run_ptr, runs, n = _check_counts("masks_from_counts_numpy", run_ptr, runs, H, W)
    bounds, dense = np.zeros((n, 4), np.int32), [None] * n
    for i in range(n):
        c = runs[run_ptr[i]:run_ptr[i + 1]].astype(np.int64)
        if c.sum() != H * W:
            raise ValueError("masks_from_counts_numpy: the counts of mask %d sum to %d, not %d x %d" % (i, c.sum(), H, W))
        m = np.repeat(np.arange(len(c)) & 1, c).astype(bool).reshape(W, H).T
        if not m.any():
            bounds[i] = (0, 0, -1, -1)
            continue
        xs, ys = np.flatnonzero(m.any(axis=0)), np.flatnonzero(m.any(axis=1))
        x1, y1, x2, y2 = int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])
        bounds[i] = (x1, y1, x2, y2)
        dense[i] = m[y1:y2 + 1, x1:x2 + 1]
    return PackedMasks.from_dense(bounds, dense, classes, scores)


def _chars(counts):
    """counts of ONE mask -> (uint8 [n, 7] characters, bool [n, 7] which of them are emitted): rleToString's loop for every entry
    at once (a count or a difference of two is below 2^31 in size: at most seven groups of five bits)."""
    x = np.asarray(counts, np.int64).copy()
    x[3:] -= np.asarray(counts, np.int64)[1:-2]
    k = np.arange(7, dtype=np.int64)
    c = (x[:, None] >> (5 * k)) & 0x1f
    rest = x[:, None] >> (5 * (k + 1))                                       # arithmetic shift
    more = np.where(c & 0x10, rest != -1, rest != 0)
    emitted = np.ones(more.shape, bool)
    emitted[:, 1:] = np.logical_and.accumulate(more[:, :-1], axis=1)
    return (c | np.where(more, 0x20, 0)).astype(np.uint8) + 48, emitted


def counts_to_string(counts):
    """rleToString: the counts of one mask -> str."""
    counts = np.asarray(counts).reshape(-1)
    if counts.size == 0:
        return ""
    chars, emitted = _chars(counts)
    return chars[emitted].tobytes().decode("ascii")


def string_to_counts(s):
    """rleFrString: str or bytes -> the counts of one mask, uint32."""
    raw = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), np.uint8)
    if raw.size == 0:
        return np.zeros(0, np.uint32)
    c = raw.astype(np.int64) - 48
    if ((c < 0) | (c > 0x3f)).any():
        raise ValueError("string_to_counts: a character outside chr(48) .. chr(111)")
    last = (c & 0x20) == 0                                                   # the last character of an entry
    if not last[-1]:
        raise ValueError("string_to_counts: the string ends inside an entry")
    first = np.flatnonzero(np.concatenate(([True], last[:-1])))
    k = np.arange(len(c)) - np.repeat(first, np.diff(np.concatenate((first, [len(c)]))))
    if k.max() > 6:
        raise ValueError("string_to_counts: an entry of more than seven characters")
    x = np.add.reduceat((c & 0x1f) << (5 * k), first)                        # (the groups do not overlap: + is |)
    ends = np.flatnonzero(last)
    x = np.where(c[ends] & 0x10, x | (np.int64(-1) << (5 * (k[ends] + 1))), x)
    # from the fourth entry on x is the difference to the entry two places before: two interleaved running sums
    out = x.copy()
    out[1::2] = np.cumsum(x[1::2])
    out[2::2] = np.cumsum(x[2::2])
    if ((out < 0) | (out > 0xffffffff)).any():
        raise ValueError("string_to_counts: a count outside uint32")
    return out.astype(np.uint32)


def rle_counts_call(pm, H, W, runs=None, device_id=0):
    """mnc_mask_rle as it is: runs None asks for run_ptr and the total only.  -> (run_ptr, total)."""
    run_ptr, total = np.zeros(len(pm) + 1, np.int64), ctypes.c_size_t(0)
    _lib.call("mnc_mask_rle", *(_set_args(pm, areas=False) + (int(H), int(W), _lib.ptr(run_ptr), _lib.ptr(runs),
                                                             runs.size if runs is not None else 0, ctypes.addressof(total), int(device_id))))
    return run_ptr, int(total.value)


def rle_counts(pm, H, W, device_id=None):
    """rle_counts_numpy on the GPU (mnc_mask_rle, csrc/mask_rle.hip): the same (run_ptr, runs) bit for bit.  Invalid sets and
    sizes raise _lib.MncError (MNC_ERR_INVALID) before anything is launched."""
    device_id = _device_id(device_id)
    _, total = rle_counts_call(pm, H, W, None, device_id)
    runs = np.zeros(max(total, 1), np.uint32)
    run_ptr, total = rle_counts_call(pm, H, W, runs, device_id)
    return run_ptr, runs[:total]


def _device_rle_call(dev, H, W, runs_cap):
    """One mnc_mask_rle_dev and the copy of head + run_ptr -> (device address of the result, the copied bytes, kept, total_runs)."""
    d_rle = ctypes.c_void_p()
    front = np.zeros(RLE_HEAD.itemsize + 8 * (dev.rows + 1), np.uint8)
    _lib.call("mnc_mask_rle_dev", dev._ctx.h, dev.d_info, dev.d_bits, dev.rows, int(H), int(W), int(runs_cap), ctypes.addressof(d_rle))
    _lib.call("mnc_d2h", dev._ctx.h, _lib.ptr(front), d_rle.value, front.nbytes)
    head = front[:RLE_HEAD.itemsize].view(RLE_HEAD)[0]
    return d_rle.value, front, int(head["kept"]), int(head["total_runs"])


def device_rle_counts(dev, H, W, runs_cap=FIRST_RUNS):
    """mnc_mask_rle_dev of a device-resident result (mnc_amd.masks._DeviceResult): a first try with room for runs_cap runs, one
    more at the true total when that was too little; head + run_ptr in one copy, the runs in a second.  -> (run_ptr, runs)."""
    dev.check()
    d_rle, front, kept, total = _device_rle_call(dev, H, W, runs_cap)
    if total > runs_cap:
        d_rle, front, kept, total = _device_rle_call(dev, H, W, total)
    runs = np.zeros(total, np.uint32)
    if total:
        _lib.call("mnc_d2h", dev._ctx.h, _lib.ptr(runs), d_rle + front.nbytes, runs.nbytes)
    return front[RLE_HEAD.itemsize:].view(np.int64)[:kept + 1].copy(), runs


def masks_from_counts_call(run_ptr, runs, H, W, bits=None, device_id=0):
    """mnc_mask_from_rle as it is: bits None asks for bounds, offsets, areas and the size only.  -> (bounds, offsets, areas,
    bytes needed)."""
    n = len(run_ptr) - 1
    bounds, offsets, areas = np.zeros((n, 4), np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    need = ctypes.c_size_t(0)
    _lib.call("mnc_mask_from_rle", _lib.ptr(run_ptr), _lib.ptr(runs), n, int(H), int(W), _lib.ptr(bounds), _lib.ptr(offsets),
              _lib.ptr(areas), _lib.ptr(bits), bits.nbytes if bits is not None else 0, ctypes.addressof(need), int(device_id))
    return bounds, offsets, areas, int(need.value)


def masks_from_counts(run_ptr, runs, H, W, classes=None, scores=None, device_id=None):
    """masks_from_counts_numpy on the GPU (mnc_mask_from_rle): the same PackedMasks field by field."""
    device_id = _device_id(device_id)
    run_ptr = np.ascontiguousarray(run_ptr, np.int64).reshape(-1)
    runs = np.ascontiguousarray(runs, np.uint32).reshape(-1)
    if len(run_ptr) < 1 or (len(run_ptr) > 1 and run_ptr.max() > len(runs)):
        raise ValueError("masks_from_counts: run_ptr is empty or reaches past the runs")
    bounds, offsets, areas, bits = sized_then_filled(lambda bits: masks_from_counts_call(run_ptr, runs, H, W, bits, device_id))
    return PackedMasks(bounds, offsets, areas, classes, scores, bits)


def _to_rles(run_ptr, runs, H, W):
    return [{"size": [int(H), int(W)], "counts": counts_to_string(runs[run_ptr[i]:run_ptr[i + 1]])} for i in range(len(run_ptr) - 1)]


def mask_rle_numpy(pm, H, W):
    """-> [{"size": [H, W], "counts": str}] per instance through rle_counts_numpy: the CPU form of PackedMasks.rle."""
    return _to_rles(*(rle_counts_numpy(pm, H, W) + (H, W)))


def mask_rle(pm, H, W, device_id=None):
    """-> [{"size": [H, W], "counts": str}] per instance of a PackedMasks, the counts made on the GPU (pm.rle(H, W)); device_id
    names the GPU for host arrays (a device-resident result is encoded where it lies)."""
    return pm.rle(H, W, device_id)


def counts_of_rles(rles):
    """COCO RLEs of one image size -- {"size": [H, W], "counts": str, bytes or an uncompressed list} each -> (run_ptr, runs, H,
    W).  Raises ValueError on mixed sizes (an empty list has no size: H = W = 1)."""
    rles = list(rles)
    sizes = {(int(r["size"][0]), int(r["size"][1])) for r in rles}
    if len(sizes) > 1:
        raise ValueError("masks_from_rle: the masks are of different sizes: %s" % sorted(sizes))
    H, W = sizes.pop() if sizes else (1, 1)
    counts = [string_to_counts(r["counts"]) if isinstance(r["counts"], (str, bytes)) else _list_counts(r["counts"]) for r in rles]
    run_ptr = np.zeros(len(rles) + 1, np.int64)
    run_ptr[1:] = np.cumsum([len(c) for c in counts])
    return run_ptr, (np.concatenate(counts) if counts else np.zeros(0, np.uint32)), H, W


def _list_counts(counts):
    c = np.asarray(counts, np.int64).reshape(-1)
    if ((c < 0) | (c > 0xffffffff)).any():
        raise ValueError("masks_from_rle: a count outside uint32")
    return c.astype(np.uint32)


def masks_from_rle(rles, classes=None, scores=None, device_id=None):
    """COCO RLEs (all of one image size) -> PackedMasks with tight bounds on the GPU (mnc_mask_from_rle), so that overlaps() and
    nms() work on crowd ground truth, somebody else's results or a file of our own read back."""
    run_ptr, runs, H, W = counts_of_rles(rles)
    return masks_from_counts(run_ptr, runs, H, W, classes, scores, device_id)


def masks_from_rle_numpy(rles, classes=None, scores=None):
    """masks_from_rle through masks_from_counts_numpy: the CPU statement."""
    run_ptr, runs, H, W = counts_of_rles(rles)
    return masks_from_counts_numpy(run_ptr, runs, H, W, classes, scores)
