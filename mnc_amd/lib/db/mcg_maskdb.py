"""The MCG proposal maskdb of the CFM task: the validation branch of the reference's tools/prepare_mcg_maskdb.py:55-97.

One image of the published MCG candidates (data/MCG-raw/<name>.mat) holds `superpixels`, a label map [H, W] (1-based uint16),
and `labels`, a cell array of n lists of superpixel ids.  Proposal i is the union P_i of its superpixels (np.in1d: duplicates and
ids that occur nowhere change nothing); the maskdb entry is

    boxes[i] = [min col, min row, max col, max row] of P_i                                        float64
    masks[i] = cv2.resize(P_i[y1:y2+1, x1:x2+1], (S, S), interpolation=cv2.INTER_NEAREST)         0 / 1

The nearest rule is OpenCV's resizeNN (modules/imgproc/src/resize.cpp): destination index d reads source index
min(floor(d * ifx), w - 1) with ifx = 1.0 / (float(S) / w) in float64 -- the inverse scale formed in TWO steps, then cvFloor.  It
differs from the exact integer d * w // S (w = 87, d = 7: 28, not 29) and from the one-step d * (w / float(S)).  cv2 is not a
dependency of this project, so the rule rests on OpenCV's published source, as the bilinear restatement in oracle/host.py does.

    read_mcg_raw(path)                   -> (superpixels int32 [H, W] C-contiguous, label_ptr int32 [n + 1], label_ids int32)
    mcg_maskdb_numpy(sp, ptr, ids, ...)  the reference's loop in numpy: no cv2, no GPU
    mcg_maskdb_device(sp, ptr, ids, ...) the same through mnc_mcg_maskdb (csrc/mcg_maskdb.hip); raises without the library or a GPU
    write_maskdb(path, db)               the .mat file the reference writes ({'masks': bool, 'boxes': float64})

Both forms return what scipy.io.loadmat gives back for the reference's file: boxes float64 [n, 4], masks uint8 [n, S, S]."""
import numpy as np


def nearest_src_index(dst_size, src_size):
    """cv2.resize INTER_NEAREST along one axis: the source index of every destination index, int64 [dst_size]."""
    inv = 1.0 / (float(dst_size) / src_size)
    return np.minimum(np.floor(np.arange(dst_size) * inv).astype(np.int64), src_size - 1)


def read_mcg_raw(path):
    """One MCG-raw file -> (superpixels, label_ptr, label_ids): the label map as C-contiguous int32 (loadmat returns it
    Fortran-ordered), the cell array `labels` (labels[i][0][0] is proposal i's list) flattened to CSR int32."""
    import scipy.io
    mat = scipy.io.loadmat(path)
    superpixels = np.ascontiguousarray(mat['superpixels'], dtype=np.int32)
    labels = mat['labels']
    lists = [np.asarray(labels[i][0]).reshape(-1) for i in range(len(labels))]
    label_ptr = np.zeros(len(lists) + 1, np.int32)
    if lists:
        label_ptr[1:] = np.cumsum([len(x) for x in lists])
    label_ids = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return superpixels, label_ptr, np.ascontiguousarray(label_ids)


def _num_kept(n, top_k):
    return n if top_k == -1 else len(range(n)[:top_k])           # mcg_boxes[:top_k, :]


def mcg_maskdb_numpy(superpixels, label_ptr, label_ids, mask_size=21, top_k=-1):
    """tools/prepare_mcg_maskdb.py:67-94 for one image, with cv2.resize(..., INTER_NEAREST) written out.  Only the first top_k
    proposals are computed (top_k = -1: all).  A proposal that covers no pixel raises ValueError (the reference dies in np.min)."""
    superpixels = np.asarray(superpixels)
    S = int(mask_size)
    n = _num_kept(len(label_ptr) - 1, int(top_k))
    boxes = np.zeros((n, 4))
    masks = np.zeros((n, S, S), dtype=np.uint8)
    for i in range(n):
        label = label_ids[label_ptr[i]:label_ptr[i + 1]]
        proposal = np.isin(superpixels, label)
        r, c = np.where(proposal)
        if r.size == 0:
            raise ValueError('mcg_maskdb_numpy: proposal %d covers no pixel' % i)
        y1, x1, y2, x2 = np.min(r), np.min(c), np.max(r), np.max(c)
        sy = y1 + nearest_src_index(S, y2 - y1 + 1)
        sx = x1 + nearest_src_index(S, x2 - x1 + 1)
        masks[i] = proposal[sy[:, None], sx[None, :]]
        boxes[i] = [x1, y1, x2, y2]
    return {'boxes': boxes, 'masks': masks}


def mcg_maskdb_device(superpixels, label_ptr, label_ids, mask_size=21, top_k=-1, device_id=None):
    """mcg_maskdb_numpy through mnc_mcg_maskdb: one device call per image.  A proposal that covers no pixel, ids outside
    [0, 65535] and a mask_size outside [1, 32] raise mnc_amd._lib.MncError.  There is no fallback."""
    from mnc_amd import _lib
    if device_id is None:
        from mnc_config import cfg
        device_id = int(cfg.get('GPU_ID', 0))
    superpixels = np.ascontiguousarray(superpixels, dtype=np.int32)
    if superpixels.ndim != 2:
        raise ValueError('mcg_maskdb_device: superpixels must be [H, W] (got %r)' % (superpixels.shape,))
    S = int(mask_size)
    n = _num_kept(len(label_ptr) - 1, int(top_k))
    label_ptr = np.ascontiguousarray(np.asarray(label_ptr)[:n + 1], dtype=np.int32)
    label_ids = np.ascontiguousarray(label_ids, dtype=np.int32)
    if n and int(label_ptr.max()) > label_ids.size:
        raise ValueError('mcg_maskdb_device: label_ptr reaches %d, label_ids has %d' % (int(label_ptr.max()), label_ids.size))
    boxes = np.zeros((n, 4), np.float64)
    masks = np.zeros((n, max(S, 0), max(S, 0)), np.uint8)
    H, W = superpixels.shape
    _lib.call('mnc_mcg_maskdb', _lib.ptr(superpixels), int(H), int(W), _lib.ptr(label_ptr), _lib.ptr(label_ids), n, S,
              _lib.ptr(boxes), _lib.ptr(masks), int(device_id))
    return {'boxes': boxes, 'masks': masks}


def write_maskdb(path, db):
    """The validation maskdb file of one image, as tools/prepare_mcg_maskdb.py:91-95 writes it."""
    import scipy.io
    scipy.io.savemat(path, {'masks': np.asarray(db['masks']).astype(bool), 'boxes': np.asarray(db['boxes'], np.float64)})
