"""COCO's `segm` evaluation of packed instance masks (include/mnc_hip.h n8, csrc/mask_match.hip): the rule of the published
cocoeval.py (computeIoU, evaluateImg, accumulate, summarize) and of rleIou in maskApi.c, on mnc_amd.masks.PackedMasks.

    match_numpy(dt, gt, iscrowd, ...)   the CPU statement of the matching of one image: the plain loop of evaluateImg
    match_closed_numpy(...)             the same tables from the closed form the kernel uses (a detection takes the largest IoU,
                                        of several equal the highest index; not-ignored before ignored)
    match(dt, gt, iscrowd, ...)         the same tables through mnc_mask_match (the GPU); PackedMasks.match is the method, which
                                        matches a device-resident result where it lies (mnc_mask_match_dev)
    match_boundary_numpy(dt, gt, H, W, ...) / match_boundary(...)   the matching on min(mask IoU, boundary IoU) (n11,
                                        mnc_amd/boundary.py): the statement and mnc_mask_match_boundary (the GPU)
    accumulate(images, ...)             per-image tables -> precision [T, R, K, A, M] and recall [T, K, A, M], host numpy
    flatten_records(images, ...)        the image records as the flat arrays of mnc_coco_accumulate (include/mnc_hip.h n10)
    accumulate_flat_numpy(flat, ...)    the same tables from the flat arrays by the closed form csrc/coco_accum.hip uses (one stable
                                        sort by (class, score); per cell the least tp count that reaches each recall threshold)
    accumulate_flat(flat, ...)          mnc_coco_accumulate on those arrays
    accumulate_device(images, ...)      accumulate through it (the GPU): the same tables bit for bit
    summarize(acc)                      -> the twelve numbers, an ordered dict
    CocoSegmEval                        .add(image_id, dt, gt, iscrowd, ...) per image, .accumulate(), .summarize(), .stats;
                                        iou_type="boundary" scores by the boundary protocol (add then needs image_size=(H, W))

Every table of a match is in the caller's index order with -1 for "none": rank int32 [D], dt_match int32 [A, T, D], dt_ignore uint8
[A, T, D], gt_match int32 [A, T, G], gt_ignore uint8 [A, G], iou float64 [D, G] (None unless asked for).  There is no fallback:
without the library or a GPU match() and accumulate_device() raise; device=False / match_numpy / accumulate is the path that needs
neither."""
import collections
import ctypes

import numpy as np

from . import _lib

MAX_N = 2048
MAX_T = 16
MAX_A = 8
# csrc/coco_accum.hip: the keys of one sort workgroup and the elements of one step of a cell's walk (tests size their cases
# from these; tests/test_coco_accum_host.py checks them against the source), and the limits of mnc_coco_accumulate
ACCUM_SORT_TILE = 2048
ACCUM_SCAN_CHUNK = 1024
ACCUM_MAX_N = 1 << 24
ACCUM_MAX_K = 4096
ACCUM_MAX_M = 8
ACCUM_MAX_R = 1024
IOU_THRS = np.linspace(.5, .95, 10)
AREA_RNGS = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)
AREA_LABELS = ("all", "small", "medium", "large")
MAX_DETS = (1, 10, 100)
REC_THRS = np.linspace(0, 1, 101)
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")

Match = collections.namedtuple("Match", "rank dt_match dt_ignore gt_match gt_ignore iou")


def _params(who, D, scores, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det):
    """The arguments as the arrays of the C ABI, checked as mnc_mask_match checks them (ValueError in the place of
    MNC_ERR_INVALID).  D detections with `scores` (None: they lie on the device)."""
    G = len(gt)
    thrs = np.ascontiguousarray(IOU_THRS if iou_thrs is None else iou_thrs, np.float64).reshape(-1)
    rngs = np.ascontiguousarray(AREA_RNGS if area_rngs is None else area_rngs, np.float64).reshape(-1, 2)
    crowd = np.ascontiguousarray(np.zeros(G) if iscrowd is None else iscrowd).reshape(-1)
    ign = np.ascontiguousarray(np.zeros(G) if ignore is None else ignore).reshape(-1)
    area = np.ascontiguousarray(gt.areas if eval_area is None else eval_area, np.float64).reshape(-1)
    max_det = int(max_det)
    if D > MAX_N or G > MAX_N:
        raise ValueError("%s: %d detections / %d ground truths not in [0, %d]" % (who, D, G, MAX_N))
    if not 1 <= len(thrs) <= MAX_T or not 1 <= len(rngs) <= MAX_A or not 1 <= max_det <= MAX_N:
        raise ValueError("%s: T=%d not in [1, %d], A=%d not in [1, %d] or max_det=%d not in [1, %d]"
                         % (who, len(thrs), MAX_T, len(rngs), MAX_A, max_det, MAX_N))
    if len(crowd) != G or len(ign) != G or len(area) != G:
        raise ValueError("%s: iscrowd, ignore and eval_area must have one entry per ground truth" % who)
    if np.isnan(thrs).any() or np.isnan(rngs).any() or (rngs[:, 0] > rngs[:, 1]).any():
        raise ValueError("%s: a NaN threshold or range bound, or lo > hi" % who)
    if scores is not None and np.isnan(np.asarray(scores, np.float32)).any():
        raise ValueError("%s: a NaN score" % who)
    if not np.isin(crowd, (0, 1)).all() or not np.isin(ign, (0, 1)).all():
        raise ValueError("%s: a crowd or ignore value other than 0 / 1" % who)
    return thrs, rngs, crowd.astype(np.uint8), ign.astype(np.uint8), area, max_det


def ranks_numpy(classes, scores):
    """rank[d] = the position of detection d among the detections of its class by score descending, equal scores lower index
    first.  -> int32 [D]."""
    classes, scores = np.asarray(classes, np.int32), np.asarray(scores, np.float32)
    rank = np.zeros(len(classes), np.int32)
    for k in np.unique(classes):
        idx = np.flatnonzero(classes == k)
        rank[idx[np.argsort(-scores[idx], kind="mergesort")]] = np.arange(len(idx), dtype=np.int32)
    return rank


def iou_numpy(dt, gt, crowd):
    """Step 2: inter of mask_overlaps_numpy; union = area_d + area_g - inter, for a crowd ground truth area_d (rleIou).  ->
    float64 [D, G]."""
    from .masks import mask_overlaps_numpy
    inter = mask_overlaps_numpy(dt, gt)[0] if len(dt) and len(gt) else np.zeros((len(dt), len(gt)), np.int64)
    union = np.where(np.asarray(crowd, bool)[None, :], np.broadcast_to(dt.areas[:, None], inter.shape),
                     dt.areas[:, None] + gt.areas[None, :] - inter)
    return np.where(union < 1, 0.0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64))


def _gt_ignore(crowd, ign, area, rngs):
    return np.array([(ign != 0) | (crowd != 0) | (area < lo) | (area > hi) for lo, hi in rngs], np.uint8).reshape(len(rngs), len(area))


def _match_tables(dt, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, return_iou, who, choose, _overlap=None):
    """_overlap: a function of the crowd flags -> the [D, G] table to match on in the place of iou_numpy's (match_boundary_numpy)."""
    thrs, rngs, crowd, ign, area, max_det = _params(who, len(dt), dt.scores, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det)
    D, G, T, A = len(dt), len(gt), len(thrs), len(rngs)
    rank = ranks_numpy(dt.classes, dt.scores)
    iou = iou_numpy(dt, gt, crowd) if _overlap is None else _overlap(crowd)
    gig = _gt_ignore(crowd, ign, area, rngs)
    dt_match, dt_ignore = np.full((A, T, D), -1, np.int32), np.zeros((A, T, D), np.uint8)
    gt_match = np.full((A, T, G), -1, np.int32)
    for k in np.unique(dt.classes):
        dets = np.flatnonzero(dt.classes == k)
        dets = [int(d) for d in dets[np.argsort(rank[dets])] if rank[d] < max_det]
        gts = np.flatnonzero(np.asarray(gt.classes) == k)
        for a in range(A):
            order = [int(g) for g in gts[np.argsort(gig[a][gts], kind="mergesort")]]       # not ignored first, each group by index
            lo, hi = rngs[a]
            for t in range(T):
                for d in dets:
                    m = choose(d, order, iou, gig[a], crowd, gt_match[a, t], min(thrs[t], 1 - 1e-10))
                    if m >= 0:
                        dt_match[a, t, d], gt_match[a, t, m], dt_ignore[a, t, d] = m, d, gig[a, m]
                    elif dt.areas[d] < lo or dt.areas[d] > hi:
                        dt_ignore[a, t, d] = 1
    return Match(rank, dt_match, dt_ignore, gt_match, gig, iou if return_iou else None)


def _choose_loop(d, order, iou, gig, crowd, gtm, thr):
    """evaluateImg's walk for one detection."""
    best, m = thr, -1
    for g in order:
        if gtm[g] >= 0 and not crowd[g]:
            continue
        if m >= 0 and not gig[m] and gig[g]:
            break
        if iou[d, g] < best:
            continue
        best, m = iou[d, g], g
    return m


def _choose_closed(d, order, iou, gig, crowd, gtm, thr):
    """The closed form: the largest IoU >= thr among the not-ignored, unmatched; else among the ignored that are crowd or
    unmatched; of several equal the highest index."""
    for want in (0, 1):
        cand = [g for g in order if gig[g] == want and (gtm[g] < 0 or (want and crowd[g])) and iou[d, g] >= thr]
        if cand:
            top = max(iou[d, g] for g in cand)
            return max(g for g in cand if iou[d, g] == top)
    return -1


def match_numpy(dt, gt, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, return_iou=False):
    """The matching of one image as the plain loop on the host -- the specification csrc/mask_match.hip is tested against.  dt: a
    PackedMasks with classes and scores; gt: one with classes; iscrowd, ignore (default 0) and eval_area (default gt.areas) per
    ground truth; iou_thrs [T], area_rngs [A][2], max_det.  -> Match.  Raises ValueError where mnc_mask_match returns
    MNC_ERR_INVALID for a parameter."""
    return _match_tables(dt, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, return_iou, "match_numpy", _choose_loop)


def match_closed_numpy(dt, gt, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, return_iou=False):
    """match_numpy with the closed form in the place of the walk (what the kernel computes, stated on the host)."""
    return _match_tables(dt, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, return_iou, "match_closed_numpy",
                         _choose_closed)


def _gt_args(gt, crowd, ign, area, thrs, rngs, max_det):
    from .masks import _set_args
    return _set_args(gt) + (_lib.ptr(gt.classes), _lib.ptr(crowd), _lib.ptr(ign), _lib.ptr(area), _lib.ptr(thrs), len(thrs),
                            _lib.ptr(rngs), len(rngs), max_det)


def _tables(D, G, T, A, return_iou):
    """The output tables of one matching, zeroed: rank, dt_match, dt_ignore, gt_match, gt_ignore, iou (None: not wanted)."""
    return (np.zeros(D, np.int32), np.zeros((A, T, D), np.int32), np.zeros((A, T, D), np.uint8), np.zeros((A, T, G), np.int32),
            np.zeros((A, G), np.uint8), np.zeros((D, G), np.float64) if return_iou else None)


def match(dt, gt, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, return_iou=False,
          device_id=None):
    """match_numpy on the GPU (mnc_mask_match, csrc/mask_match.hip): the same tables bit for bit.  Invalid sets and parameters
    raise ValueError or _lib.MncError (MNC_ERR_INVALID) before anything is launched."""
    from .masks import _device_id, _set_args
    thrs, rngs, crowd, ign, area, max_det = _params("match", len(dt), dt.scores, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det)
    tables = _tables(len(dt), len(gt), len(thrs), len(rngs), return_iou)
    _lib.call("mnc_mask_match", *(_set_args(dt) + (_lib.ptr(dt.classes), _lib.ptr(dt.scores)) +
                                  _gt_args(gt, crowd, ign, area, thrs, rngs, max_det) +
                                  tuple(_lib.ptr(t) for t in tables) + (_device_id(device_id),)))
    return Match(*tables)


def device_match(dev, kept, gt, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100,
                 return_iou=False):
    """mnc_mask_match_dev of a device-resident result (mnc_amd.masks._DeviceResult) of `kept` instances against the host set gt:
    the detections are read where they lie, only the tables come back (five copies, six with the IoU).  -> Match."""
    dev.check()
    thrs, rngs, crowd, ign, area, max_det = _params("device_match", dev.rows, None, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs,
                                                    max_det)
    R, G, T, A = dev.rows, len(gt), len(thrs), len(rngs)
    out = [ctypes.c_void_p() for _ in range(6)]
    _lib.call("mnc_mask_match_dev", dev._ctx.h, dev.d_info, dev.d_bits, R, *(_gt_args(gt, crowd, ign, area, thrs, rngs, max_det) + (
        int(bool(return_iou)),) + tuple(ctypes.addressof(o) for o in out)))
    rank, dt_match, dt_ignore, gt_match, gt_ignore, iou = _tables(R, G, T, A, return_iou)
    tables = [t for t in zip((rank, dt_match, dt_ignore, gt_match, gt_ignore, iou), out) if t[0] is not None and t[0].size]
    for i, (host, d_ptr) in enumerate(tables):
        _lib.call("mnc_d2h" if i == len(tables) - 1 else "mnc_d2h_async", dev._ctx.h, _lib.ptr(host), d_ptr.value, host.nbytes)
    return Match(rank[:kept].copy(), np.ascontiguousarray(dt_match[:, :, :kept]), np.ascontiguousarray(dt_ignore[:, :, :kept]),
                 gt_match, gt_ignore, None if iou is None else np.ascontiguousarray(iou[:kept]))


def match_boundary_numpy(dt, gt, H, W, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100,
                         d=None, ratio=0.02, return_iou=False):
    """match_numpy on the overlap min(mask IoU, boundary IoU) (include/mnc_hip.h n11) -- the specification mnc_mask_match_boundary
    is tested against.  The boundary IoU is iou_numpy of the two sets' boundary bands (mnc_amd.boundary.boundary_numpy in the H x W
    image at distance d; None: boundary_distance(H, W, ratio)): for a crowd ground truth the union is the area of the detection's
    band.  Everything else is match_numpy's: the area-range rules look at the masks' areas and eval_area, not at the bands'.
    -> Match, whose iou (with return_iou) is the minimum that was matched on; with return_iou (Match, biou)."""
    from .boundary import _distance, boundary_numpy
    H, W, d = _distance("match_boundary_numpy", H, W, d, ratio)
    kept = {}

    def overlap(crowd):
        kept["biou"] = iou_numpy(boundary_numpy(dt, H, W, d), boundary_numpy(gt, H, W, d), crowd)
        return np.minimum(iou_numpy(dt, gt, crowd), kept["biou"])

    m = _match_tables(dt, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, return_iou, "match_boundary_numpy", _choose_loop,
                      overlap)
    return (m, kept["biou"]) if return_iou else m


def match_boundary(dt, gt, H, W, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, d=None,
                   ratio=0.02, return_iou=False, device_id=None):
    """match_boundary_numpy on the GPU (mnc_mask_match_boundary: csrc/mask_boundary.hip makes both boundary sets on the device,
    csrc/mask_match.hip matches on the minimum): the same tables bit for bit.  Invalid sets and parameters raise ValueError or
    _lib.MncError (MNC_ERR_INVALID) before anything is launched."""
    from .boundary import _distance
    from .masks import _device_id, _set_args
    H, W, d = _distance("match_boundary", H, W, d, ratio)
    thrs, rngs, crowd, ign, area, max_det = _params("match_boundary", len(dt), dt.scores, gt, iscrowd, ignore, eval_area, iou_thrs,
                                                    area_rngs, max_det)
    tables = _tables(len(dt), len(gt), len(thrs), len(rngs), return_iou)
    biou = np.zeros((len(dt), len(gt)), np.float64) if return_iou else None
    _lib.call("mnc_mask_match_boundary", *(_set_args(dt) + (_lib.ptr(dt.classes), _lib.ptr(dt.scores)) +
                                           _gt_args(gt, crowd, ign, area, thrs, rngs, max_det) + (H, W, d) +
                                           tuple(_lib.ptr(t) for t in tables) + (_lib.ptr(biou), _device_id(device_id))))
    m = Match(*tables)
    return (m, biou) if return_iou else m


def image_record(dt, gt, m):
    """What accumulate keeps of one image: classes, scores and the tables of its Match."""
    return {"dt_classes": np.asarray(dt.classes, np.int32).copy(), "dt_scores": np.asarray(dt.scores, np.float32).copy(),
            "gt_classes": np.asarray(gt.classes, np.int32).copy(), "rank": m.rank, "dt_match": m.dt_match, "dt_ignore": m.dt_ignore,
            "gt_ignore": m.gt_ignore}


def accumulate(images, iou_thrs=None, area_rngs=None, max_dets=MAX_DETS, classes=None, rec_thrs=None):
    """The published accumulate on host numpy.  images: image_record()s in image order, matched with max_det >= max(max_dets).
    classes: the category ids K (None: every class that occurs, sorted).  -> {"precision": float64 [T, R, K, A, M], "recall":
    float64 [T, K, A, M], "classes", "iou_thrs", "area_rngs", "max_dets", "rec_thrs"}; a cell without a not-ignored ground truth
    stays -1."""
    thrs = np.asarray(IOU_THRS if iou_thrs is None else iou_thrs, np.float64).reshape(-1)
    rngs = np.asarray(AREA_RNGS if area_rngs is None else area_rngs, np.float64).reshape(-1, 2)
    rec_thrs = np.asarray(REC_THRS if rec_thrs is None else rec_thrs, np.float64).reshape(-1)
    max_dets = [int(m) for m in max_dets]
    images = list(images)
    if classes is None:
        seen = [im[key] for im in images for key in ("dt_classes", "gt_classes")]
        classes = np.unique(np.concatenate(seen)) if seen else np.zeros(0, np.int32)
    classes = [int(k) for k in classes]
    T, R, K, A, M = len(thrs), len(rec_thrs), len(classes), len(rngs), len(max_dets)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for ki, k in enumerate(classes):
        for a in range(A):
            for mi, max_det in enumerate(max_dets):
                scores, dtm, dtig, npig = [], [], [], 0
                for im in images:
                    sel = np.flatnonzero((im["dt_classes"] == k) & (im["rank"] < max_det))
                    sel = sel[np.argsort(im["rank"][sel])]
                    scores.append(im["dt_scores"][sel].astype(np.float64))
                    dtm.append(im["dt_match"][a][:, sel])
                    dtig.append(im["dt_ignore"][a][:, sel])
                    npig += int(np.count_nonzero(im["gt_ignore"][a][im["gt_classes"] == k] == 0))
                if npig == 0:
                    continue
                scores = np.concatenate(scores) if scores else np.zeros(0)
                inds = np.argsort(-scores, kind="mergesort")
                matched = (np.concatenate(dtm, axis=1) if dtm else np.zeros((T, 0), np.int32))[:, inds] >= 0
                ignored = (np.concatenate(dtig, axis=1) if dtig else np.zeros((T, 0), np.uint8))[:, inds] != 0
                tp_sum = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, ki, a, mi] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]                       # monotone from the right
                    at = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(R)
                    q[at < nd] = pr[at[at < nd]]
                    precision[t, :, ki, a, mi] = q
    return {"precision": precision, "recall": recall, "classes": classes, "iou_thrs": thrs, "area_rngs": rngs, "max_dets": max_dets,
            "rec_thrs": rec_thrs}


def _accum_params(iou_thrs, area_rngs, max_dets, rec_thrs):
    thrs = np.asarray(IOU_THRS if iou_thrs is None else iou_thrs, np.float64).reshape(-1)
    rngs = np.asarray(AREA_RNGS if area_rngs is None else area_rngs, np.float64).reshape(-1, 2)
    rec_thrs = np.ascontiguousarray(REC_THRS if rec_thrs is None else rec_thrs, np.float64).reshape(-1)
    return thrs, rngs, [int(m) for m in max_dets], rec_thrs


def _class_list(images, classes):
    if classes is None:
        seen = [im[key] for im in images for key in ("dt_classes", "gt_classes")]
        classes = np.unique(np.concatenate(seen)) if seen else np.zeros(0, np.int32)
    return [int(k) for k in classes]


def _class_index(values, uniq):
    """The index of each value in the sorted, distinct `uniq`, -1 where it is not there.  -> int32."""
    values = np.asarray(values, np.int64).reshape(-1)
    if not len(uniq):
        return np.full(len(values), -1, np.int32)
    pos = np.minimum(np.searchsorted(uniq, values), len(uniq) - 1)
    return np.where(uniq[pos] == values, pos, -1).astype(np.int32)


def flatten_records(images, classes, max_dets, T=None, A=None):
    """The image_record()s, in the order given, as the flat arrays of mnc_coco_accumulate: within an image the caller's index
    order; a detection whose rank reaches the largest of max_dets is in no list and is left out.  classes: the sorted, distinct
    category ids that are evaluated.  T, A: the planes of an empty list of images (else taken from the records).  -> {"dt_class_idx"
    int32 [N], "dt_score" float32 [N], "dt_rank" int32 [N], "dt_flags" uint8 [A, T, N] (bit 0: matched, bit 1: ignored),
    "gt_class_idx" int32 [Gn], "gt_ignore" uint8 [A, Gn]}.  No loop over classes."""
    images = list(images)
    uniq = np.asarray(classes, np.int64).reshape(-1)
    if len(uniq) > 1 and not (np.diff(uniq) > 0).all():
        raise ValueError("flatten_records: classes must be sorted and distinct")
    for im in images:
        A = im["dt_match"].shape[0] if A is None else A
        T = im["dt_match"].shape[1] if T is None else T
        D, G = len(im["dt_classes"]), len(im["gt_classes"])
        if im["dt_match"].shape != (A, T, D) or im["dt_ignore"].shape != (A, T, D) or im["gt_ignore"].shape != (A, G) or \
                len(im["dt_scores"]) != D or len(im["rank"]) != D:
            raise ValueError("flatten_records: an image record's tables do not have the shapes [%d, %d, D] / [%d, G]" % (A, T, A))
    A, T = int(A or 0), int(T or 0)

    def cat(parts, dtype, shape, axis=0):
        return np.ascontiguousarray(np.concatenate(parts, axis=axis), dtype) if parts else np.zeros(shape, dtype)

    rank = cat([im["rank"] for im in images], np.int32, 0)
    keep = rank < max(int(m) for m in max_dets)
    matched = cat([im["dt_match"] for im in images], np.int32, (A, T, 0), 2) >= 0
    ignored = cat([im["dt_ignore"] for im in images], np.uint8, (A, T, 0), 2) != 0
    flags = matched.astype(np.uint8) | (ignored.astype(np.uint8) << 1)
    return {"dt_class_idx": _class_index(cat([im["dt_classes"] for im in images], np.int64, 0)[keep], uniq),
            "dt_score": cat([im["dt_scores"] for im in images], np.float32, 0)[keep],
            "dt_rank": np.ascontiguousarray(rank[keep]),
            "dt_flags": np.ascontiguousarray(flags[:, :, keep]),
            "gt_class_idx": _class_index(cat([im["gt_classes"] for im in images], np.int64, 0), uniq),
            "gt_ignore": cat([im["gt_ignore"] for im in images], np.uint8, (A, 0), 1)}


def accumulate_flat_numpy(flat, K, max_dets, rec_thrs):
    """What csrc/coco_accum.hip computes, stated on the host: one stable sort of all detections by (class, score descending);
    per cell, tp being non-decreasing and c -> c / npig monotone, the first entry with rc >= rec_thrs[r] is the one where tp
    first reaches need_r, the least count c with c / npig >= rec_thrs[r] (entry 0 when need_r == 0); an entry at or above the
    max_det counts as neither tp nor fp and repeats its left neighbour's pr.  -> precision [T, R, K, A, M], recall [T, K, A, M],
    npig int64 [K, A]; equal to accumulate's bit for bit (tests/test_coco_accum_host.py)."""
    cls, rank, flags = flat["dt_class_idx"], flat["dt_rank"], flat["dt_flags"]
    A, T, N = flags.shape
    R, M = len(rec_thrs), len(max_dets)
    score = flat["dt_score"].astype(np.float32) + np.float32(0)
    order = np.lexsort((-score, np.where(cls < 0, K, cls)))                     # (stable: equal keys keep the input order)
    seg = np.searchsorted(np.where(cls < 0, K, cls)[order], np.arange(K + 1))
    npig = np.zeros((K, A), np.int64)
    for a in range(A):
        g = flat["gt_class_idx"][flat["gt_ignore"][a] == 0]
        npig[:, a] = np.bincount(g[g >= 0], minlength=K)[:K]
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        sel = order[seg[k]:seg[k + 1]]
        for a in range(A):
            if npig[k, a] == 0:
                continue
            counts = np.arange(len(sel) + 2, dtype=np.float64) / float(npig[k, a])
            need = np.searchsorted(counts, rec_thrs, side="left")                 # the least c with c / npig >= the threshold
            for m, max_det in enumerate(max_dets):
                inside = rank[sel] < max_det
                for t in range(T):
                    f = flags[a, t, sel]
                    tp, fp = np.cumsum(inside & (f == 1)), np.cumsum(inside & (f == 0))
                    recall[t, k, a, m] = (tp[-1] / float(npig[k, a])) if len(sel) else 0.0
                    pr = tp.astype(np.float64) / ((fp + tp).astype(np.float64) + np.spacing(1))
                    best = np.maximum.accumulate(pr[::-1])[::-1]
                    at = np.where(need == 0, 0, np.searchsorted(tp, need, side="left"))
                    q = np.zeros(R)
                    q[at < len(sel)] = best[at[at < len(sel)]]
                    precision[t, :, k, a, m] = q
    return precision, recall, npig


def _check_flat(who, flat, K, T, A, max_dets, rec_thrs):
    """mnc_coco_accumulate's refusals (ValueError in the place of MNC_ERR_INVALID)."""
    N, Gn = len(flat["dt_class_idx"]), len(flat["gt_class_idx"])
    if N > ACCUM_MAX_N or Gn > ACCUM_MAX_N:
        raise ValueError("%s: %d detections / %d ground truths not in [0, 2^24]" % (who, N, Gn))
    if not 1 <= K <= ACCUM_MAX_K or not 1 <= T <= MAX_T or not 1 <= A <= MAX_A or not 1 <= len(max_dets) <= ACCUM_MAX_M or \
            not 1 <= len(rec_thrs) <= ACCUM_MAX_R:
        raise ValueError("%s: K=%d not in [1, %d], T=%d not in [1, %d], A=%d not in [1, %d], M=%d not in [1, %d] or R=%d not in [1, %d]"
                         % (who, K, ACCUM_MAX_K, T, MAX_T, A, MAX_A, len(max_dets), ACCUM_MAX_M, len(rec_thrs), ACCUM_MAX_R))
    if any(not 1 <= m <= MAX_N for m in max_dets):
        raise ValueError("%s: a max_det not in [1, %d]" % (who, MAX_N))
    if np.isnan(rec_thrs).any() or np.isnan(flat["dt_score"]).any():
        raise ValueError("%s: a NaN score or recall threshold" % who)
    if (flat["dt_rank"] < 0).any():
        raise ValueError("%s: a negative rank" % who)
    if flat["dt_flags"].shape != (A, T, N) or flat["gt_ignore"].shape != (A, Gn) or (flat["gt_ignore"] > 1).any():
        raise ValueError("%s: tables not of the shapes [%d, %d, N] / [%d, Gn], or an ignore value other than 0 / 1" % (who, A, T, A))


def accumulate_flat(flat, K, max_dets, rec_thrs, device_id=None):
    """mnc_coco_accumulate on the flat arrays of flatten_records (T and A are the planes of flat["dt_flags"]).  -> precision
    [T, R, K, A, M], recall [T, K, A, M], npig int64 [K, A]."""
    from .masks import _device_id
    A, T = flat["dt_flags"].shape[:2]
    max_dets = [int(m) for m in max_dets]
    rec_thrs = np.ascontiguousarray(rec_thrs, np.float64).reshape(-1)
    _check_flat("accumulate_flat", flat, K, T, A, max_dets, rec_thrs)
    R, M = len(rec_thrs), len(max_dets)
    precision, recall, npig = np.zeros((T, R, K, A, M)), np.zeros((T, K, A, M)), np.zeros((K, A), np.int64)
    md = np.asarray(max_dets, np.int32)
    _lib.call("mnc_coco_accumulate", _lib.ptr(flat["dt_class_idx"]), _lib.ptr(flat["dt_score"]), _lib.ptr(flat["dt_rank"]),
              _lib.ptr(flat["dt_flags"]), len(flat["dt_class_idx"]), _lib.ptr(flat["gt_class_idx"]), _lib.ptr(flat["gt_ignore"]),
              len(flat["gt_class_idx"]), K, T, A, _lib.ptr(md), M, _lib.ptr(rec_thrs), R, _lib.ptr(precision), _lib.ptr(recall),
              _lib.ptr(npig), _device_id(device_id))
    return precision, recall, npig


def accumulate_device(images, iou_thrs=None, area_rngs=None, max_dets=MAX_DETS, classes=None, rec_thrs=None, device_id=None):
    """accumulate on the GPU (mnc_coco_accumulate, csrc/coco_accum.hip): the same arguments, the same dict, the same bits.  The
    records are flattened on the host (flatten_records), sorted and accumulated in one call.  Invalid arguments raise ValueError or
    _lib.MncError (MNC_ERR_INVALID) before anything is launched; without the library or a GPU it raises."""
    thrs, rngs, max_dets, rec_thrs = _accum_params(iou_thrs, area_rngs, max_dets, rec_thrs)
    images = list(images)
    classes = _class_list(images, classes)
    T, R, K, A, M = len(thrs), len(rec_thrs), len(classes), len(rngs), len(max_dets)
    out = {"classes": classes, "iou_thrs": thrs, "area_rngs": rngs, "max_dets": max_dets, "rec_thrs": rec_thrs}
    if K == 0:                                                     # nothing to evaluate: accumulate's empty tables
        return dict(out, precision=-np.ones((T, R, 0, A, M)), recall=-np.ones((T, 0, A, M)))
    if M == 0:
        raise ValueError("accumulate_device: no max_dets")
    uniq, inverse = np.unique(np.asarray(classes, np.int64), return_inverse=True)
    flat = flatten_records(images, uniq, max_dets, T, A)
    precision, recall, _ = accumulate_flat(flat, len(uniq), max_dets, rec_thrs, device_id)
    if len(uniq) != K or (inverse != np.arange(K)).any():          # classes given unsorted or twice: the tables in their order
        precision, recall = np.ascontiguousarray(precision[:, :, inverse]), np.ascontiguousarray(recall[:, inverse])
    return dict(out, precision=precision, recall=recall)


def _mean(s):
    s = s[s > -1]
    return float(np.mean(s)) if s.size else -1.0


def summarize(acc):
    """-> OrderedDict of the twelve COCO numbers (STAT_NAMES), each the mean over the entries > -1 of its slice, -1 when there are
    none: AP over all thresholds, at 0.5 and at 0.75 (all areas, the last of max_dets), AP small / medium / large; AR at the three
    max_dets (all areas), AR small / medium / large (area ranges 1, 2, 3 in the order given).  A slice the parameters do not have
    (fewer area ranges or max_dets, no threshold 0.5 / 0.75) is -1."""
    p, r = acc["precision"], acc["recall"]
    A, M = p.shape[3], p.shape[4]

    def thr(v):
        return np.flatnonzero(np.isclose(acc["iou_thrs"], v))

    def ap(a, t=None):
        if a >= A:
            return -1.0
        s = p[:, :, :, a, M - 1]
        return _mean(s if t is None else s[thr(t)])

    def ar(a, m):
        return _mean(r[:, :, a, m]) if a < A and 0 <= m < M else -1.0

    vals = [ap(0), ap(0, .5), ap(0, .75), ap(1), ap(2), ap(3), ar(0, M - 3), ar(0, M - 2), ar(0, M - 1), ar(1, M - 1), ar(2, M - 1),
            ar(3, M - 1)]
    return collections.OrderedDict(zip(STAT_NAMES, vals))


def summary_lines(acc, stats):
    """The twelve lines in COCO's wording."""
    thrs, M = acc["iou_thrs"], acc["max_dets"]
    span = "%0.2f:%0.2f" % (thrs[0], thrs[-1])
    rows = [(1, span, 0, -1), (1, "0.50", 0, -1), (1, "0.75", 0, -1), (1, span, 1, -1), (1, span, 2, -1), (1, span, 3, -1),
            (0, span, 0, -3), (0, span, 0, -2), (0, span, 0, -1), (0, span, 1, -1), (0, span, 2, -1), (0, span, 3, -1)]
    out = []
    for (is_ap, iou, a, m), value in zip(rows, stats):
        out.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if is_ap else "Average Recall", "(AP)" if is_ap else "(AR)", iou, AREA_LABELS[a],
            M[m] if -m <= len(M) else -1, value))
    return out


class CocoSegmEval(object):
    """COCO's segm protocol over the images added.  device=True matches on the GPU (PackedMasks.match: a device-resident result
    where it lies), device=False with match_numpy, so that the whole path works without one.  accumulate_on_device: the tables
    through accumulate_device (True) or accumulate (False); None: as `device`.  device=False with nothing else said never touches
    the GPU.  The tables, and so the stats, are the same bits either way.  iou_type="boundary": COCO's boundary protocol -- the
    matching on min(mask IoU, boundary IoU) (match_boundary / match_boundary_numpy) at dilation_ratio of the image diagonal; add()
    then needs image_size=(H, W).  With "segm" (the default) neither argument is looked at."""

    def __init__(self, iou_thrs=None, area_rngs=None, max_dets=MAX_DETS, device=True, classes=None, accumulate_on_device=None,
                 iou_type="segm", dilation_ratio=0.02):
        if iou_type not in ("segm", "boundary"):
            raise ValueError("CocoSegmEval: iou_type %r is not 'segm' or 'boundary'" % (iou_type,))
        self.iou_type, self.dilation_ratio = iou_type, float(dilation_ratio)
        self.iou_thrs = np.asarray(IOU_THRS if iou_thrs is None else iou_thrs, np.float64).reshape(-1)
        self.area_rngs = np.asarray(AREA_RNGS if area_rngs is None else area_rngs, np.float64).reshape(-1, 2)
        self.max_dets = tuple(int(m) for m in max_dets)
        self.device, self.classes = bool(device), classes
        self.accumulate_on_device = self.device if accumulate_on_device is None else bool(accumulate_on_device)
        self._images = {}
        self.eval = self.stats = None

    def add(self, image_id, dt, gt, iscrowd, ignore=None, eval_area=None, image_size=None):
        """Match one image's detections to its ground truths (max_det = the largest of max_dets) and keep the tables.  image_size:
        (H, W), required with iou_type="boundary" (ValueError without it), ignored with "segm".  -> Match."""
        if image_id in self._images:
            raise ValueError("CocoSegmEval.add: image %r was added before" % (image_id,))
        args = (gt, iscrowd, ignore, eval_area, self.iou_thrs, self.area_rngs, max(self.max_dets))
        if self.iou_type == "boundary":
            if image_size is None:
                raise ValueError("CocoSegmEval.add: iou_type='boundary' needs image_size=(H, W) of image %r" % (image_id,))
            H, W = (int(v) for v in image_size)
            args = (gt, H, W) + args[1:] + (None, self.dilation_ratio)
            m = dt.match_boundary(*args) if self.device else match_boundary_numpy(dt, *args)
        else:
            m = dt.match(*args) if self.device else match_numpy(dt, *args)
        self._images[image_id] = image_record(dt, gt, m)
        return m

    def accumulate(self):
        """Images in the order of their sorted ids, as the published evaluator takes them."""
        try:
            ids = sorted(self._images)
        except TypeError:
            ids = list(self._images)
        run = accumulate_device if self.accumulate_on_device else accumulate
        self.eval = run([self._images[i] for i in ids], self.iou_thrs, self.area_rngs, self.max_dets, self.classes)
        return self.eval

    def summarize(self):
        if self.eval is None:
            self.accumulate()
        out = summarize(self.eval)
        self.stats = np.array(list(out.values()), np.float64)
        return out

    def lines(self):
        if self.stats is None:
            self.summarize()
        return summary_lines(self.eval, self.stats)
