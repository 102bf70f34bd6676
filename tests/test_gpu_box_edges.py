"""GPU: the library entries on the on-threshold corpora of tests/box_edge_inputs.py -- NMS at 0.3f / 0.5f / 0.7f, voting membership
at IoU exactly 1/2, binarisation at 0.4f, score selection, ROIPooling's rounding and bin edges -- against the plain statements
there, the CPU oracle and, where oracle/_ref is built, the reference's own .cu code.  Every comparison is exact.  The corpus
properties and the variations each case tells apart are checked without a GPU in tests/test_box_edges_host.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import box_edge_inputs as BE  # noqa: E402
import mnc_amd  # noqa: E402
from gpu_util import Dev, to_c8  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from oracle import host as ohost  # noqa: E402
from oracle import native  # noqa: E402

pytestmark = pytest.mark.gpu
mnc_amd.install_paths()
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def _nms(dets, thr, max_keep=None):
    n = len(dets)
    keep, num = np.full(n, -1, np.int32), ctypes.c_int(-1)
    if max_keep is None:
        _lib.call("mnc_nms", _lib.ptr(keep), ctypes.addressof(num), _lib.ptr(dets), n, 5, float(thr), 0)
    else:
        _lib.call("mnc_nms_topk", _lib.ptr(keep), ctypes.addressof(num), _lib.ptr(dets), n, 5, float(thr), int(max_keep), 0)
    return list(keep[:num.value])


def _mask(dets, thr):
    n = len(dets)
    words = np.full((n, (n + 63) // 64), 0xFFFFFFFFFFFFFFFF, np.uint64)
    _lib.call("mnc_nms_mask", _lib.ptr(words), _lib.ptr(dets), n, 5, float(thr), 0)
    return words


def _check_mask(dets, thr, bits):
    """Column tiles >= the row tile equal the statement's words; the tiles below, which the scan never reads, are 0."""
    n = len(dets)
    got, want = _mask(dets, thr), BE.mask_words(bits)
    upper = np.arange(want.shape[1])[None, :] >= np.arange(n)[:, None] // 64
    assert np.array_equal(got[upper], want[upper]) and not got[~upper].any()


@pytest.mark.parametrize("t", BE.NMS_THRESHOLDS)
def test_nms_on_threshold_pairs(t):
    """mnc_nms, mnc_nms_mask, mnc_nms_topk and nms.gpu_nms: j goes iff the float32 IoU is the float ABOVE the threshold."""
    from nms.gpu_nms import gpu_nms
    runs = 0
    for (tt, cls, k, i, j, n) in BE.nms_placements():
        if tt != t:
            continue
        dets = BE.place_pair(BE.NMS_PAIRS[(t, cls)][k], i, j, n)
        bits, keep = BE.nms_statement(dets, t)
        assert (j not in keep) == (cls == "above")
        assert _nms(dets, t) == keep, (cls, i, j, n)
        _check_mask(dets, t, bits)
        word = _mask(dets, t)[i, j // 64]
        assert word == (np.uint64(1) << np.uint64(j % 64) if cls == "above" else 0)
        # the cut before, at and after j: keep[:m] of the full list, m counted in survivors
        at = keep.index(j) + 1 if j in keep else j
        for m in (max(at - 1, 1), at, min(at + 1, n)):
            assert _nms(dets, t, m) == keep[:m], (cls, i, j, n, m)
        # nms.gpu_nms sorts by score itself: shuffled rows, indices into the shuffled array
        perm = np.random.default_rng(n + j).permutation(n)
        assert gpu_nms(np.ascontiguousarray(dets[perm]), t, 0) == [int(np.where(perm == p)[0][0]) for p in keep]
        runs += 1
    assert runs == 14 * sum(1 for key in BE.NMS_PAIRS if key[0] == t)      # 8 positions, 14 (position, size) each class


@pytest.mark.parametrize("t", (0.3, 0.7))
def test_nms_batched_same_pair_at_three_positions(t):
    """mnc_nms_batched: three score columns put one pair at (0, 1), (63, 64) and (64, 128) of 129 boxes."""
    from nms.gpu_nms import gpu_nms_batched
    n = 129
    for cls in ("below", "on", "above"):
        pair = BE.NMS_PAIRS[(t, cls)][3]
        base = BE.place_pair(pair, 0, 1, n)
        scores, want = np.zeros((n, 3), np.float32), []
        for b, (i, j) in enumerate(((0, 1), (63, 64), (64, 128))):
            rest = [p for p in range(2, n)]
            order = rest[:i] + [0] + rest[i:j - 1] + [1] + rest[j - 1:]
            assert len(order) == n and order[i] == 0 and order[j] == 1
            scores[order, b] = 1.0 - np.arange(n) / 256.0
            _, keep = BE.nms_statement(base[order], t)
            assert (j not in keep) == (cls == "above")
            want.append([order[p] for p in keep])
        got = gpu_nms_batched(np.ascontiguousarray(base[:, :4]), scores, t, 0)
        assert [list(g) for g in got] == want, cls
        top = gpu_nms_batched(np.ascontiguousarray(base[:, :4]), scores, t, 0, max_keep=64)
        assert [list(g) for g in top] == [w[:64] for w in want], cls


def test_nms_degenerate_boxes():
    for name, dets, thr, want in BE.degenerate_cases():
        bits, keep = BE.nms_statement(dets, thr)
        assert want is None or keep == want
        assert _nms(dets, thr) == keep, name
        _check_mask(dets, thr, bits)


def test_bbox_overlaps_on_integer_pairs():
    from utils.cython_bbox import bbox_overlaps
    pairs = list(BE.HALF_PAIRS) + list(BE.NEAR_HALF.values()) + [p for p, _ in BE.TOUCHING_PAIRS]
    a, b = np.array([p[0] for p in pairs], np.float64), np.array([p[1] for p in pairs], np.float64)
    for x, y in ((a, b), (b, a)):
        got = bbox_overlaps(x, y)
        assert np.array_equal(got, BE.overlaps_statement(x, y)) and np.array_equal(got, native.bbox_overlaps(x, y))
    d = np.diag(bbox_overlaps(a, b))
    nh = len(BE.HALF_PAIRS)
    assert (d[:nh] == 0.5).all() and d[nh] < 0.5 < d[nh + 1]
    assert [v > 0 for v in d[nh + 2:]] == [inter > 0 for _, inter in BE.TOUCHING_PAIRS]


@pytest.mark.parametrize("n,m_index", BE.VOTING_SETS)
def test_voting_member_at_exactly_one_half(n, m_index):
    """mnc_mask_voting (fused) and the generic composition: M at IoU exactly 1/2 is a member of K's set, L just below is not."""
    from transform import mask_transform as mt
    v = BE.voting_set(n, m_index)
    args = (v["masks"], v["boxes"], v["scores"], v["num_classes"], v["max_per_image"], v["W"], v["H"])
    want = ohost.gpu_mask_voting(*args)
    fused = mt.gpu_mask_voting(*args)
    generic = mt.gpu_mask_voting(v["masks"], v["boxes"].astype(np.float64), *args[2:])
    wants = [want]
    if native.ref_available():
        wants.append(ohost.gpu_mask_voting(*args, nms_fn=native.ref_gpu_nms, mv_fn=native.ref_mv))
    for w in wants:
        for got in (fused, generic):
            assert [len(b) for b in got[1]] == [len(b) for b in w[1]]
            assert np.array_equal(np.concatenate(got[1], 0), np.concatenate(w[1], 0))
            assert np.array_equal(np.concatenate(got[0], 0), np.concatenate(w[0], 0))
    assert np.array_equal(fused[1][0][0, :4], [10, 10, 49, 39])           # M's mask carries K's box to x = 49
    # mnc_mask_voting itself, with the caller's own order
    B = v["num_classes"] - 1
    order = np.stack([np.argsort(-v["scores"][:, c + 1], kind="stable") for c in range(B)]).astype(np.int32)
    cap = B * min(v["max_per_image"], n)
    om, ob, osc = np.zeros((cap, 1, 21, 21), np.float32), np.zeros((cap, 4), np.int32), np.zeros(cap, np.float32)
    cnt, R = np.zeros(B, np.int32), ctypes.c_int(0)
    _lib.call("mnc_mask_voting", _lib.ptr(v["boxes"]), _lib.ptr(v["masks"]), _lib.ptr(v["scores"]), _lib.ptr(order), n,
              v["num_classes"], 21, v["max_per_image"], float(ohost.MASK_MERGE_NMS_THRESH), float(ohost.MASK_MERGE_IOU_THRESH),
              v["H"], v["W"], _lib.ptr(om), _lib.ptr(ob), _lib.ptr(osc), _lib.ptr(cnt), ctypes.addressof(R), 0)
    assert list(cnt) == [len(b) for b in want[1]]
    assert np.array_equal(om[:R.value], np.concatenate(want[0], 0))
    assert np.array_equal(ob[:R.value], np.concatenate(want[1], 0)[:, :4].astype(np.int32))


def test_mv_binarises_strictly_at_float_0p4():
    """mnc_mv: an aggregate of exactly 0.4f is NOT above the threshold (the centre fallback); the float above it is."""
    from nms.mv import mv
    for name, c in BE.mv_cases():
        gm, gb = mv(*BE.mv_args(c))
        om, ob = native.mv(*BE.mv_args(c))
        assert np.array_equal(gb[0], BE.mv_box_statement(c)), name
        assert np.array_equal(gb, ob) and np.array_equal(gm, om), name
        if native.ref_available():
            rm, rb = native.ref_mv(*BE.mv_args(c))
            assert np.array_equal(gb, rb) and np.array_equal(gm, rm), name


def test_image_voting_binarises_non_strictly_at_float32_0p4():
    """mnc_mask_voting_image: `masks >= cfg.BINARIZE_THRESH` on a float32 mask (mask_transform.py:122) is a float32 comparison,
    so 0.4f is inside; the float below it is not."""
    for name, level in BE.BIN_LEVELS:
        c = BE.image_vote_case(level)
        om, ob, osc = np.zeros((1, 441), np.float32), np.zeros((1, 4), np.int32), np.zeros(1, np.float32)
        cnt, R = np.zeros(1, np.int32), ctypes.c_int(0)
        _lib.call("mnc_mask_voting_image", _lib.ptr(c["boxes"]), _lib.ptr(c["masks"]), _lib.ptr(c["scores"]), 1, 2, 21, 100, 0.3, 0.5,
                  float(BE.BIN), c["H"], c["W"], _lib.ptr(om), _lib.ptr(ob), _lib.ptr(osc), _lib.ptr(cnt), ctypes.addressof(R), 0)
        box, mask = BE.image_vote_statement(c)
        assert R.value == 1 and list(cnt) == [1]
        assert np.array_equal(ob[0], box) and np.array_equal(om[0].reshape(21, 21), mask), name


def test_instance_masks_binarise_non_strictly_at_float32_0p4():
    from transform.mask_transform import instance_masks
    boxes, masks, H, W = BE.instance_mask_case()
    want = BE.instance_mask_statement(masks)
    pm = instance_masks(boxes, masks, H, W, binarize_thresh=BE.BIN)
    for i in range(len(boxes)):
        assert np.array_equal(pm.dense(i), want[i]), i
    assert list(pm.areas) == [0, 441, 441, 440]


@pytest.mark.parametrize("thr,scores,kept", BE.SCORE_CASES)
def test_record_selection_widens_the_score(dev, thr, scores, kept):
    """mnc_mask_records and mnc_render_records keep a record iff (double)score >= thresh."""
    from mnc_amd.instances import HEAD_BYTES
    from mnc_amd.masks import records_masks
    S, H, W, cap = 21, BE.MV_H, BE.MV_W, 8
    rec = np.zeros((cap, 6 + S * S), np.float32)
    for r, s in enumerate(scores):
        rec[r, :6] = (5 + 22 * r, 4, 25 + 22 * r, 24, s, 1 + r)
        rec[r, 6:] = 0.9
    head = np.zeros(HEAD_BYTES // 4, np.int32)
    head[0] = len(scores)
    want = BE.score_statement(scores, thr)
    assert tuple(want) == kept
    d_rec, d_cnt = dev.put(rec), dev.put(head, np.int32)
    pm = records_masks(dev, d_rec, d_cnt, cap, 21, S, H, W, thr, BE.BIN).fetch()
    assert len(pm) == int(want.sum()) and list(pm.classes) == [1 + r for r in range(len(scores)) if want[r]]
    assert np.array_equal(pm.scores, np.array(scores, np.float32)[want])
    d_inst, d_kept = dev.empty((H * W,), np.int32, fill=-7), dev.empty((1,), np.int32, fill=-1)
    dev.call("mnc_render_records", d_rec, d_cnt, cap, 21, S, float(thr), float(BE.BIN), H, W, None, 0.8, d_inst, None, None, None,
             None, d_kept)
    dev.sync()
    assert int(dev.get(d_kept, (1,), np.int32)[0]) == int(want.sum())
    inst = dev.get(d_inst, (H, W), np.int32)
    assert sorted(set(inst.ravel()) - {0}) == list(range(1, int(want.sum()) + 1))


@pytest.mark.parametrize("P", BE.ROI_P)
def test_roi_pool_rounding_and_bin_edges(dev, P):
    """mnc_roi_pool: corners round half away from zero (0.5 -> 1, 2.5 -> 3, -0.5 -> -1, 0.49999997 -> 0) and the bin edges are
    the float32 floor / ceil, including the sides at which ceilf lands one above the exact rational."""
    feat, rois = BE.roi_feature(), BE.roi_cases()
    C, H, W, R = BE.ROI_C, BE.ROI_H, BE.ROI_W, len(rois)
    d_out = dev.empty((R * P * P * C,), fill=np.nan)
    dev.call("mnc_roi_pool", dev.put(to_c8(feat[0])[None]), 1, C, H, W, dev.put(rois), R, P, P, BE.ROI_SCALE, d_out)
    got = dev.get(d_out, (R, P, P, C)).transpose(0, 3, 1, 2)
    assert np.array_equal(got, BE.roi_pool_statement(feat, rois, P, P))
    assert np.array_equal(got, native.roi_pool(feat, rois, P, P, BE.ROI_SCALE))
