"""Per-instance binary masks at image resolution on the GPU (csrc/inst_masks.hip: mnc_instance_masks, mnc_mask_records,
mnc_net_masks and the Python surfaces over them) against the numpy statement of the rule (instance_masks_numpy, which
tests/test_instance_masks_host.py pins to the reference's golden label map) and against the entries that are already pinned
(mnc_render_instances, mnc_sds_best_overlap).  Every comparison is exact, padding bits included."""
import ctypes
import glob
import io
import os
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import render_inputs as RI  # noqa: E402
from mnc_amd import _lib, models, synth  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, InstanceBlock, records_from_lists, split_records  # noqa: E402
from mnc_amd.masks import HEAD, INFO, PackedMasks, from_lists, instance_masks_call, records_masks  # noqa: E402
from mnc_amd.native_net import ImageStream, NativeNet  # noqa: E402
from mnc_config import cfg  # noqa: E402
from transform.mask_transform import instance_masks, instance_masks_numpy  # noqa: E402
from utils import vis_seg  # noqa: E402
from utils.voc_eval import pack_sds_gt, sds_best_overlap  # noqa: E402

pytestmark = pytest.mark.gpu

S = RI.S
H, W = 70, 130
WIDTHS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129]      # word and strip boundaries, the narrow-box folding
HEIGHTS = [1, 2, 21, 50]                                           # below, at and above the mask's own size


def _same(got, want):
    for f in PackedMasks.FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
    return True


def _masks(rng, n, size=S):
    if size == S:
        return np.stack([RI._mask(rng, int(rng.integers(0, 4))) for _ in range(n)])
    yy, xx = np.mgrid[0:size, 0:size]
    return np.stack([(0.5 + 0.5 * np.sin(rng.uniform(0, 6) + rng.uniform(0.2, 0.9) * xx + rng.uniform(0.2, 0.9) * yy)).astype(np.float32)
                     for _ in range(n)])


def _both(boxes, masks, clip, thr=None, h=H, w=W):
    got = instance_masks(boxes, masks, h, w, clip=clip, binarize_thresh=thr)
    want = instance_masks_numpy(boxes, masks, h, w, clip=clip, binarize_thresh=thr)
    assert _same(got, want)
    return got


def test_widths_and_heights_at_every_boundary():
    rng = np.random.default_rng(1)
    boxes = []
    for w in WIDTHS:
        for h in HEIGHTS:
            x1, y1 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
            boxes.append([x1, y1, x1 + w - 1, y1 + h - 1])
    boxes = np.array(boxes, np.float64)
    masks = _masks(rng, len(boxes))
    for clip in (True, False):
        pm = _both(boxes, masks, clip)
        assert sorted({pm.size(i) for i in range(len(pm))}) == sorted((h, w) for w in WIDTHS for h in HEIGHTS)
        assert 0 < pm.areas.sum() < sum(w * h for w in WIDTHS for h in HEIGHTS)


def test_rounding_and_clipping():
    rng = np.random.default_rng(2)
    boxes = np.array([[10.5, 11.5, 40.5, 41.5], [11.5, 10.5, 41.5, 40.5], [0.5, 1.5, 2.5, 3.5],          # x.5: half to even
                      [0.0, 0.0, 30.0, 20.0], [-0.49, -0.5, 30.0, 20.0], [W - 31.0, H - 21.0, W - 1.0, H - 1.0],   # touching
                      [-7.3, 5.0, 25.0, 30.0], [5.0, -9.8, 25.0, 30.0], [100.0, 30.0, W + 12.6, 60.0],     # crossing each border
                      [20.0, 40.0, 90.0, H + 8.2], [-5.2, -3.7, W + 4.1, H + 6.3],                        # ... and all four
                      [0.0, 0.0, W - 1.0, H - 1.0]])                                                       # the whole image
    masks = _masks(rng, len(boxes))
    clipped = _both(boxes, masks, True)
    assert clipped.bounds[:, :2].min() == 0 and clipped.bounds[:, 2].max() == W - 1 and clipped.bounds[:, 3].max() == H - 1
    assert clipped.size(len(boxes) - 1) == (H, W)
    free = _both(boxes, masks, False)
    assert free.bounds[:, 0].min() < 0 and free.bounds[:, 1].min() < 0 and free.bounds[:, 2].max() > W - 1
    assert np.array_equal(free.bounds[:3], [[10, 12, 40, 42], [12, 10, 42, 40], [0, 2, 2, 4]])


def test_threshold_edge_and_constant_masks():
    t = np.float32(0.4)
    below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))
    vals = [t, below, above, np.float32(0), np.float32(1)]
    checker = np.where(np.add.outer(np.arange(S), np.arange(S)) % 2, below, t).astype(np.float32)
    masks = np.stack([np.full((S, S), v, np.float32) for v in vals] + [checker])
    boxes = np.array([[3, 4, 3 + 99, 4 + 44]] * len(masks), np.float64)
    pm = _both(boxes, masks, True, 0.4)
    w, h = 100, 45
    assert pm.areas[3] == 0 and not pm.bits[pm.offsets[3] // 8:pm.offsets[4] // 8].any()                  # all 0: every word 0
    assert pm.areas[4] == w * h and pm.dense(4).all()                                                      # all 1
    ones = pm.bits[pm.offsets[4] // 8:pm.offsets[5] // 8].reshape(h, 2)
    assert (ones[:, 0] == np.uint64(2 ** 64 - 1)).all() and (ones[:, 1] == np.uint64(2 ** 36 - 1)).all()  # padding bits 0
    assert 0 < pm.areas[5] < w * h


@pytest.mark.parametrize("size", [7, 32])
def test_other_mask_sizes(size):
    rng = np.random.default_rng(size)
    boxes = np.array([[4, 3, 4 + w - 1, 3 + h - 1] for w, h in ((5, 60), (33, 9), (64, 31), (120, 66), (size, size))], np.float64)
    _both(boxes, _masks(rng, len(boxes), size), True)


def test_no_instance_and_more_instances_than_one_round_of_workgroups():
    empty = instance_masks(np.zeros((0, 4)), np.zeros((0, S, S), np.float32), H, W)
    assert len(empty) == 0 and empty.bits.size == 0 and empty.bounds.shape == (0, 4)
    rng = np.random.default_rng(5)
    n = 300
    x = np.sort(rng.uniform(-12, 412, (n, 2)), 1)
    y = np.sort(rng.uniform(-12, 1212, (n, 2)), 1)
    boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1], rng.uniform(0, 1, n)], 1)
    classes = rng.integers(1, 21, n)
    masks = _masks(rng, n)
    got = instance_masks(boxes, masks, 1200, 400, classes=classes)
    assert _same(got, instance_masks_numpy(boxes, masks, 1200, 400, classes=classes))
    assert np.array_equal(got.scores, boxes[:, 4].astype(np.float32)) and np.array_equal(got.classes, classes)
    # more work items (32 rows of a box wider than 32 columns) than the launch has workgroups: the grid-stride walk
    assert sum(-(-got.size(i)[0] // 32) for i in range(n) if got.size(i)[1] > 32) > 2048


def test_invalid_arguments_launch_nothing_and_a_valid_call_follows():
    rng = np.random.default_rng(3)
    mk = _masks(rng, 3).reshape(3, -1)
    good = np.array([[5.0, 6.0, 40.0, 50.0], [20.0, 10.0, 70.0, 30.0], [1.0, 1.0, 9.0, 9.0]])
    inverted = good.copy()
    inverted[1] = [50.0, 10.0, 10.0, 40.0]
    want = instance_masks_numpy(good, mk.reshape(3, S, S), H, W)
    words = want.bits.size
    for args, cap in (((inverted, mk, 3, S, H, W, True), words), ((good, np.zeros((3, 33 * 33), np.float32), 3, 33, H, W, True), words),
                      ((good, mk, 3, S, H, 0, True), words), ((good * 2.0 ** 23, mk, 3, S, H, W, False), words),
                      ((good, mk, 3, S, H, W, True), words - 1)):                          # (the last one: bits_cap too small)
        sentinel = np.full(cap, 0x5A5A, np.uint64)
        with pytest.raises(_lib.MncError) as e:
            instance_masks_call(*(args + (0.4, sentinel)))
        assert e.value.code == 1                                              # MNC_ERR_INVALID
        assert (sentinel == 0x5A5A).all()                                     # nothing was written
        assert _same(instance_masks(good, mk.reshape(3, S, S), H, W), want)  # the valid call that follows


def test_cross_check_against_the_render_and_the_evaluation_entries():
    rng = np.random.default_rng(7)
    n = 12
    x = np.sort(rng.uniform(-10, W + 10, (n, 2)), 1)
    y = np.sort(rng.uniform(-10, H + 10, (n, 2)), 1)
    boxes = np.stack([x[:, 0], y[:, 0], x[:, 1] + 1, y[:, 1] + 1], 1)
    masks = _masks(rng, n)
    classes = [int(c) for c in rng.integers(1, 21, n)]
    # painting the masks in list order == mnc_render_instances' instance image
    pm = instance_masks(boxes, masks, H, W, clip=True)
    pred = {"boxes": [np.append(b, 1.0) for b in boxes], "masks": list(masks), "cls_name": classes}
    inst, _ = vis_seg._convert_pred_to_image_device(W, H, pred)
    paint = np.zeros((H, W), inst.dtype)
    for i in range(n):
        paint[pm.full(i, H, W)] = i + 1
    assert paint.max() > 3 and np.array_equal(paint, inst)
    # mnc_sds_best_overlap against one ground truth covering the whole rounded box: its intersection is the mask's area
    m01 = (masks >= 0.5).astype(np.uint8)                                     # (that entry takes 0 / 1 byte masks)
    free = instance_masks(boxes, m01.astype(np.float32), H, W, clip=False)
    gts = [{"mask_bound": free.bounds[i].astype(np.float64), "mask": np.ones(free.size(i), bool)} for i in range(n)]
    gb, go, gbits, ga, _ = pack_sds_gt(gts)
    best, inter, union = sds_best_overlap(boxes, m01.reshape(n, -1), np.arange(n), np.arange(1, n + 1), gb, go, gbits, ga,
                                          cfg.BINARIZE_THRESH)
    assert np.array_equal(best, np.arange(n)) and np.array_equal(inter, free.areas) and np.array_equal(union, ga)
    assert 0 < free.areas.sum() < ga.sum()


def _block(rec, counts, cap):
    """A device instance block holding `rec`, as the voting leaves it -> (InstanceBlock, its context)."""
    from mnc_amd.engine import _Ctx
    ctx = _Ctx(0)
    blk = InstanceBlock(types.SimpleNamespace(_ctx=ctx), 21, S, 100, 300)
    assert blk.rows_cap >= cap
    head = np.zeros(HEAD_BYTES // 4, np.int32)
    head[:len(counts)] = counts
    raw = np.concatenate((head.view(np.uint8), np.ascontiguousarray(rec).reshape(-1).view(np.uint8)))
    _lib.call("mnc_h2d", ctx.h, blk.ptr, _lib.ptr(raw), raw.nbytes)
    return blk, ctx


@pytest.mark.parametrize("score_thresh", [0.0, 0.5])
def test_mask_records_and_instance_view(score_thresh):
    rng = np.random.default_rng(11)
    h, w = 120, 200
    list_mask, list_box = RI.class_lists(rng, w, h, 0.5)
    cap = 200
    rec, total = records_from_lists(list_mask, list_box, cap, S)
    assert 3 < total < cap
    counts = [total] + [len(b) for b in list_box]
    blk, ctx = _block(rec, counts, cap)
    try:
        lm, lb = split_records(rec[:total], counts[1:], S)
        bxs, mks, classes = from_lists(lm, lb, score_thresh)
        assert (len(bxs) == total) if score_thresh == 0.0 else (3 < len(bxs) < total)
        want = instance_masks(bxs, mks, h, w, clip=True, classes=classes)                  # the host entry on lists()
        assert _same(want, instance_masks_numpy(bxs, mks, h, w, clip=True, classes=classes))
        view = blk.view()
        got = view.masks(h, w, score_thresh=score_thresh)
        assert _same(got, want)
        # the entry itself over the block's whole capacity (rows past the count are not looked at), sizes only and packed
        full = records_masks(ctx, blk.records_ptr, blk.counts_ptr, blk.rows_cap, 21, S, h, w, score_thresh)
        assert _same(full, want)
        stale = view.masks(h, w, score_thresh=score_thresh)
        view.masks(h, w, score_thresh=score_thresh)
        with pytest.raises(RuntimeError):
            stale.bounds                                                                   # a later masks() reused the buffers
        d_info = ctypes.c_void_p()
        _lib.call("mnc_mask_records", ctx.h, blk.records_ptr, blk.counts_ptr, blk.rows_cap, 21, S, float(score_thresh),
                  float(cfg.BINARIZE_THRESH), h, w, ctypes.addressof(d_info), None)       # d_bits NULL: sizes only
        raw = np.zeros(HEAD_BYTES + len(want) * INFO.itemsize, np.uint8)
        _lib.call("mnc_d2h", ctx.h, _lib.ptr(raw), d_info.value, raw.nbytes)
        head, info = raw[:HEAD_BYTES].view(HEAD)[0], raw[HEAD_BYTES:].view(INFO)
        assert head["kept"] == len(want) and head["bits_bytes"] == want.bits.nbytes
        assert np.array_equal(info["bounds"], want.bounds) and np.array_equal(info["offset"], want.offsets) and not info["area"].any()
        # the same rows, in the same order, as mnc_render_records keeps at this threshold
        res = view.render(h, w, vis_thresh=score_thresh)
        paint = np.zeros((h, w), np.int32)
        for i in range(len(want)):
            paint[want.full(i, h, w)] = i + 1
        assert res.kept == len(want) and np.array_equal(res.inst, paint)
    finally:
        blk.release()
        ctx.close()


def _net_and_images(seed=4):
    path = models.write_mnc_5stage_test_prototxt(width_div=8)
    w = synth.synthetic_weights(path, seed=seed)
    rng = np.random.default_rng(12)
    images = [rng.integers(0, 256, ((75, 100) if k % 3 else (90, 120)) + (3,), dtype=np.uint8) for k in range(5)]
    return w, images


def _want_of_records(counts, rec, im, thr):
    lm, lb = split_records(rec, counts[1:], S)
    bxs, mks, classes = from_lists(lm, lb, thr)
    return instance_masks_numpy(bxs, mks, im.shape[0], im.shape[1], clip=True, binarize_thresh=0.4, classes=classes)


def test_native_net_masks_and_the_graph_is_undisturbed():
    w, images = _net_and_images()
    ref = NativeNet(w)
    nat = NativeNet(w)
    try:
        with pytest.raises(_lib.MncError) as e:
            nat.masks()
        assert e.value.code == 4                                              # MNC_ERR_STATE
        want = [ref.forward_image(im) for im in images]
        thr = float(np.median(np.concatenate([r[:, 4] for _, r in want])))
        kept = []
        for k, im in enumerate(images):
            counts, rec = nat.forward_image(im)
            # the records are the ones a net that never packed masks gives: the graph replays as before
            assert np.array_equal(counts, want[k][0]) and np.array_equal(rec, want[k][1], equal_nan=True), k
            assert _same(nat.masks(), _want_of_records(counts, rec, im, 0.0))
            got = nat.masks(score_thresh=thr)
            assert _same(got, _want_of_records(counts, rec, im, thr))
            kept.append(len(got))
            # launch / masks / fetch: the masks of an image in flight, and the fetch after it
            nat.launch(im)
            assert _same(nat.masks(score_thresh=thr), got)
            c2, r2 = nat.fetch()
            assert np.array_equal(c2, counts) and np.array_equal(r2, rec, equal_nan=True)
        assert max(kept) > 0 and min(kept) < int(max(c[0] for c, _ in want))
    finally:
        ref.close()
        nat.close()


def test_image_stream_hands_out_each_images_own_masks():
    w, images = _net_and_images()
    ref = NativeNet(w, use_graph=False)
    try:
        want = [ref.forward_image(im) for im in images]
    finally:
        ref.close()
    thr = float(np.median(np.concatenate([r[:, 4] for _, r in want])))
    st = ImageStream(w, in_flight=3, masks=True, masks_args={"score_thresh": thr})
    try:
        got = list(st.map(images))
    finally:
        st.close()
    assert len(got) == len(images)
    for k, (counts, rec, pm) in enumerate(got):
        assert np.array_equal(counts, want[k][0]) and np.array_equal(rec, want[k][1], equal_nan=True)
        assert _same(pm, _want_of_records(counts, rec, images[k], thr))


def test_demo_save_masks_writes_files_that_load_back(tmp_path):
    import caffe
    import demo
    from transform.mask_transform import gpu_mask_voting
    jpg = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "demo", "*.jpg")))[0]
    proto = models.write_mnc_5stage_test_prototxt(width_div=8)
    with redirect_stdout(io.StringIO()) as buf:
        demo.main(["--def", proto, "--images", jpg, "--no-vis", "--save-masks", str(tmp_path / "dev"), "--vis-thresh", "0.0"])
    name = os.path.splitext(os.path.basename(jpg))[0]
    path = str(tmp_path / "dev" / (name + "_masks.npz"))
    assert os.listdir(str(tmp_path / "dev")) == [name + "_masks.npz"] and path in buf.getvalue()
    got = PackedMasks.load(path)
    # the same image through the same net by hand, and the numpy form of its instances
    net = caffe.Net(proto, synth.synthetic_weights(proto, seed=0), caffe.TEST)
    try:
        im = demo._read_image_bgr(jpg)
        boxes, masks, scores = demo.im_detect(im, net)
        lm, lb = gpu_mask_voting(masks, boxes, scores, 21, 100, im.shape[1], im.shape[0])
        bxs, mks, classes = from_lists(lm, lb, 0.0)
        want = instance_masks_numpy(bxs, mks, im.shape[0], im.shape[1], clip=True, classes=classes)
        assert len(want) > 0 and _same(got, want)
        out, cpu = demo._save_masks(str(tmp_path / "cpu"), name, im.shape, lm, lb, None, 0.0, cpu=True)      # --cpu: the numpy form
        assert _same(PackedMasks.load(out), want) and _same(cpu, want)
    finally:
        net.close()
