"""The visualisation tail on the GPU (csrc/render.hip: mnc_render_instances, mnc_render_records, mnc_net_render and the Python
surfaces over them) against the reference's own golden label maps and against the repository's host functions, bit for bit."""
import os
import pickle
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import golden_inputs as GI  # noqa: E402
import render_inputs as RI  # noqa: E402
from gpu_util import Dev  # noqa: E402
from mnc_amd import _lib, models, synth  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, records_from_lists, split_records  # noqa: E402
from mnc_amd.native_net import ImageStream, NativeNet  # noqa: E402
from mnc_config import cfg  # noqa: E402
from utils import vis_seg  # noqa: E402

pytestmark = pytest.mark.gpu

S = RI.S
CLASSES = tuple("c%d" % i for i in range(1, 21))


def _host_tail(list_mask, list_box, H, W, photo, vis_thresh, alpha=0.8):
    """The host path: get_vis_dict + _convert_pred_to_image + the colour map + Image.blend."""
    import demo
    from PIL import Image
    pred = demo.get_vis_dict(list_box, list_mask, "x", CLASSES, vis_thresh)
    inst, cls = vis_seg._convert_pred_to_image(W, H, pred)
    cm = vis_seg._get_voc_color_map().astype(np.uint8)
    inst_rgb, cls_rgb = cm[inst], cm[cls]
    background = Image.fromarray(np.ascontiguousarray(photo[:, :, ::-1])).convert("RGBA")
    ovl = np.asarray(Image.blend(background, Image.fromarray(cls_rgb).convert("RGBA"), alpha).convert("RGB"))
    return len(pred["boxes"]), inst, cls, inst_rgb, cls_rgb, ovl


def test_render_instances_equals_the_reference_golden():
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_eval_outputs.npz"))
    case = GI.sds_case()
    for ii in (0, 3):
        H, W = case["images"][ii]["im"].shape[:2]
        inst, cls = vis_seg._convert_pred_to_image_device(W, H, GI.vis_pred_dict(case, ii))
        assert inst.dtype == ref["vis_inst_%d" % ii].dtype and cls.dtype == ref["vis_cls_%d" % ii].dtype
        assert np.array_equal(inst, ref["vis_inst_%d" % ii])
        assert np.array_equal(cls, ref["vis_cls_%d" % ii])


def test_render_instances_equals_the_host_function_on_random_cases():
    cases = RI.all_cases()
    cov = RI.coverage(cases)
    assert all(cov.values()), cov
    sizes = {(H, W) for W, H, _, _ in cases}
    assert sizes >= {(2, 2), (375, 500), (600, 1000)} and any(W % 64 for _, W in sizes)
    bad = []
    for k, (W, H, pred, _) in enumerate(cases):
        want = vis_seg._convert_pred_to_image(W, H, pred)
        got = vis_seg._convert_pred_to_image_device(W, H, pred)
        rule = RI.rule_images(W, H, pred, cfg.BINARIZE_THRESH)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[0], rule[0])
                and np.array_equal(got[1], rule[1])):
            bad.append(k)
    assert not bad, bad


def test_more_instances_than_the_tile_list_holds():
    """Past 256 instances on one tile the kernel walks the global list: 300 overlapping instances."""
    rng = np.random.default_rng(5)
    W, H = 90, 40
    boxes = [np.array([rng.uniform(-3, 30), rng.uniform(-3, 10), rng.uniform(40, 95), rng.uniform(20, 45), 1.0]) for _ in range(300)]
    pred = {"boxes": boxes, "masks": [RI._mask(rng, int(rng.integers(0, 4))) for _ in range(300)],
            "cls_name": [int(c) for c in rng.integers(1, 21, 300)]}
    want = vis_seg._convert_pred_to_image(W, H, pred)
    got = vis_seg._convert_pred_to_image_device(W, H, pred)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _render_block(dev, rec, counts, cap, H, W, photo, vis_thresh, alpha=0.8):
    d_rec = dev.put(rec)
    head = np.zeros(HEAD_BYTES // 4, np.int32)
    head[:len(counts)] = counts
    d_cnt = dev.put(head, np.int32)
    d_img = dev.put(photo, np.uint8) if photo is not None else None
    px = H * W
    d_inst, d_cls = dev.empty((px,), np.int32, fill=-7), dev.empty((px,), np.int32, fill=-7)
    d_rgb = [dev.empty((px * 3,), np.uint8, fill=9) for _ in range(3)]
    d_kept = dev.empty((1,), np.int32, fill=-1)
    dev.call("mnc_render_records", d_rec, d_cnt, cap, 21, S, float(vis_thresh), float(cfg.BINARIZE_THRESH), H, W, d_img,
             float(alpha), d_inst, d_cls, d_rgb[0], d_rgb[1], d_rgb[2], d_kept)
    dev.sync()
    return (int(dev.get(d_kept, (1,), np.int32)[0]), dev.get(d_inst, (H, W), np.int32), dev.get(d_cls, (H, W), np.int32)) + \
        tuple(dev.get(p, (H, W, 3), np.uint8) for p in d_rgb)


@pytest.mark.parametrize("vis_thresh,H,W", [(0.5, 120, 200), (0.3, 375, 500)])
def test_render_records_equals_the_host_tail(vis_thresh, H, W):
    rng = np.random.default_rng(int(vis_thresh * 10))
    list_mask, list_box = RI.class_lists(rng, W, H, vis_thresh)
    scores = np.concatenate([b[:, 4] for b in list_box])
    assert (scores > vis_thresh).any() and (scores < vis_thresh).any() and (scores == np.float32(vis_thresh)).any()
    cap = 2000
    rec, total = records_from_lists(list_mask, list_box, cap, S)
    counts = [total] + [len(b) for b in list_box]
    photo = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    dev = Dev()
    try:
        got = _render_block(dev, rec, counts, cap, H, W, photo, vis_thresh)
        # the host path on what a fetch of the block gives (int32 | float32 -> float64 boxes)
        lm, lb = split_records(rec[:total], counts[1:], S)
        want = _host_tail(lm, lb, H, W, photo, vis_thresh)
        assert want[0] > 3 and got[0] == want[0]
        for g, w_ in zip(got[1:], want[1:]):
            assert g.shape == w_.shape and np.array_equal(g, w_)
        # an empty block: zero label maps, the photograph blended with black
        got0 = _render_block(dev, rec, [0] * 21, cap, H, W, photo, vis_thresh)
        want0 = _host_tail([m[:0] for m in lm], [b[:0] for b in lb], H, W, photo, vis_thresh)
        assert got0[0] == 0 and not got0[1].any() and not got0[2].any()
        for g, w_ in zip(got0[1:], want0[1:]):
            assert np.array_equal(g, w_)
    finally:
        dev.close()


def test_invalid_arguments_and_the_inverted_box():
    rng = np.random.default_rng(3)
    W, H = 80, 60
    mk = [RI._mask(rng, 1) for _ in range(3)]
    good = [np.array([5.0, 6.0, 40.0, 50.0]), np.array([20.0, 10.0, 70.0, 30.0])]
    inverted = np.array([50.0, 10.0, 10.0, 40.0])

    def call(boxes, masks, H_, W_, S_=S):
        b = np.ascontiguousarray(np.stack(boxes), np.float64)
        m = np.ascontiguousarray(np.stack(masks), np.float32).reshape(len(boxes), -1)
        c = np.arange(1, len(boxes) + 1, dtype=np.int32)
        inst, cls = np.zeros((max(H_, 1), max(W_, 1)), np.int32), np.zeros((max(H_, 1), max(W_, 1)), np.int32)
        _lib.call("mnc_render_instances", _lib.ptr(b), _lib.ptr(m), _lib.ptr(c), len(boxes), S_, 0.4, H_, W_, _lib.ptr(inst),
                  _lib.ptr(cls), 0)
        return inst, cls

    for args in (([good[0], inverted, good[1]], mk, H, W), (good, mk[:2], 1, W), (good, mk[:2], H, 1),
                 (good, [np.zeros((33, 33), np.float32)] * 2, H, W, 33)):
        with pytest.raises(_lib.MncError) as e:
            call(*args)
        assert e.value.code == 1                                              # MNC_ERR_INVALID
    # the device entry: the inverted box paints nothing but consumes its id
    rec = np.zeros((8, 6 + S * S), np.float32)
    for i, b in enumerate([good[0], inverted, good[1]]):
        rec[i, :4], rec[i, 4], rec[i, 5] = b, 0.9, i + 1
        rec[i, 6:] = mk[i].reshape(-1)
    dev = Dev()
    try:
        got = _render_block(dev, rec, [3], 8, H, W, None, 0.5)
    finally:
        dev.close()
    pred = {"boxes": good, "masks": [mk[0], mk[2]], "cls_name": [1, 3]}
    inst, cls = vis_seg._convert_pred_to_image(W, H, pred)
    assert got[0] == 3
    assert np.array_equal(got[2], cls)
    assert np.array_equal(got[1], np.where(inst == 2, 3, inst))


def _spy_render_calls(monkeypatch):
    """-> a list that receives one entry per mnc_render_records call made through _lib.call from here on."""
    calls = []
    real = _lib.call

    def spy(name, *args):
        if name == "mnc_render_records":
            calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    return calls


def _net_and_images(seed=4):
    path = models.write_mnc_5stage_test_prototxt(width_div=8)
    w = synth.synthetic_weights(path, seed=seed)
    rng = np.random.default_rng(12)
    images = [rng.integers(0, 256, ((75, 100) if k % 3 else (90, 120)) + (3,), dtype=np.uint8) for k in range(7)]
    return w, images


def _check_render(out, counts, rec, im, vis_thresh):
    lm, lb = split_records(rec, counts[1:], S)
    H, W = im.shape[:2]
    want = _host_tail(lm, lb, H, W, im, vis_thresh)
    assert out["kept"] == want[0]
    assert np.array_equal(out["inst"], want[1]) and np.array_equal(out["cls"], want[2])
    assert np.array_equal(out["inst_rgb"], want[3]) and np.array_equal(out["cls_rgb"], want[4])
    assert np.array_equal(out["overlay"], want[5])
    return want[0]


def test_native_net_render_and_the_graph_is_undisturbed():
    w, images = _net_and_images()
    ref = NativeNet(w)
    nat = NativeNet(w)
    try:
        with pytest.raises(_lib.MncError) as e:
            nat.render()
        assert e.value.code == 4                                              # MNC_ERR_STATE
        want = [ref.forward_image(im) for im in images]
        # synthetic weights give meaningless scores: a threshold that keeps some and drops some
        allscores = np.concatenate([r[:, 4] for _, r in want])
        vis_thresh = float(np.median(allscores))
        kept = []
        for k, im in enumerate(images):
            counts, rec = nat.forward_image(im)
            assert np.array_equal(counts, want[k][0]) and np.array_equal(rec, want[k][1], equal_nan=True), k
            out = nat.render(vis_thresh=vis_thresh, rgb=True)
            kept.append(_check_render(out, counts, rec, im, vis_thresh))
            # the default call shape (no RGB label images) and single outputs: NULL pointers beside non-NULL ones
            dflt = nat.render(vis_thresh=vis_thresh)
            assert sorted(dflt) == ["cls", "inst", "kept", "overlay"]
            only = nat.render(vis_thresh=vis_thresh, inst=False, overlay=False)
            assert sorted(only) == ["cls", "kept"]
            none = nat.render(vis_thresh=vis_thresh, inst=False, cls=False, overlay=False)
            assert none == {"kept": out["kept"]}
            for part in (dflt, only):
                for key in part:
                    assert np.array_equal(part[key], out[key]), key
            # launch / render / fetch: the rendering of an image in flight, and the fetch after it
            nat.launch(im)
            out2 = nat.render(vis_thresh=vis_thresh, rgb=True)
            c2, r2 = nat.fetch()
            assert np.array_equal(c2, counts) and np.array_equal(r2, rec, equal_nan=True)
            for key in out:
                assert np.array_equal(out[key], out2[key]), key
        assert max(kept) > 0
    finally:
        ref.close()
        nat.close()


def test_native_net_render_with_fewer_proposals_than_speculated():
    """pre_nms_topn = 40: fewer proposals than post_nms_topn survive, so the record block is final only after the heads' re-run on
    the exact count -- which render() makes itself when it comes before fetch(), and fetch() makes again."""
    path = models.write_mnc_5stage_test_prototxt(width_div=8)
    w = synth.synthetic_weights(path, seed=2)
    ref = NativeNet(w, use_graph=False, pre_nms_topn=40)
    nat = NativeNet(w, pre_nms_topn=40)
    try:
        rng = np.random.default_rng(8)
        for _ in range(3):
            im = rng.integers(0, 256, (75, 100, 3), dtype=np.uint8)
            counts, rec = ref.forward_image(im)
            assert ref.blob("rois").shape[0] <= 40
            vis_thresh = float(np.median(rec[:, 4])) if len(rec) else 0.5
            nat.launch(im)
            out = nat.render(vis_thresh=vis_thresh, rgb=True)
            c2, r2 = nat.fetch()
            assert np.array_equal(c2, counts) and np.array_equal(r2, rec, equal_nan=True)
            _check_render(out, counts, rec, im, vis_thresh)
    finally:
        ref.close()
        nat.close()


def test_image_stream_hands_out_each_images_own_rendering():
    w, images = _net_and_images()
    ref = NativeNet(w, use_graph=False)
    try:
        want = [ref.forward_image(im) for im in images]
    finally:
        ref.close()
    vis_thresh = float(np.median(np.concatenate([r[:, 4] for _, r in want])))
    st = ImageStream(w, in_flight=3, render=True, render_args={"vis_thresh": vis_thresh, "rgb": True})
    try:
        got = list(st.map(images))
    finally:
        st.close()
    assert len(got) == len(images)
    for k, (counts, rec, out) in enumerate(got):
        assert np.array_equal(counts, want[k][0]) and np.array_equal(rec, want[k][1], equal_nan=True)
        assert out["inst"].shape == images[k].shape[:2]
        _check_render(out, counts, rec, images[k], vis_thresh)


def test_instance_view_render_on_the_engine(monkeypatch, tmp_path):
    """InstanceView.render: from the record block gpu_mask_voting filled on the engine's net, without lists()."""
    import caffe
    import demo
    from transform.mask_transform import gpu_mask_voting
    path = models.write_mnc_5stage_test_prototxt(width_div=8)
    w = synth.synthetic_weights(path, seed=4)
    net = caffe.Net(path, w, caffe.TEST)
    try:
        im = np.random.default_rng(2).integers(0, 256, (90, 120, 3), dtype=np.uint8)
        boxes, masks, scores = demo.im_detect(im, net)
        lm, lb = gpu_mask_voting(masks, boxes, scores, 21, 100, im.shape[1], im.shape[0])
        vis_thresh = float(np.median(np.concatenate([b[:, 4] for b in lb])))
        res = boxes._net._inst.view().render(im.shape[0], im.shape[1], vis_thresh=vis_thresh, image=im)
        want = _host_tail(lm, lb, im.shape[0], im.shape[1], im, vis_thresh)
        # the record's class id is get_vis_dict's cls_ind + 1: the class image carries it
        assert res.kept == want[0] and want[0] > 0
        assert np.array_equal(res.inst, want[1]) and np.array_equal(res.cls, want[2])
        assert np.array_equal(res.inst_rgb, want[3]) and np.array_equal(res.cls_rgb, want[4])
        assert np.array_equal(res.overlay, want[5])
        # demo.main's form: _visualise with the view -- the class image comes from the RECORD's class id, which must be
        # get_vis_dict's cls_ind + 1 (checked against the host form on the fetched lists, PIL-only branch)
        from PIL import Image
        monkeypatch.setitem(sys.modules, "matplotlib", None)
        pred = demo.get_vis_dict(lb, lm, "x", demo.CLASSES, vis_thresh)
        assert len(pred["boxes"]) > 0 and set(pred["cls_name"]) <= set(range(1, 21))
        calls = _spy_render_calls(monkeypatch)
        files = {}
        for on in (False, True):
            monkeypatch.setitem(cfg.TEST, "USE_GPU_VIS", on)
            out = str(tmp_path / ("view_%d.png" % on))
            demo._visualise(im, pred, out, boxes._net._inst.view() if on else None, vis_thresh)
            files[on] = np.asarray(Image.open(out))
            assert len(calls) == int(on)
        assert np.array_equal(files[True], files[False])
    finally:
        net.close()


def test_demo_visualise_and_vis_seg_task_write_the_same_pixels(tmp_path, monkeypatch):
    import caffe
    import demo
    from PIL import Image
    from caffeWrapper.TesterWrapper import TesterWrapper
    from datasets.pascal_voc_seg import PascalVOCSeg
    monkeypatch.setitem(sys.modules, "matplotlib", None)                      # the PIL-only branch of _visualise
    case = GI.sds_case()
    pred = GI.vis_pred_dict(case, 0)
    assert set(pred["cls_name"]) <= set(range(1, 21))
    assert cfg.TEST.USE_GPU_VIS is False                                      # the switch exists and is off
    calls = _spy_render_calls(monkeypatch)
    outs = {}
    for on in (False, True):
        monkeypatch.setitem(cfg.TEST, "USE_GPU_VIS", on)
        out = str(tmp_path / ("demo_%d.png" % on))
        demo._visualise(case["images"][0]["im"], pred, out)
        outs[on] = np.asarray(Image.open(out))
        assert len(calls) == int(on)                                          # the device path was taken, once, only when on
    assert outs[True].shape == outs[False].shape and np.array_equal(outs[True], outs[False])

    class NoNet(object):
        def __init__(self, *a):
            self.name = "fake"

    monkeypatch.setattr(caffe, "Net", NoNet)
    root = str(tmp_path / "VOCdevkitSDS")
    GI.write_sds_devkit(root, case)
    decoded = {}
    for on in (False, True):
        monkeypatch.setitem(cfg.TEST, "USE_GPU_VIS", on)
        monkeypatch.setattr(cfg, "ROOT_DIR", str(tmp_path / ("root_%d" % on)))
        imdb = PascalVOCSeg("val", "2012", root, image_ext=".npy")
        t = TesterWrapper("x.prototxt", imdb, "fake.caffemodel", "vis_seg")
        with open(os.path.join(t.output_dir, "res_boxes.pkl"), "wb") as f:
            pickle.dump(case["pred_boxes"], f)
        with open(os.path.join(t.output_dir, "res_masks.pkl"), "wb") as f:
            pickle.dump(case["pred_masks"], f)
        del calls[:]
        t.get_result()
        assert len(calls) == (len(case["images"]) if on else 0)               # one device rendering per image, none when off
        decoded[on] = {(sub, rec["name"]): np.asarray(Image.open(os.path.join(t.output_dir, sub, rec["name"] + ext)))
                       for sub, ext in (("SegInst", ".jpg"), ("SegCls", ".jpg"), ("SegRes", ".png")) for rec in case["images"]}
    assert len(decoded[True]) == 3 * len(case["images"])
    for key, px in decoded[False].items():
        assert px.shape == decoded[True][key].shape and np.array_equal(px, decoded[True][key]), key
