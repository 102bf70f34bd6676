"""GPU: image-space mask voting (cfg.TEST.USE_GPU_MASK_MERGE = False, csrc/mv_image.hip) against outputs of the REFERENCE'S OWN
cpu_mask_voting / TesterWrapper (tests/golden/make_golden_image_voting.py -> reference_image_voting.npz), bit for bit, through
every layer: the host entry, the device entry, mask_transform.cpu_mask_voting, the tester, NativeNet and ImageStream."""
import ctypes
import os

import numpy as np
import pytest

import golden_inputs as GI
import image_voting_inputs as IV
import mnc_amd
from mnc_amd import _lib, models, synth
from mnc_amd.engine import Net, _Ctx, _DevBuf
from mnc_amd.devarray import DeviceArray
from mnc_amd.native_net import ImageStream, NativeNet
from oracle import host as ohost

pytestmark = pytest.mark.gpu
mnc_amd.install_paths()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["small", "full", "ties", "centre", "borders", "many"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(REPO, "tests", "golden", "reference_image_voting.npz"))


@pytest.fixture(scope="module")
def cases():
    return IV.voting_cases()


def _host_entry(c):
    """mnc_mask_voting_image -> (masks [R,S,S] f32, boxes [R,4] i32, scores [R] f32, class counts [20])."""
    n, S = len(c["boxes"]), c["masks"].shape[-1]
    cap = 20 * min(c["max_per_image"], n)
    om, ob = np.zeros((cap, S, S), np.float32), np.zeros((cap, 4), np.int32)
    osc, cnt, R = np.zeros(cap, np.float32), np.zeros(20, np.int32), ctypes.c_int(0)
    _lib.call("mnc_mask_voting_image", _lib.ptr(c["boxes"]), _lib.ptr(c["masks"]), _lib.ptr(c["scores"]), n, 21, S,
              c["max_per_image"], 0.3, 0.5, 0.4, c["H"], c["W"], _lib.ptr(om), _lib.ptr(ob), _lib.ptr(osc), _lib.ptr(cnt),
              ctypes.addressof(R), 0)
    R = R.value
    return om[:R], ob[:R], osc[:R], cnt


@pytest.mark.parametrize("tag", CASES)
def test_host_entry_equals_the_reference(gold, cases, tag):
    m, b, s, cnt = _host_entry(cases[tag])
    gb = gold["%s_box" % tag]
    assert np.array_equal(cnt, gold["%s_count" % tag])
    assert np.array_equal(b.astype(np.float64), gb[:, :4]) and np.array_equal(s.astype(np.float64), gb[:, 4])
    assert np.array_equal(m, gold["%s_mask" % tag][:, 0])


@pytest.mark.parametrize("tag", ["small", "ties", "centre", "many"])
def test_device_entry_records_equal_the_host_entry(cases, tag):
    c = cases[tag]
    n, S = len(c["boxes"]), 21
    ctx = _Ctx(0)
    bufs = [_DevBuf(ctx) for _ in range(5)]
    try:
        d = [bufs[i].ensure(a.nbytes) for i, a in enumerate((c["boxes"], c["masks"], c["scores"]))]
        for p, a in zip(d, (c["boxes"], c["masks"], c["scores"])):
            _lib.call("mnc_h2d", ctx.h, p, _lib.ptr(a), a.nbytes)
        cap = 20 * min(c["max_per_image"], n) + 3                       # 3 padding rows past the voting's own capacity
        D = 6 + S * S
        d_rec = bufs[3].ensure(cap * D * 4)
        d_cnt = bufs[4].ensure(21 * 4)
        _lib.call("mnc_vote_instances_ex", ctx.h, 1, d[0], d[1], d[2], n, 21, S, c["max_per_image"], 0.3, 0.5, 0.4, c["H"], c["W"],
                  d_rec, cap, d_cnt)
        rec, cnt = np.full((cap, D), 7.0, np.float32), np.zeros(21, np.int32)
        _lib.call("mnc_d2h", ctx.h, _lib.ptr(rec), d_rec, rec.nbytes)
        _lib.call("mnc_d2h", ctx.h, _lib.ptr(cnt), d_cnt, cnt.nbytes)
    finally:
        for b in bufs:
            b.release()
        ctx.close()
    m, b, s, hc = _host_entry(c)
    R = len(s)
    assert cnt[0] == R and np.array_equal(cnt[1:], hc)
    assert np.array_equal(rec[:R, :4], b.astype(np.float32)) and np.array_equal(rec[:R, 4], s)
    assert np.array_equal(rec[:R, 5], np.repeat(np.arange(1, 21), hc).astype(np.float32))
    assert np.array_equal(rec[:R, 6:], m.reshape(R, -1))
    assert not rec[R:].any()


def test_cpu_mask_voting_equals_the_reference_lists(gold, cases):
    from transform.mask_transform import cpu_mask_voting
    for tag in CASES:
        c = cases[tag]
        rb, rm = cpu_mask_voting(c["masks"], c["boxes"], c["scores"], 21, c["max_per_image"], c["W"], c["H"])
        assert len(rb) == len(rm) == 20
        assert [len(b) for b in rb] == list(gold["%s_count" % tag])
        for b, m in zip(rb, rm):
            assert b.dtype == np.float64 and m.dtype == np.float64 and b.shape[1:] == (5,) and m.shape[1:] == (1, 21, 21)
        assert np.array_equal(np.concatenate(rb, 0), gold["%s_box" % tag])
        assert np.array_equal(np.concatenate(rm, 0), gold["%s_mask" % tag].astype(np.float64))
    rb, rm = cpu_mask_voting(np.zeros((0, 1, 21, 21), np.float32), np.zeros((0, 4), np.float32), np.zeros((0, 21), np.float32),
                             21, 100, 50, 40)
    assert all(b.shape == (0, 5) for b in rb) and all(m.shape == (0, 1, 21, 21) for m in rm)


class _Blob(object):
    def __init__(self):
        self.data = np.zeros((1,), np.float32)

    def reshape(self, *dims):
        self.data = np.zeros(dims, np.float32)


class _DeviceTailNet(object):
    """The canned tester net with im_detect's tail on the device: boxes / masks / scores uploaded as DeviceArrays (what
    Net.detect_tail hands the tester), voted by Net.vote_instances on this object's own context."""
    VOTE_MODES = Net.VOTE_MODES
    vote_instances = Net.vote_instances

    def __init__(self, canned):
        self.canned, self.calls, self.name = canned, 0, "fakedev"
        self.blobs = {"data": _Blob(), "im_info": _Blob()}
        self._ctx = _Ctx(0)
        self._bufs = [_DevBuf(self._ctx) for _ in range(3)]
        self._gen = 0

    def forward(self, **kw):
        self.out = self.canned[self.calls]
        self.calls += 1
        return {}

    def detect_tail(self, scale, im_shape):
        o = self.out
        arrs = ohost.im_detect_tail(o["rois"], o["mask_proposal"], o["seg_cls_prob"], o["rois_ext"], o["mask_proposal_ext"],
                                    o["seg_cls_prob_ext"], scale, im_shape)
        self._gen += 1
        out = []
        for buf, a in zip(self._bufs, arrs):
            a = np.ascontiguousarray(a, np.float32)
            p = buf.ensure(a.nbytes)
            _lib.call("mnc_h2d", self._ctx.h, p, _lib.ptr(a), a.nbytes)
            out.append(DeviceArray(self, p, a.shape, self._bufs, (self, "_gen")))
        return tuple(out)

    def close(self):
        inst = getattr(self, "_inst", None)
        if inst is not None:
            inst.release()
        for b in self._bufs:
            b.release()
        self._ctx.close()


@pytest.mark.parametrize("device_results", [True, False])
def test_tester_without_gpu_mask_merge_equals_the_reference(gold, tmp_path, monkeypatch, device_results):
    import caffe
    from caffeWrapper.TesterWrapper import TesterWrapper
    from datasets.pascal_voc_seg import PascalVOCSeg
    from mnc_config import cfg
    case = GI.sds_case()
    root = str(tmp_path / "VOCdevkitSDS")
    GI.write_sds_devkit(root, case)
    canned = GI.tester_net_outputs(case)
    assert IV.tester_digest(canned) == str(gold["tester_digest"])

    class FakeNet(object):
        def __init__(self, *a):
            self.blobs = {k: _Blob() for k in list(canned[0]) + ["data", "im_info"]}
            self.calls, self.name = 0, "fake"

        def forward(self, **kw):
            for k, v in canned[self.calls].items():
                self.blobs[k].data = v.copy()
            self.calls += 1
            return {}

    monkeypatch.setattr(caffe, "Net", (lambda *a: _DeviceTailNet(canned)) if device_results else FakeNet)
    monkeypatch.setattr(cfg, "ROOT_DIR", str(tmp_path))
    monkeypatch.setitem(cfg.TEST, "USE_GPU_MASK_MERGE", False)
    monkeypatch.setitem(cfg.TEST, "DEVICE_RESULTS", device_results)
    imdb = PascalVOCSeg("val", "2012", root, image_ext=".npy")
    t = TesterWrapper("x.prototxt", imdb, "fake.caffemodel", "seg")
    try:
        all_boxes, all_masks = t.get_segmentation_result()
        assert t.net.calls == len(case["images"])
    finally:
        if device_results:
            t.net.close()
    n = len(case["images"])
    assert np.array_equal(np.array([[len(all_boxes[c][i]) for i in range(n)] for c in range(1, 21)]), gold["tester_counts"])
    boxes = np.concatenate([all_boxes[c][i] for c in range(1, 21) for i in range(n)], 0)
    masks = np.concatenate([all_masks[c][i] for c in range(1, 21) for i in range(n)], 0)
    assert boxes.dtype == np.float64 and np.array_equal(boxes, gold["tester_boxes"])
    assert masks.dtype == np.float64 and np.array_equal(masks.reshape(len(masks), -1).sum(1), gold["tester_mask_sums"])
    assert IV.digest(masks) == str(gold["tester_masks_digest"])


def _small_weights(seed=5):
    path = models.write_mnc_5stage_test_prototxt(width_div=8)
    return synth.synthetic_weights(path, seed=seed)


def _images():
    rng = np.random.default_rng(31)
    a1, a2 = (rng.integers(0, 256, (90, 120, 3), dtype=np.uint8) for _ in range(2))
    b = rng.integers(0, 256, (77, 130, 3), dtype=np.uint8)
    return [a1, a2, a1, b]                        # A, A (captured), A again (replayed), B


def _records_from_blobs(nat, im):
    """cpu_mask_voting on the net's own boxes / mask_proposal / seg_cls_prob, as records."""
    from transform.mask_transform import cpu_mask_voting
    boxes, masks, scores = nat.blob("boxes"), nat.blob("mask_proposal"), nat.blob("seg_cls_prob")
    rb, rm = cpu_mask_voting(masks, boxes, scores, 21, 100, im.shape[1], im.shape[0])
    cls = np.concatenate([np.full(len(b), c + 1.0) for c, b in enumerate(rb)])
    rec = np.hstack((np.concatenate(rb, 0), cls[:, None], np.concatenate(rm, 0).reshape(len(cls), -1))).astype(np.float32)
    return np.array([len(cls)] + [len(b) for b in rb], np.int32), rec


def test_native_net_image_voting_equals_cpu_mask_voting_on_its_blobs():
    w = _small_weights()
    direct = NativeNet(w, use_graph=False, voting="image")
    graph = NativeNet(w, use_graph=True, voting="image")
    try:
        assert direct.voting == graph.voting == "image"
        for k, im in enumerate(_images()):
            c0, r0 = direct.forward_image(im)
            c1, r1 = graph.forward_image(im)
            assert np.array_equal(c0, c1) and np.array_equal(r0, r1, equal_nan=True), k
            cw, rw = _records_from_blobs(direct, im)
            assert c0[0] > 0 and np.array_equal(c0, cw) and np.array_equal(r0, rw), k
    finally:
        graph.close()
        direct.close()


def test_image_stream_image_voting_equals_native_net():
    w = _small_weights()
    ref = NativeNet(w, use_graph=False, voting="image")
    st = ImageStream(w, in_flight=3, voting="image")
    try:
        assert all(n.voting == "image" for n in st.nets)
        images = _images() + _images()[:2]
        want = [ref.forward_image(im) for im in images]
        got = list(st.map(images))
        assert len(got) == len(want)
        for (c0, r0), (c1, r1) in zip(want, got):
            assert np.array_equal(c0, c1) and np.array_equal(r0, r1, equal_nan=True)
    finally:
        st.close()
        ref.close()


def test_switching_back_to_mv_equals_a_net_that_never_switched():
    w = _small_weights()
    plain = NativeNet(w)
    live = NativeNet(w)
    shared = NativeNet(live, voting="image")                # a net built from another takes its own rule
    try:
        assert live.voting == "mv" and shared.voting == "image"
        ims = _images()
        for im in ims[:2]:                                 # A twice: live's graph for A is captured under "mv"
            live.forward_image(im)
        live.set_voting("image")
        ci, ri = live.forward_image(ims[0])
        cs, rs = shared.forward_image(ims[0])
        assert np.array_equal(ci, cs) and np.array_equal(ri, rs)
        live.set_voting("mv")
        for im in ims:
            c0, r0 = plain.forward_image(im)
            c1, r1 = live.forward_image(im)
            assert np.array_equal(c0, c1) and np.array_equal(r0, r1, equal_nan=True)
    finally:
        shared.close()
        live.close()
        plain.close()
