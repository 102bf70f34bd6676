"""GPU: the full-width pipeline against the oracle at the input sizes a VOC run really feeds (tests/size_sweep_inputs.py), not only at
600x1000 where the scale is 1, the resize is the identity and the trunk sees one chain of map sizes (tests/test_gpu_parity8.py).
Each size gives the 13 trunk layers other maps -- other Winograd F(4x4) launch plans (csrc/conv_wino4.hip picks unsplit / uniform K
ranges / the tail plan from how the map fills the chip), other partial 4x4 tiles and partial workgroup tiles on the right and bottom
edges --, another anchor count (down to fewer than the pre-NMS 6000, and on the 60x1000 strip fewer rois than 300), another scratch
need, and a non-unit scale in prep and in the detect tail.

  end to end   test_gpu_parity8's teacher-forced protocol per size (its tolerances, imported), the oracle side built from THIS image;
               ONE net over the whole list, three calls per size (direct launches, graph capture, graph replay: the same bits),
               then the list in reverse on the same net: bit-equal to the first pass.  The same images through ImageStream with
               three in flight, and the `mixed` mode teacher-forced (conv_sw.hip's plans are chosen by shape too).
  op level     `mnc_net_blob` shows conv5_3 only, and an edge-tile error in conv1_2 can wash out over eleven layers; so every
               distinct (H, W, Cin, Cout) the sweep's trunks launch is run through the entry the fp32 pipeline uses for that layer
               (pipeline.hip run_trunk: mnc_conv3x3_c3 for conv1_1, mnc_conv3x3_wino4_pool for conv1_2 / 2_2 / 3_3 / 4_3,
               mnc_conv3x3_wino4 otherwise), no tuning override, against an fp64 conv2d of the same fp32 operands: 1e-4 of the
               output range over the whole map AND over the first / last row and column of 4x4 tiles alone, each normalised by
               its own maximum (a strip of small wrong values hides behind a large interior value under the global metric).
               Inputs as the layer sees them: non-negative (|normal|, as after ReLU), conv1_1 pixels minus means in [-124, 152].
               F(4x4)'s input transform subtracts neighbouring values, so a positive-mean input is where its cancellation error
               is largest; tests/test_gpu_ops.py::test_conv3x3_winograd_f4 feeds zero-mean noise and quotes ~1e-5.

Figures (MI355X, profiles/size_sweep_report.txt -- every stage of every size, every op-level case):
  stages, worst over the list   fp32 8.2e-06 of the range (rpn_cls_prob_reshape at 333x500; bar 1e-4), mixed 9.6e-04 (seg_cls_prob at
                                75x500; bar 1e-3 -- the mode's fp16 InnerProducts, as at 600x1000), bf16x3 7.7e-05 (bar 3e-4).
  F(4x4) on non-negative input, worst per layer class, whole map / worst edge strip:
      conv1_2 6.3e-06 / 5.8e-06   conv2_1 5.9e-06 / 5.5e-06   conv2_2 9.5e-06 / 9.0e-06   conv3_1 8.6e-06 / 6.9e-06
      conv3_2, 3_3 1.2e-05 / 1.1e-05   conv4_1 1.2e-05 / 1.1e-05   conv4_2, 4_3 1.4e-05 / 1.3e-05   conv5_x 6.7e-06 / 5.8e-06
      (conv1_1, the direct kernel, on pixels minus means: 2.8e-07)
  The 16 cases the default (throughput) plan runs unfused (size_sweep_inputs.split_cases(): conv4_2 / conv4_3 on 361 .. 576 tiles, two
  row blocks of the batched InnerProduct launch under its 304-row cut) are run through mnc_conv3x3_wino4_split / _split_pool too,
  against the same fp64 reference: worst whole map 1.4e-05 (75x100, 75x113), worst edge strip 1.3e-05 (71x125) -- the fused kernel's.
  -- the ~1e-5 quoted for zero-mean input holds for positive-mean input at every shape of the sweep: no finding about the kernel's
  accuracy on real activations, no shape within a factor 7 of the bar.
  Run time: the module 41 s, test_gpu_parity8's fp32 case 13 s in the same run.  The op-level list and the reduced modes were cut for
  it (size_sweep_inputs.OP_LEVEL_SKIP_STAGE12; test_size_sweep_reduced_precision_modes); no entry of the end-to-end list was.
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mnc_amd
import size_sweep_inputs as S
from gpu_util import Dev, err, from_c8, to_c8
from mnc_amd import _lib, models, synth
from mnc_amd.instances import split_records
from mnc_amd.native_net import ImageStream, NativeNet
from oracle import host as ohost
from oracle import net as onet
from test_gpu_parity8 import FP32_TOL, MIXED_TOL, NUMPY_SIMD_EXP, X3_TOL, _log, oracle_for_image

pytestmark = pytest.mark.gpu
mnc_amd.install_paths()

K = 21
_oracle = {}


@pytest.fixture(scope="module")
def vgg():
    return synth.synthetic_weights(models.write_mnc_5stage_test_prototxt(), seed=0)


def _entry(w, h, ww, seed):
    """The oracle's device-independent half for one entry of the list (computed once, shared by the math modes)."""
    if (h, ww) not in _oracle:
        _oracle[(h, ww)] = oracle_for_image(w, S.image(h, ww, seed), full=False)
    return _oracle[(h, ww)]


def _teacher_forced(nat, w, o, got_m, got_b, math, tol, tag, lines):
    """test_gpu_parity8's teacher-forced checks on the blobs of the image `nat` has just run; the row count R comes from the
    oracle's ProposalLayer on the device's RPN blobs."""
    im, im_info = o["im"], o["im_info"]
    assert np.array_equal(nat.blob("data"), o["data"]), tag                                # device prep (non-unit scale), bit-exact
    c5 = nat.blob("conv5_3")
    _, C, h, ww = c5.shape
    assert (h, ww) == tuple(o["conv5_3"].shape[2:]), tag
    c5 = from_c8(c5.reshape(-1), C, h, ww)[None]
    prob, bbox = nat.blob("rpn_cls_prob_reshape"), nat.blob("rpn_bbox_pred")
    rep = [("conv5_3", err(c5, o["conv5_3"])), ("rpn_cls_prob_reshape", err(prob, o["prob"])), ("rpn_bbox_pred", err(bbox, o["bbox"]))]
    rois, rois_ext = nat.blob("rois"), nat.blob("rois_ext")
    want_rois = ohost.proposal_forward(prob, bbox, im_info)
    R = rois.shape[0]
    assert rois.shape[1] == 5 and 0 < R <= 300 and rois_ext.shape == rois.shape, tag
    if NUMPY_SIMD_EXP:
        assert rois.shape == want_rois.shape, (tag, rois.shape, want_rois.shape)
        assert np.array_equal(rois, want_rois), tag
    hs = nat.blob("head_scores")
    masks, scores = nat.blob("mask_proposal"), nat.blob("seg_cls_prob")
    assert hs.shape == (2 * R, 6 * K) and masks.shape == (2 * R, 1, 21, 21) and scores.shape == (2 * R, K), tag
    h1 = onet.head(w, c5[0], rois, False)                                                  # oracle head on the DEVICE's conv5_3 + rois
    rep += [("mask_proposal", err(masks[:R], h1["mask_proposal"])), ("seg_cls_prob", err(scores[:R], h1["seg_cls_prob"])),
            ("cls_score", err(hs[:R, :K], h1["cls_score"])), ("bbox_pred", err(hs[:R, 2 * K:], h1["bbox_pred"]))]
    want_ext = ohost.stage_bridge_forward_test(rois, np.ascontiguousarray(hs[:R, 2 * K:]), scores[:R], im_info)
    if NUMPY_SIMD_EXP:
        assert np.array_equal(rois_ext, want_ext), tag
    h2 = onet.head(w, c5[0], rois_ext, True)
    rep += [("mask_proposal_ext", err(masks[R:], h2["mask_proposal"])), ("seg_cls_prob_ext", err(scores[R:], h2["seg_cls_prob"])),
            ("bbox_pred_ext", err(hs[R:, 2 * K:], h2["bbox_pred"]))]
    boxes = nat.blob("boxes")
    ob, _, _ = ohost.im_detect_tail(rois, masks[:R], scores[:R], rois_ext, masks[R:], scores[R:], o["scale"], im.shape)
    assert np.array_equal(boxes, ob), tag                                                  # un-scaling by the real scale, clip to the original
    om, obx = ohost.gpu_mask_voting(masks, boxes, scores, K, 100, im.shape[1], im.shape[0])
    assert [len(b) for b in got_b] == [len(b) for b in obx], tag
    assert np.array_equal(np.concatenate(got_b, 0), np.concatenate(obx, 0)), tag
    assert np.array_equal(np.concatenate(got_m, 0), np.concatenate(om, 0), equal_nan=True), tag
    for name, (d, rel) in rep:
        lines.append("%-9s %-6s %-22s max|d|=%.3e rel=%.3e" % (tag, math, name, d, rel))
        assert rel < tol, lines[-1]
    return R


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def test_size_sweep_fp32_one_net_down_the_list_and_back(vgg):
    """fp32, one NativeNet for the whole list.  Per size: call 1 launches every kernel (buffers and arenas settle), call 2 captures
    the HIP graph, call 3 replays it -- the same records; the teacher-forced checks run on the replayed image's blobs.  Then the list
    in reverse (two calls per size: direct, capture) on the same net: every result bit-equal to the first pass -- nothing of the
    previous size comes through the arena or a captured graph."""
    w = vgg
    t0 = time.time()
    nat = NativeNet(w, math="fp32")
    lines, first, gens = [], {}, []
    try:
        for h, ww, seed in S.SIZES:
            o = _entry(w, h, ww, seed)
            tag = "%dx%d" % (h, ww)
            runs = [nat.forward_image(o["im"]) for _ in range(3)]
            assert _same(runs[0], runs[1]) and _same(runs[0], runs[2]), tag
            gens.append(nat.arena_generation())
            counts, rec = runs[2]
            got_m, got_b = split_records(rec, counts[1:], nat.S)
            R = _teacher_forced(nat, w, o, got_m, got_b, "fp32", FP32_TOL, tag, lines)
            H, W, scale = S.net_input(h, ww)
            assert tuple(o["data"].shape[2:]) == (H, W) and o["scale"] == scale
            if (h, ww) == S.FEW_ROIS:
                assert R < 300, "%s: the oracle keeps ~125 rois here (tests/test_size_sweep_host.py), the device returned %d" % (tag, R)
            else:
                assert R == 300, (tag, R)
            lines.append("%-9s fp32   net input %dx%d scale %.4f, %d rois, %d voted instances, arena generation %d"
                         % (tag, H, W, scale, R, int(counts[0]), gens[-1]))
            first[(h, ww)] = (runs[0], {n: nat.blob(n) for n in ("rois", "rois_ext", "boxes")})
        for h, ww, seed in reversed(S.SIZES):
            o = _entry(w, h, ww, seed)
            for k in range(2):
                again = nat.forward_image(o["im"])
                assert _same(first[(h, ww)][0], again), "%dx%d, second pass call %d" % (h, ww, k)
            for n, a in first[(h, ww)][1].items():
                assert np.array_equal(a, nat.blob(n)), (h, ww, n)
        assert gens == sorted(gens) and gens[-1] > gens[0], "this test needs a later size to move a context arena: %r" % (gens,)
        lines.append("fp32 sweep: %d sizes, both directions on one net, %.1f s wall" % (len(S.SIZES), time.time() - t0))
    finally:
        nat.close()
        print("\n".join(lines))
        _log(lines)


def test_size_sweep_through_image_stream(vgg):
    """The list down and back through ImageStream with three images in flight (voting at its default): results in submission order
    and bit-equal to one net run one image at a time without a graph."""
    w = vgg
    order = list(S.SIZES) + list(reversed(S.SIZES))
    images = [S.image(h, ww, seed) for h, ww, seed in order]
    ref = NativeNet(w, use_graph=False)
    try:
        want = [ref.forward_image(im) for im in images]
    finally:
        ref.close()
    st = ImageStream(w, in_flight=3)
    try:
        assert st.nets[0].voting == "mv"
        got = list(st.map(images))
    finally:
        st.close()
    assert len(got) == len(want)
    for (h, ww, _), a, b in zip(order, want, got):
        assert int(a[0][0]) > 0 and _same(a, b), (h, ww)


@pytest.mark.parametrize("math", ["mixed"])
def test_size_sweep_reduced_precision_modes(vgg, math):
    """`mixed` (its convolutions are bf16x3's: csrc/conv_sw.hip, plans chosen by shape) over the list, teacher-forced, with
    test_gpu_parity8's bar for it; two calls per size (direct launches, graph capture) give the same records.  A separate `bf16x3`
    pass (X3_TOL) ran once and passed -- profiles/size_sweep_report.txt -- and was left out for the module's run time: it repeats
    these convolution launches and differs in the InnerProducts only, whose shapes do not depend on the image size."""
    w = vgg
    tol = {"mixed": MIXED_TOL, "bf16x3": X3_TOL}[math]
    nat = NativeNet(w, math=math)
    lines = []
    try:
        for h, ww, seed in S.SIZES:
            o = _entry(w, h, ww, seed)
            tag = "%dx%d" % (h, ww)
            a, b = nat.forward_image(o["im"]), nat.forward_image(o["im"])
            assert _same(a, b), tag
            got_m, got_b = split_records(b[1], b[0][1:], nat.S)
            _teacher_forced(nat, w, o, got_m, got_b, math, tol, tag, lines)
    finally:
        nat.close()
        print("\n".join(lines))
        _log(lines)


def test_demo_jpegs_through_the_native_path(vgg):
    """The three real JPEGs of tests/test_gpu_demo_jpeg.py (500x357, 500x375, 333x500 after decoding) through NativeNet.detect: prep
    == the oracle's, and every blob, both roi lists and the voted instances == the Python engine's on the same decoded image (which
    that test holds to the oracle's tails)."""
    import demo
    from mnc_amd.engine import Net
    from test_gpu_demo_jpeg import _jpegs
    from test_gpu_pipeline import _check_against_engine
    w = vgg
    images = _jpegs()
    assert len(images) == 3
    net = Net(models.write_mnc_5stage_test_prototxt(), w, 1)
    nat = NativeNet(w)
    try:
        for path in images:
            im = demo._read_image_bgr(path)
            data, im_info, scale = ohost.prepare_mnc_args(im)
            assert scale != 1.0
            got_m, got_b = _check_against_engine(nat, net, im)
            assert np.array_equal(nat.blob("data"), data), path
            assert sum(len(b) for b in got_b) > 0
    finally:
        nat.close()
        net.close()


# ---- op level: the trunk shapes the sweep launches ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    d = Dev(0)
    yield d
    d.close()


@pytest.fixture
def scoped(dev):
    """Device buffers of one case are freed when it ends (a hundred cases of up to 140 MB a tensor share the module's context)."""
    n0 = len(dev._ptrs)
    yield dev
    from mnc_amd import _lib
    dev.sync()
    for p in dev._ptrs[n0:]:
        _lib.call("mnc_dev_free", dev.h, p)
    del dev._ptrs[n0:]


def _strips(H, W):
    """The first and the last row / column of 4x4 output tiles (the last ones partial when H or W is not a multiple of 4)."""
    r0, c0 = 4 * ((H - 1) // 4), 4 * ((W - 1) // 4)
    return (("first tile row", np.s_[:, :4, :]), ("first tile col", np.s_[:, :, :4]),
            ("last tile row", np.s_[:, r0:, :]), ("last tile col", np.s_[:, :, c0:]))


_CASES = S.sweep_conv_cases()
_SPLIT = S.split_cases()


@pytest.mark.parametrize("layer,kind,H,W,Cin,Cout", _CASES, ids=["%s-%dx%d" % (c[0], c[2], c[3]) for c in _CASES])
def test_trunk_conv_at_the_shapes_the_sweep_launches(scoped, layer, kind, H, W, Cin, Cout):
    dev = scoped
    rng = np.random.default_rng(H * 1000 + W + Cin + Cout)
    if kind == "c3":                   # pixels minus means, as prep hands them over: [-122.8, 152.1]
        x = (rng.integers(0, 256, (H, W, 3)).astype(np.float32) - ohost.PIXEL_MEANS).astype(np.float32).transpose(2, 0, 1).copy()
        assert x.min() >= -124 and x.max() <= 153
    else:                              # what a ReLU leaves
        x = rng.standard_normal((Cin, H, W), dtype=np.float32)
        np.abs(x, out=x)
    w = (rng.normal(0, 1, (Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = rng.normal(0, 0.1, Cout).astype(np.float32)
    tx, tw, tb = torch.from_numpy(x)[None], torch.from_numpy(w), torch.from_numpy(b)
    want = F.relu(F.conv2d(tx.double(), tw.double(), tb.double(), padding=1))[0].numpy()
    d_b = dev.put(b)
    d_y = dev.empty((Cout, H, W), fill=-7.0)
    if kind == "c3":
        dev.call("mnc_conv3x3_c3", dev.put(x), dev.put(w), d_b, d_y, H, W, Cout, 1)
    else:
        d_x = dev.put(to_c8(x))
        d_w = dev.empty((Cin * Cout * 36,), fill=np.nan)
        dev.call("mnc_pack_conv3x3_wino4", dev.put(w), d_w, Cout, Cin)
        dev.call("mnc_conv3x3_wino4", d_x, d_w, d_b, d_y, H, W, Cin, Cout, 1)
    got = from_c8(dev.get(d_y, (Cout * H * W,)), Cout, H, W)
    assert np.isfinite(got).all()
    d = np.abs(got - want)                                           # (float64)
    figs = [("whole map", float(d.max() / want.max()))] + [(n, float(d[s].max() / want[s].max())) for n, s in _strips(H, W)]
    line = "%-7s %-5s %4dx%-4d %3d->%-3d " % (layer, kind, H, W, Cin, Cout) + "  ".join("%s %.2e" % f for f in figs)
    if max(f[1] for f in figs) > 2e-5:      # the fp32 arithmetic's own share: the same convolution in plain fp32 on the CPU
        line += "  (torch fp32 on the CPU vs fp64: %.2e)" % err(F.relu(F.conv2d(tx, tw, tb, padding=1))[0].numpy(), want)[1]
    print(line)
    _log([line])
    for name, rel in figs:
        assert rel < 1e-4, (name, line)
    if kind == "pool":                 # the entry the pipeline takes for this layer: == the maximum over the un-fused kernel's outputs
        OH, OW = S.pool_out(H), S.pool_out(W)
        d_p = dev.empty((Cout, OH, OW), fill=-7.0)
        dev.call("mnc_conv3x3_wino4_pool", d_x, d_w, d_b, d_p, H, W, Cin, Cout, 1)
        pooled = from_c8(dev.get(d_p, (Cout * OH * OW,)), Cout, OH, OW)
        ref = F.max_pool2d(torch.from_numpy(got)[None], 2, 2, ceil_mode=True)[0].numpy()
        assert pooled.shape == ref.shape and np.array_equal(pooled, ref), line
    # The form the default (throughput) plan runs this layer in: transform passes around one batched InnerProduct launch
    # (csrc/conv_wino4_split.hip) exactly where the library's own rule says so on this untuned context -- and that is the list
    # size_sweep_inputs.split_cases() states from the shapes alone, so a changed rule cannot silently skip this leg.
    lib = _lib.load()
    split = bool(lib.mnc_conv3x3_wino4_split_selected(dev.h, H, W, Cin, Cout))
    assert split == ((layer, kind, H, W, Cin, Cout) in _SPLIT), line
    if not split:
        return
    d_raw = dev.put(w)
    d_u = dev.empty((36 * Cout * Cin,), fill=np.nan)
    dev.call("mnc_pack_conv3x3_wino4_split", d_raw, d_u, Cout, Cin)
    d_ws = dev.empty((int(lib.mnc_conv3x3_wino4_split_ws_bytes(H, W, Cin, Cout)) // 4,), fill=np.nan)
    d_ys = dev.empty((Cout, H, W), fill=-7.0)
    dev.call("mnc_conv3x3_wino4_split", d_x, d_u, d_b, d_ys, d_ws, H, W, Cin, Cout, 1)
    got_s = from_c8(dev.get(d_ys, (Cout * H * W,)), Cout, H, W)
    assert np.isfinite(got_s).all()
    d = np.abs(got_s - want)
    figs = [("whole map", float(d.max() / want.max()))] + [(n, float(d[s].max() / want[s].max())) for n, s in _strips(H, W)]
    line = "%-7s %-5s %4dx%-4d %3d->%-3d split: " % (layer, kind, H, W, Cin, Cout) + "  ".join("%s %.2e" % f for f in figs)
    print(line)
    _log([line])
    for name, rel in figs:
        assert rel < 1e-4, (name, line)
    if kind == "pool":
        d_ps = dev.empty((Cout, OH, OW), fill=-7.0)
        dev.call("mnc_conv3x3_wino4_split_pool", d_x, d_u, d_b, d_ps, d_ws, H, W, Cin, Cout, 1)
        pooled = from_c8(dev.get(d_ps, (Cout * OH * OW,)), Cout, OH, OW)
        ref = F.max_pool2d(torch.from_numpy(got_s)[None], 2, 2, ceil_mode=True)[0].numpy()
        assert pooled.shape == ref.shape and np.array_equal(pooled, ref), line
