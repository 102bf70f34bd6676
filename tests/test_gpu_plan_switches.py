"""GPU: the fallback plans of the two whole-image executors -- csrc/pipeline.hip (NativeNet) and the Python engine's plan
(mnc_amd/engine.py) -- behind their plan switches, on the reduced-width graph (width_div=8: trunk 32/32/32/64/64, rpn 64, fc 512,
mask fc 32), images 75x100 and 120x90.

    setting      native (context tuning, read at creation)   engine (environment, read when it plans)
    FUSE_SMALL   MNC_FUSE_SMALL=0                            MNC_FUSE_SMALL=0
    FUSE_POOLS   MNC_FUSE_POOLS=0                            MNC_FUSE_POOLS=0
    PACKED_ACT   MNC_PACKED_ACT=0                            MNC_F16_ACTS=0
    FC_SM        MNC_FC_SM=0                                 MNC_FC_SM=0
    ALL          the four together

Per (setting, math): the engine against the oracle (tests/test_gpu_engine.py: check_forward, its bars), the native net against the
engine bit for bit (tests/test_gpu_pipeline.py: _check_against_engine), the switch seen to act (LaunchScope labels of a profiled
image against a default net's; the engine's fused-layer lists against a default engine's), and the fallback plan against the
default plan of the native net where the launchers run the same additions in the same order.

(setting, math) pairs that are not run, with the line that makes each a no-op:
  * PACKED_ACT / fp32 -- pipeline.hip finalize(): `n->packed_trunk = conv_math(c) != 0 && tune(n->ctx, T_PACKED_ACT, 1) != 0`;
    engine.py _plan_formats(): `if self.conv_math not in _PACKED_OF or ...: return` (and _plan_fusions' `self.conv_math in _PACKED_OF`).
  * FC_SM / fp32, bf16x3, f16, mixed -- at this width no InnerProduct leaves kind 0 in any math mode: pipeline.hip prepare_fc():
    `const bool big = 2.0 * n->cfg.post_nms_topn * (double)N * (double)K >= 2.0e9` is false for all of them (the largest, fc6 /
    fc6_mask: 2 * 300 * 512 * 3136 = 9.6e8), so `fc->kind = ... : 0`, and sm_format() ends in `return 0` for kind 0 whatever
    `n->fc_sm` says; engine.py _fc_kind(): `if 2.0 * M * n_out * K < _X3_MIN_FLOPS: return "fp32"` leaves _sm_format() at 0 the same way.  The
    switch needs fc6 at >= 2 GFLOP (width_div <= 4).  test_fc_sm_is_a_no_op_at_this_width holds the claim itself: the day the bar
    moves and FC_SM starts to act here, that test fails and the four pairs belong into SETTING_MATH.  FC_SM=0 still rides along
    in ALL.

What the same width means for the comparison against the default plan: every InnerProduct of the reduced graph is below
fc_plan.h's 2 GFLOP bar (fc_small), so mnc_fc_pair's plan is `two_singles` (fc_pair_plan: `fast` needs kFcDma16) -- the paired
layers of the default plan are, here, the bits of two mnc_fc calls, and no K range is regrouped by any switch.  The whole exposed
state can therefore be held bit for bit between the plans (test_fallback_plan_equals_default_plan); at full width the InnerProduct
outputs could not."""
import numpy as np
import pytest

import mnc_amd
from mnc_amd import models, synth
from mnc_amd.native_net import NativeNet
from test_gpu_engine import check_forward
from test_gpu_pipeline import _check_against_engine

pytestmark = pytest.mark.gpu
mnc_amd.install_paths()

SWITCH_ENV = ("MNC_FUSE_SMALL", "MNC_FUSE_POOLS", "MNC_FC_SM", "MNC_PACKED_ACT", "MNC_F16_ACTS", "MNC_BRANCH_STREAMS")
SETTINGS = {
    "FUSE_SMALL": {"MNC_FUSE_SMALL": "0"},
    "FUSE_POOLS": {"MNC_FUSE_POOLS": "0"},
    "PACKED_ACT": {"MNC_PACKED_ACT": "0", "MNC_F16_ACTS": "0"},
    "FC_SM": {"MNC_FC_SM": "0"},
}
SETTINGS["ALL"] = {k: v for s in ("FUSE_SMALL", "FUSE_POOLS", "PACKED_ACT", "FC_SM") for k, v in SETTINGS[s].items()}
MATHS = ("fp32", "bf16x3", "f16", "mixed")
# (the module docstring names the pairs left out)
SETTING_MATH = ([("FUSE_SMALL", m) for m in MATHS] + [("FUSE_POOLS", m) for m in MATHS]
                + [("PACKED_ACT", m) for m in MATHS if m != "fp32"] + [("ALL", m) for m in MATHS])

BLOBS = ("conv5_3", "rpn_cls_prob_reshape", "rpn_bbox_pred", "rois", "rois_ext", "boxes", "mask_proposal", "seg_cls_prob")
_CACHE = {}


def _weights(seed=1):
    if ("w", seed) not in _CACHE:
        path = models.write_mnc_5stage_test_prototxt(width_div=8)
        _CACHE["w", seed] = (path, synth.synthetic_weights(path, seed=seed))
    return _CACHE["w", seed]


def _images():
    """Three images of one size (eager run, graph capture, replay), then one of the second size."""
    if "images" not in _CACHE:
        rng = np.random.default_rng(17)
        _CACHE["images"] = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((75, 100),) * 3 + ((120, 90),)]
    return _CACHE["images"]


def _default_plan(monkeypatch):
    for k in SWITCH_ENV:
        monkeypatch.delenv(k, raising=False)


def _apply(monkeypatch, setting):
    _default_plan(monkeypatch)
    for k, v in (SETTINGS[setting] if isinstance(setting, str) else setting).items():
        monkeypatch.setenv(k, v)


def _outputs(nat, im):
    """The exposed state of one image on a native net: the blobs of mnc_net_blob and the voted instances."""
    counts, rec = nat.forward_image(im)
    out = {n: nat.blob(n) for n in BLOBS}
    out["counts"], out["records"] = counts, rec
    return out


def _same(a, b, what):
    for n in BLOBS + ("counts", "records"):
        assert a[n].shape == b[n].shape and np.array_equal(a[n], b[n], equal_nan=(n == "records")), (what, n)


def _default_outputs(monkeypatch, math):
    """_outputs of every image of _images() on a default-plan native net (one run per math mode, shared by the tests)."""
    if ("default", math) not in _CACHE:
        _default_plan(monkeypatch)
        nat = NativeNet(_weights()[1], math=math)
        try:
            _CACHE["default", math] = [_outputs(nat, im) for im in _images()]
        finally:
            nat.close()
    return _CACHE["default", math]


def _profiled_labels(nat, im):
    """LaunchScope labels of one image with per-launch events on (which turns the graph off: direct launches)."""
    nat.profile(True)
    try:
        nat.forward_image(im)
        return [r[0] for r in nat.profile_records()]
    finally:
        nat.profile(False)


def _engine_plan(net):
    """What the engine's planner decided, as far as the switches reach: the paired InnerProducts, the one-pass box / mask
    poolings, the convolutions with a folded MAX 2x2/2, the convolutions writing packed 2-byte tensors."""
    L = net._layers
    return {"pairs": [(a.name, a.pair.name) for a in L if a.pair is not None],
            "one_pass": [(a.name, a.with_mask.name) for a in L if a.with_mask is not None],
            "conv_pool": [a.name for a in L if a.type == "Convolution" and a.fused_pool],
            "packed_out": [a.name for a in L if a.out_h]}


def _expect_native_labels(setting, math, got, dflt):
    """The labels a setting must add / remove, read off the launchers (pipeline.hip run_trunk / run_stage / run_heads_and_vote).
    Presence and absence only: an image with fewer proposals than post_nms_topn runs its heads twice (mnc_net_fetch)."""
    assert got != dflt, "%s: the profiled launches equal the default plan's -- the switch did nothing" % setting
    has, dhas = (lambda n: n in got), (lambda n: n in dflt)
    parts = ("FUSE_SMALL", "FUSE_POOLS", "PACKED_ACT") if setting == "ALL" else (setting,)
    lowp_pool = {"bf16x3": "maxpool2_c8_bf16x3", "mixed": "maxpool2_c8_bf16x3", "f16": "maxpool2_c8_f16"}.get(math)
    # the default plan, so that the assertions below are about a difference
    assert dhas("heads_finish") and dhas("rpn_heads") and dhas("box_mask_pool") and dhas("c8_to_hwc")
    for absent in ("stage_bridge", "detect_tail", "softmax_rows", "rpn_softmax", "conv1x1_to_nchw", "maxpool2_rhwc", "mask_pool_pool2"):
        assert not dhas(absent), absent
    if math != "fp32":
        assert not dhas(lowp_pool) and not dhas("maxpool2_c8")       # packed trunk, every pool folded into its convolution
    if "FUSE_SMALL" in parts:
        assert not has("heads_finish") and not has("rpn_heads")
        assert has("conv1x1_to_nchw") and has("rpn_softmax")
        assert has("softmax_rows") and has("stage_bridge") and has("detect_tail")
        # (mnc_roi_warp_sm makes its own pixel-major copy, once per stage, where the default plan makes one per image)
        assert dflt.count("c8_to_hwc") == 1 and got.count("c8_to_hwc") == 2 * got.count("stage_bridge")
        if math != "fp32" and "PACKED_ACT" not in parts:
            assert got.count(lowp_pool) == 4                             # packed trunk: convolution, then pool
    else:
        assert has("heads_finish") and has("rpn_heads") and not has("stage_bridge") and not has("detect_tail")
    if "FUSE_POOLS" in parts:
        assert not has("box_mask_pool") and has("maxpool2_rhwc") and has("mask_pool_pool2")
    else:
        assert has("box_mask_pool") and not has("maxpool2_rhwc") and not has("mask_pool_pool2")
    if "PACKED_ACT" in parts and math != "fp32":
        assert got.count("maxpool2_c8") == 4 and not has(lowp_pool)      # fp32 c8 tensors between the layers, pooled as such


def _expect_engine_plan(setting, math, got, dflt):
    assert got != dflt, "%s: the engine's plan equals the default plan -- the switch did nothing" % setting
    parts = ("FUSE_SMALL", "FUSE_POOLS", "PACKED_ACT") if setting == "ALL" else (setting,)
    trunk_pools = ["conv1_2", "conv2_2", "conv3_3", "conv4_3"]
    assert dflt["pairs"] == [("fc6", "fc6_mask"), ("fc7", "fc7_mask"), ("fc6_ext", "fc6_mask_ext"), ("fc7_ext", "fc7_mask_ext")]
    assert dflt["one_pass"] == [("roi_interpolate_conv5_box", "mask_pooling"), ("roi_interpolate_conv5_box_ext", "mask_pooling_ext")]
    assert dflt["conv_pool"] == trunk_pools and bool(dflt["packed_out"]) == (math != "fp32")
    # (without the one-pass pooling the mask branch's input does not exist when fc6 runs: no pairs either -- as in run_stage)
    assert got["pairs"] == ([] if ("FUSE_SMALL" in parts or "FUSE_POOLS" in parts) else dflt["pairs"])
    assert got["one_pass"] == ([] if "FUSE_POOLS" in parts else dflt["one_pass"])
    if "PACKED_ACT" in parts and math != "fp32":
        assert got["conv_pool"] == [] and got["packed_out"] == []
    else:
        assert got["conv_pool"] == trunk_pools and got["packed_out"] == dflt["packed_out"]


@pytest.mark.parametrize("setting,math", SETTING_MATH)
def test_fallback_plan_engine_against_oracle(setting, math, monkeypatch):
    """The Python engine under the setting, one forward on a random data / im_info as test_reduced_net_blobwise runs it, through
    the parity protocol of test_gpu_engine.check_forward: rois and rois_ext bit-exact against the reference's layers on the
    device's own inputs, every float blob within the math mode's own bar (FP32_TOL / X3_TOL / F16_TOL / MIXED_TOL).  And the
    planner followed the switch: its fused-layer lists differ from a default engine's in exactly the layers the setting names."""
    from mnc_amd.engine import Net
    path, w = _weights()
    _default_plan(monkeypatch)
    ref = Net(path, w, 1, math=math)                      # planned only, never run
    try:
        dflt = _engine_plan(ref)
    finally:
        ref.close()
    _apply(monkeypatch, setting)
    net = Net(path, w, 1, math=math)
    try:
        _expect_engine_plan(setting, math, _engine_plan(net), dflt)
        H, W = 96, 160
        data = np.random.default_rng(0).uniform(-120, 130, (1, 3, H, W)).astype(np.float32)
        im_info = np.array([[H, W, 1.0]], np.float32)
        net.forward(data=data, im_info=im_info)
        check_forward(net, w, data, im_info)
    finally:
        net.close()


@pytest.mark.parametrize("setting,math", SETTING_MATH)
def test_fallback_plan_native_equals_engine(setting, math, monkeypatch):
    """Under one setting the two executors run the same plan: the native net equals the engine bit for bit (trunk and RPN blobs,
    rois of both stages, boxes, masks, scores, voted instances; the voting against the oracle's) on three images of one size --
    eager, graph capture, replay -- and one of a second size.  Then one image with per-launch events on, against a default net
    on the same weights: the LaunchScope labels differ, in the labels the launchers of the setting's branch carry."""
    from mnc_amd.engine import Net
    path, w = _weights()
    _default_plan(monkeypatch)
    ref = NativeNet(w, math=math)                         # the context reads its tuning values here: a default plan for good
    _apply(monkeypatch, setting)
    net = Net(path, w, 1, math=math)
    nat = NativeNet(w, math=math)
    try:
        for im in _images():
            _check_against_engine(nat, net, im)
        im = _images()[0]
        _expect_native_labels(setting, math, _profiled_labels(nat, im), _profiled_labels(ref, im))
    finally:
        nat.close()
        net.close()
        ref.close()


@pytest.mark.parametrize("setting,math", [("FUSE_SMALL", m) for m in MATHS] + [("ALL", "fp32"), ("ALL", "f16")])
def test_unfused_tail_with_few_proposals(setting, math, monkeypatch):
    """FUSE_SMALL=0 with pre_nms_topn = 40: fewer proposals survive than post_nms_topn = 300, the heads are re-run on the exact
    count R, and the separate mnc_stage_bridge / detect_tail_launch (which moves the proposal count into the result block) run
    with R < post_nms_topn -- with and without the graph equal to the engine bit for bit, as the default plan is held in
    test_native_pipeline_without_graph_and_with_few_proposals."""
    from mnc_amd.engine import Net
    from mnc_config import cfg
    path, w = _weights(seed=2)
    monkeypatch.setitem(cfg.TEST, "RPN_PRE_NMS_TOP_N", 40)
    _apply(monkeypatch, setting)
    net = Net(path, w, 1, math=math)
    nat = NativeNet(w, math=math, use_graph=False, pre_nms_topn=40)
    nat_g = NativeNet(w, math=math, use_graph=True, pre_nms_topn=40)
    try:
        rng = np.random.default_rng(8)
        for _ in range(3):
            im = rng.integers(0, 256, (75, 100, 3), dtype=np.uint8)
            a = _check_against_engine(nat, net, im)
            b = _check_against_engine(nat_g, net, im)
            assert 0 < nat.blob("rois").shape[0] <= 40 and nat_g.blob("rois").shape == nat.blob("rois").shape
            assert np.array_equal(np.concatenate(a[1], 0), np.concatenate(b[1], 0))
    finally:
        nat.close()
        nat_g.close()
        net.close()


@pytest.mark.parametrize("setting,math", SETTING_MATH)
def test_fallback_plan_equals_default_plan(setting, math, monkeypatch):
    """The native net under the setting against a default-plan native net on the same weights and images: EVERY exposed blob
    (conv5_3, rpn_cls_prob_reshape, rpn_bbox_pred, rois, rois_ext, boxes, mask_proposal, seg_cls_prob) and the voted instances
    np.array_equal -- the strongest relation, and the one the launchers support at this width:
      * trunk, all settings -- PACKED_ACT=0: "Bit for bit the fp32-tensor route" (a producer's epilogue rounds as the consumer's
        staging would); FUSE_SMALL=0 in the packed trunk: convolution then pool against the pool in the convolution's epilogue,
        the rounding to the 2-byte form is monotonic and the max is taken of the same values; fp32: the same launches.
      * RPN -- FUSE_SMALL=0: mnc_conv1x1_to_nchw + mnc_rpn_softmax against mnc_rpn_heads, "the same arithmetic per channel"; rois
        are a function of these blobs alone.
      * poolings -- FUSE_POOLS=0: mnc_maxpool2_rhwc_sm + mnc_mask_pool_sm against mnc_box_mask_pool_ex, the bits
        test_per_roi_producers_write_the_fc_activation_form holds per op.
      * InnerProducts -- FUSE_SMALL=0 / FUSE_POOLS=0 un-pair fc6 + fc6_mask and fc7 + fc7_mask; a pair regroups K ranges only on
        the eight-wave kernel (>= 2 GFLOP), below it mnc_fc_pair IS two mnc_fc calls (fc_pair_plan: two_singles), and every
        InnerProduct here is below it (module docstring).  No product changes kind with a switch (all kind 0).
      * sibling classifiers -- FUSE_SMALL=0: mnc_fc's own reduction + mnc_softmax_rows_ld + mnc_stage_bridge + detect_tail_launch
        against heads_finish, "the bits of the four separate launches".
    What the fallbacks keep in buffers the default plan never writes (feat14 / box7 / mask7 in fp32, the proposal count moved by
    detect_tail_launch, the stacked rows of masks / scores / heads) is what these blobs are computed from."""
    want = _default_outputs(monkeypatch, math)
    _apply(monkeypatch, setting)
    nat = NativeNet(_weights()[1], math=math)
    try:
        for k, im in enumerate(_images()):
            _same(_outputs(nat, im), want[k], (setting, math, "image %d" % k))
    finally:
        nat.close()


def test_fc_sm_is_a_no_op_at_this_width(monkeypatch):
    """The claim the module docstring drops the four FC_SM pairs on, held by a run in the mode where FC_SM acts at full width:
    with MNC_FC_SM=0 the f16 native net launches exactly the default plan's kernels and returns its bits; the engine plans no
    stage-major second output either way.  When this fails, FC_SM has begun to act at this width: add its pairs to SETTING_MATH."""
    from mnc_amd.engine import Net
    want = _default_outputs(monkeypatch, "f16")
    path, w = _weights()
    _default_plan(monkeypatch)
    ref = NativeNet(w, math="f16")
    _apply(monkeypatch, "FC_SM")
    nat = NativeNet(w, math="f16")
    net = Net(path, w, 1, math="f16")
    try:
        im = _images()[0]
        assert _profiled_labels(nat, im) == _profiled_labels(ref, im)
        _same(_outputs(nat, im), want[0], "FC_SM")
        monkeypatch.delenv("MNC_FC_SM")
        C5, F = w["conv5_3"][0].shape[0], w["fc6"][0].shape[0]
        for blob, K, C in (("roi_interpolate_conv5", 196 * C5, C5), ("roi_interpolate_conv5_box", 49 * C5, C5),
                           ("roi_interpolate_conv5_mask", 49 * C5, C5), ("fc6", F, F), ("fc6_mask", F, F)):
            assert net._sm_format(blob, 300, K, C) == 0, blob
    finally:
        nat.close()
        net.close()
        ref.close()


@pytest.mark.parametrize("math", ["fp32", "f16"])
def test_branch_streams(math, monkeypatch):
    """BRANCH_STREAMS=1 (native only): the box branch of each head stage (mnc_maxpool2_rhwc_sm, fc6, fc7) on a second context and
    stream, forked and joined by events -- inside the captured graph too, whose branches then run in parallel.
      * FUSE_SMALL=0 with and without BRANCH_STREAMS=1 run the identical launches, only the streams differ: every exposed blob
        and the voted instances are bit-identical, without and with the graph (eager, capture, replay).  A missing fork event (the
        box branch reads feat14 too early) or join event (cls_score reads join too early) is what this catches.
      * BRANCH_STREAMS=1 alone against the default plan: the fork takes the unpaired InnerProducts where the default pairs them;
        at this width mnc_fc_pair is two mnc_fc calls (module docstring), so this too is bit-identical.
      * the second context has arenas of its own (arena_generation() sums both contexts'): nothing moves after the eager image.
    Per-launch events switch the fork off (run_stage: `ctx->profiling == 0`), so the switch's effect cannot be observed through
    profile records: there is no "the switch acted" assertion here, the bits are the test."""
    w = _weights()[1]
    images = _images()[:3]
    want = _default_outputs(monkeypatch, math)[:3]
    for base in ({"MNC_FUSE_SMALL": "0"}, {}):
        for use_graph in (False, True):
            _apply(monkeypatch, base)
            one = NativeNet(w, math=math, use_graph=use_graph)
            _apply(monkeypatch, dict(base, MNC_BRANCH_STREAMS="1"))
            two = NativeNet(w, math=math, use_graph=use_graph)
            try:
                gens = []
                for k, im in enumerate(images):
                    a, b = _outputs(one, im), _outputs(two, im)
                    _same(b, a, ("BRANCH_STREAMS", sorted(base), use_graph, "image %d" % k))
                    if not base:
                        _same(b, want[k], ("BRANCH_STREAMS against the default plan", use_graph, "image %d" % k))
                    gens.append(two.arena_generation())
                assert gens[0] == gens[1] == gens[2], gens
            finally:
                two.close()
                one.close()
