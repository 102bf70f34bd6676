"""GPU: the e4m3 InnerProduct of the "f8" math mode (mnc_amd/csrc/gemm_f8.hip) against its statement (mnc_amd/f8.py).

  quantisers   weights and activations (from fp32 rows and from the fp16 stage-major panel), bit for bit; rows with inf / NaN included
  exact        operands with exactly one right answer (tests/f8_inputs.py): the integer product, bit for bit
  random       within the fp32 summation bound of any order (f8_inputs.sum_bound: derived, not tuned); two runs, the same bytes.
               MEASURED (MI355X), max |out - ref| / bound: scaled fp8 MFMA 0.15 at (M, N, K) = (33, 272, 512), 0.18 at (300, 441, 512),
               0.0034 at (300, 256, 4480); decoding build (K < 512) 0.004 at (33, 272, 128), 0.001 at (300, 441, 384).
               Why the short products decode their codes to fp16: v_mfma_scale_f32_32x32x64_f8f6f4 does not add its 64 products as
               an fp32 chain.  On constructed sums (one product of 2^16 beside products of 2^-(i+j)) a product 2^16 times smaller than
               the largest one of its group of 8 (or 16) consecutive K values is dropped outright, also where the large products
               cancel (the unscaled fp8 form does the same; the f16 and bf16 forms keep such a product down to 2^-22).  On the scaled
               instruction the error is up to 2^-15.8 of sum |qa||qw| (median 2^-21) whatever K is, while the bound shrinks with K:
               at K = 128 it was missed (ratio 1.17, 2 of 8976 elements), at K = 384 met at 0.29.
  refusals     K % 128 != 0, null pointers: an error, nothing launched
  net level    see the tests at the end of the file

Which case reaches which branch of the plan (fc_f8_plan.h; tests/test_f8_host.py asserts these plans on the CPU):
  mt = 2 (64-row workgroups, M <= 64)        M = 1, 33            mt = 10 (320-row blocks)               M = 300, 321 at K >= 512
  decoding build (K < 512; mt = 2, tm <= 5)  K = 128, 384         scaled MFMA, one K range, fused        K = 512
  several ranges + f8_reduce_kernel          K = 4480, PLAN=1 K = 1024
  an uneven last range                       K = 4480 (18 + 17 stages)
  a ragged last column tile                  N = 272, 441         two column tiles                       N = 272, 441
  several row blocks (tm = 2)                M = 321              the latency plan's full cut            PLAN=1, M = 33, K = 1024
"""
import numpy as np
import pytest

import f8_inputs as F
from gpu_util import Dev
from mnc_amd import _lib, f8

pytestmark = pytest.mark.gpu
I32 = np.int32


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def pack_weights(dev, w):
    """-> (device codes, device exponents, codes [N][K] uint8 as rows, exponents [N], the padded tail's codes and exponents)."""
    N, K = w.shape
    nbytes = _lib.load().mnc_pack_fc_f8_bytes(N, K)
    tiles = -(-N // 256)
    assert nbytes == tiles * 256 * K
    d_q, d_e = dev.alloc(nbytes), dev.alloc(tiles * 256 * 4)
    dev.call("mnc_pack_fc_f8", dev.put(w), d_q, d_e, N, K)
    q = dev.get(d_q, (tiles, K // 128, 256, 128), np.uint8).transpose(0, 2, 1, 3).reshape(tiles * 256, K)
    e = dev.get(d_e, (tiles * 256,), I32)
    return d_q, d_e, q[:N], e[:N], (q[N:], e[N:])


def unpack_act(dev, d_q, d_e, M, K):
    q = dev.get(d_q, (K // 128, M, 128), np.uint8).transpose(1, 0, 2).reshape(M, K)
    return q, dev.get(d_e, (M,), I32)


@pytest.mark.parametrize("N,K", [(1, 128), (1, 384), (33, 128), (33, 384), (300, 128), (300, 384), (441, 128)])
def test_weight_quantiser_is_the_statement(dev, N, K):
    mark = dev.mark()
    try:
        w = F.quantiser_rows(N, K, seed=N)
        _, _, q, e, (q_pad, e_pad) = pack_weights(dev, w)
        want_q, want_e = f8.quantise_rows(w)
        assert np.array_equal(e, want_e) and np.array_equal(q, want_q)
        assert not q_pad.any() and not e_pad.any()                      # rows past N: zero codes, exponent 0
    finally:
        dev.free_since(mark)


@pytest.mark.parametrize("M", [1, 33, 300])
@pytest.mark.parametrize("K", [128, 384])
def test_activation_quantiser_is_the_statement(dev, M, K):
    """From fp32 rows, and from the fp16 stage-major panel mnc_fc_pack_act makes, with m_stride == M and m_stride > M (the rows past
    M hold other, larger data that must not reach any row's amax)."""
    mark = dev.mark()
    try:
        x = F.quantiser_rows(M, K, seed=K + M)
        d_q, d_e = dev.alloc(M * K), dev.alloc(max(M * 4, 16))
        dev.call("mnc_fc_pack_act_f8", dev.put(x), None, 0, d_q, d_e, M, K)
        q, e = unpack_act(dev, d_q, d_e, M, K)
        want_q, want_e = f8.quantise_rows(x)
        assert np.array_equal(e, want_e) and np.array_equal(q, want_q)
        xh = F.quantiser_rows(M, K, seed=K + M + 1, fp16=True)
        want_q, want_e = f8.quantise_rows(xh)
        for stride in (M, M + 7):
            full = np.full((stride, K), 60000.0, np.float32)
            full[:M] = xh
            d_sm = dev.alloc(stride * K * 2)
            dev.call("mnc_fc_pack_act", dev.put(full), d_sm, stride, K, 1)
            dev.put_into(d_q, np.zeros(M * K, np.uint8))
            dev.call("mnc_fc_pack_act_f8", None, d_sm, stride, d_q, d_e, M, K)
            q, e = unpack_act(dev, d_q, d_e, M, K)
            assert np.array_equal(e, want_e) and np.array_equal(q, want_q), stride
    finally:
        dev.free_since(mark)


def test_non_finite_values_take_no_part_in_amax(dev):
    """The statement's rule: amax over the row's finite values; an infinity saturates at +-448, a NaN encodes as NaN (0x7F | sign), a row
    with no finite non-zero value has e = 0.  One row each, as weights, as fp32 activation rows and from the fp16 panel."""
    mark = dev.mark()
    try:
        M, K = 5, 256
        x = F.quantiser_rows(M, K, seed=3, fp16=True)
        x[0, 5], x[0, 200] = np.inf, -np.inf                           # infinities beside finite values
        x[1, 130] = np.nan                                              # a NaN beside finite values
        x[2] = 0.0
        x[2, 7], x[2, 8] = np.inf, np.nan                               # nothing finite but zeros
        x[3, K - 1] = -np.nan                                           # the sign of a NaN is kept
        want_q, want_e = f8.quantise_rows(x)
        assert want_e[2] == 0 and want_q[0, 5] == 0x7E and want_q[0, 200] == 0xFE and want_q[1, 130] == 0x7F and want_q[3, K - 1] == 0xFF
        assert want_e[0] == f8.quantise_rows(np.where(np.isfinite(x), x, 0))[1][0]
        _, _, q, e, _ = pack_weights(dev, x)
        assert np.array_equal(e, want_e) and np.array_equal(q, want_q)
        d_q, d_e = dev.alloc(M * K), dev.alloc(M * 4)
        dev.call("mnc_fc_pack_act_f8", dev.put(x), None, 0, d_q, d_e, M, K)
        q, e = unpack_act(dev, d_q, d_e, M, K)
        assert np.array_equal(e, want_e) and np.array_equal(q, want_q)
        d_sm = dev.alloc(M * K * 2)
        dev.call("mnc_fc_pack_act", dev.put(x), d_sm, M, K, 1)
        dev.call("mnc_fc_pack_act_f8", None, d_sm, M, d_q, d_e, M, K)
        q, e = unpack_act(dev, d_q, d_e, M, K)
        assert np.array_equal(e, want_e) and np.array_equal(q, want_q)
    finally:
        dev.free_since(mark)


def run_fc(dev, c_a, d_w, d_we, d_b, M, N, K, ld, act, how="rows", fill=-77.0):
    """One product through mnc_fc_f8 (how = rows), mnc_fc_f8_ex on an fp16 panel of M + 5 rows (panel; the values must be fp16
    values) or mnc_fc_pack_act_f8 + mnc_fc_f8_pre (pre) -> [M][ld] with the columns past N untouched (= fill)."""
    d_o = dev.empty((M, ld), fill=fill)
    if how == "rows":
        dev.call("mnc_fc_f8", dev.put(c_a), d_w, d_we, d_b, d_o, M, N, K, ld, act)
    elif how == "panel":
        full = np.zeros((M + 5, K), np.float32)
        full[:M] = c_a
        d_sm = dev.alloc((M + 5) * K * 2)
        dev.call("mnc_fc_pack_act", dev.put(full), d_sm, M + 5, K, 1)
        dev.call("mnc_fc_f8_ex", None, d_sm, M + 5, d_w, d_we, d_b, d_o, M, N, K, ld, act, None, 0)
    else:
        d_q, d_e = dev.alloc(M * K), dev.alloc(max(M * 4, 16))
        dev.call("mnc_fc_pack_act_f8", dev.put(c_a), None, 0, d_q, d_e, M, K)
        dev.call("mnc_fc_f8_pre", d_q, d_e, M, d_w, d_we, d_b, d_o, M, N, K, ld, act)
    got = dev.get(d_o, (M, ld))
    assert (got[:, N:] == fill).all()
    return got[:, :N]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_exact(dev, c, M, N, K, pad, hows=("rows", "panel", "pre")):
    d_w, d_we, _, ew, _ = pack_weights(dev, c.w)
    assert np.array_equal(ew, c.ew)
    d_b = dev.put(c.bias)
    want = c.want.astype(np.float32)
    for how in hows:
        for act in (0, 1, 2):
            got = run_fc(dev, c.a, d_w, d_we, d_b, M, N, K, N + pad, act, how)
            what = "M=%d N=%d K=%d ld=%d act=%d %s" % (M, N, K, N + pad, act, how)
            if act == 0:
                assert np.array_equal(bits(got), bits(want)), what
            elif act == 1:
                assert np.array_equal(bits(got), bits(np.maximum(want, 0))), what
            else:
                # the sigmoid of the exact sum: expf to 1 ulp, the addition and the division half an ulp each, and
                # d/de 1/(1+e) <= 1 in relative terms -> 2 ulp of the result, asserted as 4 ulp of 1.0 at most (results are in (0, 1))
                ref = 1.0 / (1.0 + np.exp(-c.want))
                assert np.abs(got.astype(np.float64) - ref).max() <= 4 * 2.0 ** -24, what


@pytest.mark.parametrize("M", [1, 33, 300])
@pytest.mark.parametrize("N", [256, 272, 441])
@pytest.mark.parametrize("K", [128, 384, 512])
def test_exact_arithmetic(dev, M, N, K):
    """The integer product, bit for bit: act 0 and 1 exactly; act 2 is the sigmoid of that exact value.  ldc = N and ldc > N; the
    activations as fp32 rows, as an fp16 panel with m_stride > M (the operands are fp16 values) and pre-quantised."""
    mark = dev.mark()
    try:
        c = F.exact_case(M, N, K, seed=M + N + K)
        check_exact(dev, c, M, N, K, 0, hows=("rows",))
        check_exact(dev, c, M, N, K, 3)
    finally:
        dev.free_since(mark)


def test_exact_arithmetic_identity_against_an_asymmetric_w(dev):
    """The operand-map check: one non-zero per row of A, in varying columns, picks single columns of an asymmetric W -- a swapped row /
    column index, a K value summed twice or never, or a transposed accumulator tile all change the result."""
    mark = dev.mark()
    try:
        for M, N, K in [(33, 441, 384), (300, 272, 384), (33, 441, 512), (300, 272, 512)]:
            check_exact(dev, F.exact_case(M, N, K, identity=True), M, N, K, 1, hows=("rows",))
    finally:
        dev.free_since(mark)


@pytest.mark.parametrize("M,N,K,plan", [(300, 256, 4480, None), (33, 256, 1024, 1), (321, 256, 1024, None)])
def test_exact_arithmetic_over_k_ranges(dev, M, N, K, plan):
    """Several K ranges and the reduction kernel: K = 4480 is cut into ranges of 18 and 17 stages (an uneven last range); the latency
    plan cuts K = 1024 in two at M = 33 (64-row workgroups); M = 321 is two row blocks x two ranges."""
    mark = dev.mark()
    try:
        if plan is not None:
            dev.tune("PLAN", plan)
        check_exact(dev, F.exact_case(M, N, K, seed=K, small=True), M, N, K, 2, hows=("rows", "panel"))
    finally:
        dev.tune("PLAN", None)
        dev.free_since(mark)


@pytest.mark.parametrize("M,N,K", [(300, 441, 384), (33, 272, 128), (33, 272, 512), (300, 441, 512), (300, 256, 4480)])
def test_random_data_within_the_summation_bound(dev, M, N, K):
    """|out - ref| <= 2 K 2^-24 2^(ea + ew) sum |qa||qw| + ulp(ref) per element, and two runs give the same bytes.  K = 128 and 384
    run the decoding build, K = 512 (the first K on the scaled MFMA; both tile heights) and 4480 the scaled one.  Measured on an
    MI355X, max |out - ref| / bound: (33, 272, 128) 0.004, (300, 441, 384) 0.001, (33, 272, 512) 0.15, (300, 441, 512) 0.18,
    (300, 256, 4480) 0.0034."""
    mark = dev.mark()
    try:
        a, w, b = F.random_case(M, N, K, seed=K)
        d_w, d_we, qw, ew, _ = pack_weights(dev, w)
        assert np.array_equal(qw, f8.quantise_rows(w)[0])
        d_b = dev.put(b)
        ref, bound = F.sum_bound(a, w, b, K)
        assert np.array_equal(ref, f8.fc_f8_numpy(a, w, b, 0))
        for act in (0, 1):
            got = run_fc(dev, a, d_w, d_we, d_b, M, N, K, N + 1, act)
            want = np.maximum(ref, 0) if act else ref
            d = np.abs(got.astype(np.float64) - want)
            print("M=%d N=%d K=%d act=%d: max |out - ref| / bound = %.3g" % (M, N, K, act, (d / bound).max()))
            assert (d <= bound).all()
            again = run_fc(dev, a, d_w, d_we, d_b, M, N, K, N + 1, act)
            assert np.array_equal(bits(got), bits(again))
    finally:
        dev.free_since(mark)


def test_second_output_is_the_fp16_panel_of_the_rows(dev):
    """mnc_fc_f8_ex's second output (format 1) equals mnc_fc_pack_act of the fp32 rows, from the fused epilogue (one K range) and from
    the reduction kernel (several)."""
    mark = dev.mark()
    try:
        for M, N, K in [(33, 256, 128), (300, 256, 4480)]:
            a, w, b = F.random_case(M, N, K, seed=1)
            d_w, d_we, _, _, _ = pack_weights(dev, w)
            d_o, d_sm, d_sm2 = dev.empty((M, N)), dev.alloc(M * N * 2), dev.alloc(M * N * 2)
            dev.call("mnc_fc_f8_ex", dev.put(a), None, 0, d_w, d_we, dev.put(b), d_o, M, N, K, N, 1, d_sm, 1)
            dev.call("mnc_fc_pack_act", d_o, d_sm2, M, N, 1)
            assert np.array_equal(dev.get(d_sm, (M * N,), np.uint16), dev.get(d_sm2, (M * N,), np.uint16))
    finally:
        dev.free_since(mark)


def test_refusals_launch_nothing(dev):
    mark = dev.mark()
    try:
        M, N, K = 4, 256, 128
        c = F.exact_case(M, N, K)
        d_w, d_we, _, _, _ = pack_weights(dev, c.w)
        d_a, d_b = dev.put(c.a), dev.put(c.bias)
        d_o = dev.empty((M, N), fill=5.0)
        d_q, d_e = dev.empty((M * 192,), np.uint8, fill=9), dev.empty((M,), I32, fill=9)
        bad = [("mnc_fc_f8", (d_a, d_w, d_we, d_b, d_o, M, N, 192, N, 0)),
               ("mnc_fc_f8", (d_a, d_w, d_we, d_b, d_o, M, N, 64, N, 0)),
               ("mnc_fc_f8", (None, d_w, d_we, d_b, d_o, M, N, K, N, 0)),
               ("mnc_fc_f8", (d_a, None, d_we, d_b, d_o, M, N, K, N, 0)),
               ("mnc_fc_f8", (d_a, d_w, None, d_b, d_o, M, N, K, N, 0)),
               ("mnc_fc_f8", (d_a, d_w, d_we, None, d_o, M, N, K, N, 0)),
               ("mnc_fc_f8", (d_a, d_w, d_we, d_b, None, M, N, K, N, 0)),
               ("mnc_fc_f8", (d_a, d_w, d_we, d_b, d_o, M, N, K, N - 1, 0)),
               ("mnc_fc_f8", (d_a, d_w, d_we, d_b, d_o, M, N, K, N, 3)),
               ("mnc_fc_f8_ex", (d_a, d_a, M, d_w, d_we, d_b, d_o, M, N, K, N, 0, None, 0)),
               ("mnc_fc_f8_ex", (None, None, M, d_w, d_we, d_b, d_o, M, N, K, N, 0, None, 0)),
               ("mnc_fc_f8_ex", (d_a, None, M, d_w, d_we, d_b, d_o, M, N, K, N, 0, d_o, 2)),
               ("mnc_fc_f8_pre", (None, d_e, M, d_w, d_we, d_b, d_o, M, N, K, N, 0)),
               ("mnc_fc_pack_act_f8", (d_a, None, 0, d_q, d_e, M, 192)),
               ("mnc_fc_pack_act_f8", (None, None, 0, d_q, d_e, M, K)),
               ("mnc_fc_pack_act_f8", (d_a, None, 0, None, d_e, M, K)),
               ("mnc_pack_fc_f8", (d_a, d_q, d_e, M, 192)),
               ("mnc_pack_fc_f8", (d_a, d_q, None, M, K))]
        for name, args in bad:
            with pytest.raises(_lib.MncError) as ei:
                dev.call(name, *args)
            assert ei.value.code == 1, name                              # MNC_ERR_INVALID
        dev.sync()
        assert (dev.get(d_o, (M, N)) == 5.0).all()                       # nothing was launched
        assert (dev.get(d_q, (M * 192,), np.uint8) == 9).all() and (dev.get(d_e, (M,), I32) == 9).all()
        assert _lib.load().mnc_pack_fc_f8_bytes(441, 384) == 2 * 256 * 384
    finally:
        dev.free_since(mark)


# ---- net level: full width, the `full`-style synthetic weights, 600x1000 images ------------------------------------------------
# Accuracy of the mode, recorded (MI355X; DESIGN.md, the gemm_f8.hip row of the kernel table): the distance of every head output from the fp32 oracle head on the
# device's own conv5_3 and rois (teacher-forced), as a fraction of the output's range, worst of image seeds 0, 1, 2.  The run is
# deterministic; only the seed moves the figures.  The test asserts twice the worst recorded figure: a collapse guard, no parity claim.
F8_RECORDED = {"mask_proposal": 0.141, "seg_cls_prob": 0.120, "cls_score": 0.123, "bbox_pred": 0.0831, "mask_proposal_ext": 0.146,
               "seg_cls_prob_ext": 0.140, "bbox_pred_ext": 0.0897}


@pytest.fixture(scope="module")
def vgg():
    import mnc_amd
    from mnc_amd import models, synth
    mnc_amd.install_paths()
    path = models.write_mnc_5stage_test_prototxt()
    return path, synth.synthetic_weights(path, seed=0)


def test_full_width_net_runs_the_five_large_products_as_e4m3(vgg):
    """NativeNet(math="f8") and engine.Net(math="f8") give the same bytes (blobs, rois of both stages, voted instances); the profile
    records show fc6_maskest, fc6, fc7, fc6_mask, fc7_mask of both head stages as e4m3 products (kind 4) and no fp16 InnerProduct;
    teacher-forced, fc6's and fc7_mask's blobs equal fc_f8_numpy of their own inputs (as the kernel reads them: rounded to fp16 by their
    producers) within the summation bound, on every 61st output column (68 columns; the stride is coprime to the 32-column tile)."""
    from mnc_amd.engine import Net
    from mnc_amd.native_net import NativeNet
    from test_gpu_pipeline import _check_against_engine
    path, w = vgg
    net = Net(path, w, 1, math="f8")
    nat = NativeNet(w, math="f8")
    try:
        im = np.random.default_rng(0).integers(0, 256, (600, 1000, 3), dtype=np.uint8)
        _check_against_engine(nat, net, im)
        assert nat.blob("rois").shape == (300, 5)
        cols = np.arange(0, 4096, 61)       # 61 is coprime to 32: every lane position, both 32-column halves, all four waves along N
        for layer, bottom, K in (("fc6", "roi_interpolate_conv5_box", 25088), ("fc7_mask", "fc6_mask", 4096)):
            a = net.blobs[bottom]._host_read().reshape(300, K).astype(np.float16).astype(np.float32)
            got = net.blobs[layer]._host_read().reshape(300, 4096)[:, cols].astype(np.float64)
            W, b = w[layer][0].reshape(4096, K)[cols], w[layer][1][cols]
            ref, bound = F.sum_bound(a, W, b, K)
            d = np.abs(got - np.maximum(ref, 0))
            print("%s: max |out - ref| / bound = %.3g" % (layer, (d / bound).max()))
            assert (d <= bound).all(), layer
        nat.profile(True)
        nat.forward_image(im)
        names = [r[0] for r in nat.profile_records()]
        nat.profile(False)
        assert names.count("fc_f8") == 10 and names.count("fc_f8_quantise") == 10, [n for n in names if n.startswith("fc")]
        assert not [n for n in names if n.startswith(("fc_f16", "fc_bf16"))]
    finally:
        nat.close()
        net.close()


def test_distance_from_fp32_is_recorded_and_guarded(vgg):
    from gpu_util import err, from_c8
    from mnc_amd.native_net import NativeNet
    from oracle import net as onet
    _, w = vgg
    nat = NativeNet(w, math="f8")
    K, R = 21, 300
    worst = dict.fromkeys(F8_RECORDED, 0.0)
    try:
        for seed in (0, 1, 2):
            im = np.random.default_rng(seed).integers(0, 256, (600, 1000, 3), dtype=np.uint8)
            nat.forward_image(im)
            c5 = nat.blob("conv5_3")
            _, C, h, ww = c5.shape
            c5 = from_c8(c5.reshape(-1), C, h, ww)
            rois, rois_ext, hs = nat.blob("rois"), nat.blob("rois_ext"), nat.blob("head_scores")
            masks, scores = nat.blob("mask_proposal"), nat.blob("seg_cls_prob")
            h1, h2 = onet.head(w, c5, rois, False), onet.head(w, c5, rois_ext, True)
            rep = [("mask_proposal", err(masks[:R], h1["mask_proposal"])), ("seg_cls_prob", err(scores[:R], h1["seg_cls_prob"])),
                   ("cls_score", err(hs[:R, :K], h1["cls_score"])), ("bbox_pred", err(hs[:R, 2 * K:], h1["bbox_pred"])),
                   ("mask_proposal_ext", err(masks[R:], h2["mask_proposal"])), ("seg_cls_prob_ext", err(scores[R:], h2["seg_cls_prob"])),
                   ("bbox_pred_ext", err(hs[R:, 2 * K:], h2["bbox_pred"]))]
            for name, (d, rel) in rep:
                print("seed %d f8 %-18s max|d|=%.3e rel=%.3e" % (seed, name, d, rel))
                worst[name] = max(worst[name], rel)
    finally:
        nat.close()
    print("worst:", {k: float("%.3g" % v) for k, v in worst.items()})
    for name, rel in worst.items():
        assert F8_RECORDED[name] is not None and rel <= 2 * F8_RECORDED[name], (name, rel)
