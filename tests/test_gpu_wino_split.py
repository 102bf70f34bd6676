"""GPU: the unfused F(4x4, 3x3) convolution (mnc_amd/csrc/conv_wino4_split.hip) -- input transform, the 36 transform positions as one
batched InnerProduct launch (mnc_fc_batch: fc_mfma_dma16_kernel's BATCH mode, csrc/gemm.hip), output transform -- and the switch that
moves trunk layers to it (WINO_SPLIT).

Bars: the convolutions are held to the fp32 kernels' 1e-4 of the output range (tests/test_gpu_ops.py::test_conv3x3_winograd_f4);
everything that only moves or re-orders nothing (batched against single launches, filter pack, pooled against unpooled, captured
graph against direct launches) is held to identical bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mnc_amd
from gpu_util import Dev, err, from_c8, to_c8
from mnc_amd import _lib, models, synth

mnc_amd.install_paths()

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = Dev(0)
    d.tune("WINO_SPLIT", "2")
    yield d
    d.close()


def _batch(dev, d_a, sa, d_w, sw, d_o, so, B, M, N, K, ldc):
    dev.call("mnc_fc_batch", d_a, sa, d_w, sw, d_o, so, B, M, N, K, ldc)


# (M, N): one row block with a dead last sub-tile (300 RoIs' shape); 320 rows (the issue's second case: one full 320-row block
# here, 304 + 16 under a 304-row cut); two column tiles; two row blocks of 304 (a 75 x 125 map's 608 tiles); 304 + 26 rows
@pytest.mark.parametrize("M,N", [(300, 128), (320, 128), (300, 256), (608, 128), (330, 64)])
def test_batched_innerproduct_equals_separate_calls(dev, M, N):
    """B = 3 products, K = 64, at strides wider than the products (gaps must stay untouched), against three mnc_fc calls (zero bias,
    no activation) with array_equal.
    mnc_fc runs products below its 2 GFLOP bar -- these, and every Winograd position of the trunk -- on the 64-row register-staged
    kernel, whose K order (k0, k4, k1, k5, ...) is not the LDS-DMA kernel's (k0, k4, k8, k12, k1, ...): on arbitrary values the two
    agree to rounding only (printed below: the largest difference).  So the comparison against mnc_fc uses operands whose products
    and sums are exact in fp32 (small whole numbers): every order gives the same bits, and a wrong stride, row block or column tile
    does not.  The K-order claim itself -- a batched launch returns the bits of B launches of one product each -- is held on normal
    variates against the same kernel with B = 1."""
    B, K, ldc = 3, 64, N + 8
    sa, sw, so = M * K + 64, N * K + 128, M * ldc + 32
    rng = np.random.default_rng(M * 7 + N)
    for exact in (True, False):
        if exact:
            a = rng.integers(-4, 5, (B, sa)).astype(np.float32)
            w = rng.integers(-4, 5, (B, sw)).astype(np.float32)
        else:
            a = rng.normal(0, 1, (B, sa)).astype(np.float32)
            w = rng.normal(0, 1, (B, sw)).astype(np.float32)
        mark = dev.mark()
        d_a, d_w, d_zero = dev.put(a), dev.put(w), dev.put(np.zeros(N, np.float32))
        d_o = dev.empty((B, so), fill=-7.0)
        _batch(dev, d_a, sa, d_w, sw, d_o, so, B, M, N, K, ldc)
        got = dev.get(d_o, (B, so))
        want64 = np.stack([a[b, :M * K].reshape(M, K).astype(np.float64) @ w[b, :N * K].reshape(N, K).astype(np.float64).T for b in range(B)])
        got_mn = np.stack([got[b, :M * ldc].reshape(M, ldc)[:, :N] for b in range(B)])
        assert err(got_mn, want64)[1] < 1e-5, err(got_mn, want64)
        # nothing outside the B x M x N results was written
        pad = np.stack([got[b, :M * ldc].reshape(M, ldc)[:, N:] for b in range(B)])
        assert np.all(pad == -7.0) and np.all(got[:, M * ldc:] == -7.0)
        # three mnc_fc calls
        d_s = dev.empty((B, so), fill=-7.0)
        for b in range(B):
            dev.call("mnc_fc", d_a + 4 * b * sa, d_w + 4 * b * sw, d_zero, d_s + 4 * b * so, M, N, K, ldc, 0)
        single = dev.get(d_s, (B, so))
        diff = float(np.abs(single - got).max())
        print("fc_batch M=%d N=%d %s operands: max |batched - mnc_fc| = %.3e" % (M, N, "exact" if exact else "normal", diff))
        if exact:
            assert np.array_equal(got, single)
        # three launches of the same kernel, one product each
        d_1 = dev.empty((B, so), fill=-7.0)
        for b in range(B):
            _batch(dev, d_a + 4 * b * sa, 0, d_w + 4 * b * sw, 0, d_1 + 4 * b * so, 0, 1, M, N, K, ldc)
        assert np.array_equal(got, dev.get(d_1, (B, so)))
        dev.free_since(mark)


def _conv_ref(x, w, b, relu):
    y = F.conv2d(torch.from_numpy(x)[None], torch.from_numpy(w), torch.from_numpy(b), padding=1)
    return (F.relu(y) if relu else y)[0].numpy()


def _ws(dev, H, W, Cin, Cout):
    n = int(_lib.load().mnc_conv3x3_wino4_split_ws_bytes(H, W, Cin, Cout))
    assert n >= 36 * ((H + 3) // 4) * ((W + 3) // 4) * (Cin + Cout) * 4
    return dev.empty((n // 4,), fill=np.nan)


# ragged tiles in both directions, one K stage | 304 tiles: exactly one row block | 320 tiles, two column tiles | odd H and W with
# bias + ReLU + pooling 9 x 11 -> 5 x 6 | 37 x 68: 10 x 17 = 170 tiles (the 38 x 63 maps' half-empty row block), Cout below one tile
@pytest.mark.parametrize("H,W,Cin,Cout,relu", [(7, 9, 32, 128, 0), (76, 64, 64, 64, 1), (40, 128, 64, 256, 0), (9, 11, 32, 64, 1),
                                               (37, 68, 96, 96, 1)])
def test_conv3x3_wino4_split(dev, H, W, Cin, Cout, relu):
    """mnc_conv3x3_wino4_split against torch fp32 on the CPU and against the fused mnc_conv3x3_wino4, both within 1e-4 of the output
    range; with the Pooling MAX 2x2/2 behind it exactly the ceil-mode maximum over its own unpooled outputs."""
    rng = np.random.default_rng(H * 1000 + W + Cin + Cout)
    x = rng.normal(0, 1, (Cin, H, W)).astype(np.float32)
    w = (rng.normal(0, 1, (Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = rng.normal(0, 0.1, Cout).astype(np.float32)
    want = _conv_ref(x, w, b, bool(relu))
    mark = dev.mark()
    d_x, d_b, d_raw = dev.put(to_c8(x)), dev.put(b), dev.put(w)
    d_u = dev.empty((36 * Cout * Cin,), fill=np.nan)
    dev.call("mnc_pack_conv3x3_wino4_split", d_raw, d_u, Cout, Cin)
    d_ws = _ws(dev, H, W, Cin, Cout)
    d_y = dev.empty((Cout, H, W), fill=-7.0)
    dev.call("mnc_conv3x3_wino4_split", d_x, d_u, d_b, d_y, d_ws, H, W, Cin, Cout, relu)
    got = from_c8(dev.get(d_y, (Cout * H * W,)), Cout, H, W)
    assert not np.isnan(got).any()
    d_f = dev.empty((Cin * Cout * 36,))
    dev.call("mnc_pack_conv3x3_wino4", d_raw, d_f, Cout, Cin)
    d_yf = dev.empty((Cout, H, W), fill=-7.0)
    dev.call("mnc_conv3x3_wino4", d_x, d_f, d_b, d_yf, H, W, Cin, Cout, relu)
    fused = from_c8(dev.get(d_yf, (Cout * H * W,)), Cout, H, W)
    e_ref, e_fused = err(got, want), err(got, fused)
    print("conv3x3 F(4x4) split %dx%d %d->%d relu=%d: rel err %.2e against torch, %.2e against the fused kernel (fused against torch %.2e)"
          % (H, W, Cin, Cout, relu, e_ref[1], e_fused[1], err(fused, want)[1]))
    assert e_ref[1] <= 1e-4, e_ref
    assert e_fused[1] <= 1e-4, e_fused
    OH, OW = (H + 1) // 2, (W + 1) // 2
    d_p = dev.empty((Cout, OH, OW), fill=-7.0)
    dev.call("mnc_conv3x3_wino4_split_pool", d_x, d_u, d_b, d_p, d_ws, H, W, Cin, Cout, relu)
    pooled = from_c8(dev.get(d_p, (Cout * OH * OW,)), Cout, OH, OW)
    assert np.array_equal(pooled, F.max_pool2d(torch.from_numpy(got)[None], 2, 2, ceil_mode=True)[0].numpy())
    assert err(pooled, F.max_pool2d(torch.from_numpy(want)[None], 2, 2, ceil_mode=True)[0].numpy())[1] <= 1e-4
    dev.free_since(mark)


def test_filter_pack_is_the_double_transform_rounded_once(dev):
    """U[p = 6 i + j][co][ci] = (G g G^T)[i][j] in float64, rounded to fp32 once (on whole-number 24 G, divided by 576: the fused
    kernel's pack evaluates the same way)."""
    Cout, Cin = 64, 32
    rng = np.random.default_rng(5)
    g = rng.normal(0, 1, (Cout, Cin, 3, 3)).astype(np.float32)
    G24 = np.array([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], np.float64)
    want = (np.einsum("ia,ocab,jb->ijoc", G24, g.astype(np.float64), G24) / 576.0).astype(np.float32).reshape(36, Cout, Cin)
    d_u = dev.empty((36 * Cout * Cin,), fill=np.nan)
    dev.call("mnc_pack_conv3x3_wino4_split", dev.put(g), d_u, Cout, Cin)
    assert np.array_equal(dev.get(d_u, (36, Cout, Cin)), want)


def test_selection_follows_the_tuning_value(dev):
    """WINO_SPLIT 0 / 1 / 2 as every executor of a graph asks it (mnc_conv3x3_wino4_split_selected): never; the throughput plan's
    layers and none of them under the latency plan; every supported layer."""
    sel = lambda *s: _lib.load().mnc_conv3x3_wino4_split_selected(dev.h, *s)
    try:
        assert sel(75, 125, 64, 64) == 1 and sel(75, 125, 24, 64) == 0 and sel(75, 125, 64, 48) == 0      # (2, the module's value)
        dev.tune("WINO_SPLIT", "0")
        assert sel(75, 125, 512, 512) == 0
        dev.tune("WINO_SPLIT", "1")
        assert sel(300, 500, 64, 128) == 0 and sel(38, 63, 512, 512) == 0 and sel(75, 125, 64, 64) == 0
        plan = sel(75, 125, 512, 512)
        dev.tune("PLAN", "1")
        assert sel(75, 125, 512, 512) == 0
        dev.tune("PLAN", None)
        dev.tune("WINO_SPLIT", None)
        assert sel(75, 125, 512, 512) == plan            # the default is the plan's choice
    finally:
        dev.tune("PLAN", None)
        dev.tune("WINO_SPLIT", "2")


def _engine_conv5(net, im):
    import demo
    demo.im_detect(im, net)
    return net.blobs["conv5_3"]._host_read().copy()


@pytest.mark.parametrize("value,width_div", [("2", 8), ("1", 1)])
def test_split_layers_under_a_captured_graph(monkeypatch, value, width_div):
    """One net forwards three images of one size -- direct launches, capture, replay -- and equals a net that never captures, bit
    for bit: nothing is allocated or synchronised inside the capture.  WINO_SPLIT = 2 on the reduced-width graph (every layer from 32
    input channels on runs in the split form), WINO_SPLIT = 1 at VGG-16 widths (the plan's layers).  Reduced width also: the Python
    engine follows the same switch (same bits), and the switch does something (conv5_3 differs from WINO_SPLIT = 0 in the last bits,
    within 1e-4 of its range)."""
    from mnc_amd.native_net import NativeNet
    path = models.write_mnc_5stage_test_prototxt(width_div=width_div)
    w = synth.synthetic_weights(path, seed=3)
    monkeypatch.setenv("MNC_WINO_SPLIT", value)
    ref = NativeNet(w, use_graph=False)
    nat = NativeNet(w, use_graph=True)
    nets = [ref, nat]
    try:
        rng = np.random.default_rng(11)
        size = (75, 100) if width_div > 1 else (150, 200)
        im = None
        for _ in range(3):
            im = rng.integers(0, 256, size + (3,), dtype=np.uint8)
            c0, r0 = ref.forward_image(im)
            c1, r1 = nat.forward_image(im)
            assert np.array_equal(c0, c1) and np.array_equal(r0, r1, equal_nan=True)
            assert np.array_equal(ref.blob("conv5_3"), nat.blob("conv5_3"))
        if width_div > 1:
            from mnc_amd.engine import Net
            split = nat.blob("conv5_3").copy()
            net = Net(path, w, 1)
            nets.append(net)
            _, C, h, wd = split.shape
            assert np.array_equal(from_c8(split.reshape(-1), C, h, wd)[None], _engine_conv5(net, im))
            monkeypatch.setenv("MNC_WINO_SPLIT", "0")
            fused = NativeNet(w, use_graph=False)
            nets.append(fused)
            fused.forward_image(im)
            f5 = fused.blob("conv5_3")
            assert not np.array_equal(f5, split) and err(split, f5)[1] <= 1e-4, err(split, f5)
    finally:
        for n in reversed(nets):
            n.close()
