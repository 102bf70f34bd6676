"""GPU: the convolution and InnerProduct kernels of every math mode on inputs that have exactly one right answer
(tests/exact_inputs.py: every operand representable in the form the mode feeds the matrix pipe, every partial sum a whole number
of units below 2^24).  fp32 MFMA, Winograd, split-K with slabs, the bf16x3 split, f16 and bf16 must all return the integer result,
bit for bit, in any summation order -- so every comparison here is np.array_equal on an output buffer pre-filled with NaN, and a
kernel that is wrong by one unit anywhere fails.  Launcher choices are forced through mnc_ctx_set_tuning exactly where the
tolerance tests (test_gpu_ops.py, test_gpu_conv_sw.py) force them.  tests/test_exact_inputs_host.py shows on the CPU that the method
is sound and which defects it catches that the range-relative bar does not.
The unfused F(4x4) path of the throughput plan (test_conv3x3_wino4_split, test_fc_batch) was run once on a scratch build whose
batched launch takes the first row of a block under the 304-row cut as block x 320: the three convolutions and the two products
with a second block under the cut failed (NaN from row 304 on: 65536 of 1323008 values at 76x68 64->256), this module's fused F(4x4)
and fp32 InnerProduct tests passed (the others were not run), and so did test_gpu_wino_split.py's five convolutions (at most 320 tiles, one block); of that module only the
batched launch's own test at K = 64 saw it (M = 608 and 330)."""
import numpy as np
import pytest

import exact_inputs as E
import mnc_amd
from gpu_util import Dev, from_c8, to_c8
from mnc_amd import _lib

mnc_amd.install_paths()

pytestmark = pytest.mark.gpu

LOWP_MODES = ("bf16x3", "f16", "bf16")


@pytest.fixture(scope="module")
def dev():
    d = Dev(0)
    yield d
    d.close()


@pytest.fixture
def tune(dev):
    """tune(name, value): override one of the launchers' choices on the module's context for this test."""
    keys = []

    def set_(name, value):
        keys.append(name)
        dev.tune(name, value)
    yield set_
    for k in keys:
        dev.tune(k, None)


def exact(got, want, what):
    """np.array_equal, with the differing positions in the message (they usually name the tile, lane or K range)."""
    if not E.same(got, want):
        bad = np.argwhere(~(got == want))
        pytest.fail("%s: %d of %d values differ (NaN: %d); first at %s: got %r, want %r" % (
            what, len(bad), got.size, int(np.isnan(got).sum()), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def relus(shape, shapes):
    """relu = 0 hides no negative error; relu = 1 once per entry point (the second shape of its list)."""
    return (0, 1) if shape == shapes[1] else (0,)


def words(mode, n):
    return n if mode == "bf16x3" else n // 2


# ---------------------------------------------------------------- 3x3 convolutions
def conv3x3_fp32(dev, c):
    Cin, H, W = c.a.shape
    Cout = c.w.shape[0]
    d_w = dev.empty(((Cin // 8) * Cout * 76,))
    dev.call("mnc_pack_conv3x3_weights", dev.put(c.w), d_w, Cout, Cin)
    d_y = dev.empty((Cout * H * W,), fill=np.nan)
    dev.call("mnc_conv3x3", dev.put(to_c8(c.a)), d_w, dev.put(c.b), d_y, H, W, Cin, Cout, c.relu)
    return from_c8(dev.get(d_y, (Cout * H * W,)), Cout, H, W)


@pytest.mark.parametrize("H,W,Cin,Cout", E.CONV3)
def test_conv3x3_fp32(dev, H, W, Cin, Cout):
    for family in E.families("fp32"):
        for relu in relus((H, W, Cin, Cout), E.CONV3) if family == "int" else (0,):
            c = E.conv_case(family, "fp32", H, W, Cin, Cout, relu=relu)
            exact(conv3x3_fp32(dev, c), c.want, c.what)


def _wino_run(dev, fn, c, d_x, d_w, d_b, pool):
    Cin, H, W = c.a.shape
    Cout = c.w.shape[0]
    OH, OW = ((H + 1) // 2, (W + 1) // 2) if pool else (H, W)
    d_y = dev.empty((Cout * OH * OW,), fill=np.nan)
    dev.call(fn + ("_pool" if pool else ""), d_x, d_w, d_b, d_y, H, W, Cin, Cout, c.relu)
    return from_c8(dev.get(d_y, (Cout * OH * OW,)), Cout, OH, OW)


@pytest.mark.parametrize("H,W,Cin,Cout", E.CONV3 + [E.WINO4_REDUCE])
def test_conv3x3_winograd_f2(dev, tune, H, W, Cin, Cout):
    """mnc_conv3x3_wino / _wino_pool: the default plan, forced workgroup heights and uniform K splits, the default without the tail
    plan (the settings of test_conv3x3_winograd that the product build has)."""
    for relu in relus((H, W, Cin, Cout), E.CONV3):
        c = E.wino_case(2, H, W, Cin, Cout, relu=relu)
        d_x, d_b = dev.put(to_c8(c.a)), dev.put(c.b)
        d_w = dev.empty((Cin * Cout * 17,), fill=np.nan)
        dev.call("mnc_pack_conv3x3_wino", dev.put(c.w), d_w, Cout, Cin)
        packed = dev.get(d_w, (Cin * Cout * 17,)).astype(np.float64) / c.unit
        assert np.array_equal(packed, np.round(packed)), c.what + ": the packed G g G^T is not whole"      # (a precondition)
        for rows, ks, var in ((None, None, None), ("1", "1", None), ("2", "2", None), ("4", "1", None), ("1", "4", None), (None, None, "notail")):
            if ks is not None and (Cin // 8) % int(ks):
                continue
            for k in ("WINO_ROWS", "CONV_KSPLIT", "WINO_TAIL"):
                dev.tune(k, None)
            if rows is not None:
                tune("WINO_ROWS", rows)
                tune("CONV_KSPLIT", ks)
            if var == "notail":
                tune("WINO_TAIL", "0")
            exact(_wino_run(dev, "mnc_conv3x3_wino", c, d_x, d_w, d_b, False), c.want, "%s rows=%s ks=%s %s" % (c.what, rows, ks, var))
            if rows in (None, "2") and H >= 2 and W >= 2:
                exact(_wino_run(dev, "mnc_conv3x3_wino", c, d_x, d_w, d_b, True), E.maxpool2_ceil(c.want),
                      "%s pool rows=%s ks=%s %s" % (c.what, rows, ks, var))


@pytest.mark.parametrize("H,W,Cin,Cout", E.CONV3 + [E.WINO4_REDUCE])
def test_conv3x3_winograd_f4(dev, tune, H, W, Cin, Cout):
    """mnc_conv3x3_wino4 / _wino4_pool under the plans of test_conv3x3_winograd_f4: default, forced uniform K cuts, tail plan on / off,
    both block orders, the K ranges summed in the launch and by the separate reduction kernel (FC_REDUCE=0)."""
    for relu in relus((H, W, Cin, Cout), E.CONV3):
        c = E.wino_case(4, H, W, Cin, Cout, relu=relu)
        d_x, d_b = dev.put(to_c8(c.a)), dev.put(c.b)
        d_w = dev.empty((Cin * Cout * 36,), fill=np.nan)
        dev.call("mnc_pack_conv3x3_wino4", dev.put(c.w), d_w, Cout, Cin)
        packed = dev.get(d_w, (Cin * Cout * 36,)).astype(np.float64) / c.unit
        assert np.array_equal(packed, np.round(packed)), c.what + ": the packed G g G^T is not whole"      # (a precondition)
        for ks, tail, xcd in ((None, None, None), ("1", None, None), ("2", None, "0"), ("3", None, "1"), (None, "0", None), (None, "1", None)):
            if ks is not None and int(ks) > Cin // 8:
                continue
            for k in ("CONV_KSPLIT", "WINO_TAIL", "WINO_XCD", "FC_REDUCE"):
                dev.tune(k, None)
            for k, v in (("CONV_KSPLIT", ks), ("WINO_TAIL", tail), ("WINO_XCD", xcd)):
                if v is not None:
                    tune(k, v)
            what = "%s ks=%s tail=%s xcd=%s" % (c.what, ks, tail, xcd)
            exact(_wino_run(dev, "mnc_conv3x3_wino4", c, d_x, d_w, d_b, False), c.want, what)
            if H >= 2 and W >= 2:
                exact(_wino_run(dev, "mnc_conv3x3_wino4", c, d_x, d_w, d_b, True), E.maxpool2_ceil(c.want), what + " pool")
            tune("FC_REDUCE", "0")
            exact(_wino_run(dev, "mnc_conv3x3_wino4", c, d_x, d_w, d_b, False), c.want, what + " FC_REDUCE=0")


@pytest.mark.parametrize("H,W,Cin,Cout", E.WINO4_SPLIT)
def test_conv3x3_wino4_split(dev, H, W, Cin, Cout):
    """mnc_conv3x3_wino4_split / _split_pool (input transform, the 36 positions as one batched launch of the LDS-DMA InnerProduct
    kernel, output transform) on a NaN-filled workspace of exactly mnc_conv3x3_wino4_split_ws_bytes: one row block, two and three
    blocks under the 304-row cut, two 320-row blocks; one and eight K stages; a ragged, one and several column tiles.  A row no
    block writes, a row written from the wrong tile or a position at the wrong stride is a NaN or a wrong integer."""
    lib = _lib.load()
    for relu in relus((H, W, Cin, Cout), E.WINO4_SPLIT):
        c = E.wino_case(4, H, W, Cin, Cout, relu=relu)
        mark = dev.mark()
        d_x, d_b = dev.put(to_c8(c.a)), dev.put(c.b)
        d_u = dev.empty((36 * Cout * Cin,), fill=np.nan)
        dev.call("mnc_pack_conv3x3_wino4_split", dev.put(c.w), d_u, Cout, Cin)
        packed = dev.get(d_u, (36 * Cout * Cin,)).astype(np.float64) / c.unit
        assert np.array_equal(packed, np.round(packed)), c.what + ": the packed G g G^T is not whole"      # (a precondition)
        nb = int(lib.mnc_conv3x3_wino4_split_ws_bytes(H, W, Cin, Cout))
        assert nb > 0 and nb % 4 == 0
        for pool in (False, True):
            OH, OW = ((H + 1) // 2, (W + 1) // 2) if pool else (H, W)
            d_ws = dev.empty((nb // 4,), fill=np.nan)
            d_y = dev.empty((Cout * OH * OW,), fill=np.nan)
            dev.call("mnc_conv3x3_wino4_split" + ("_pool" if pool else ""), d_x, d_u, d_b, d_y, d_ws, H, W, Cin, Cout, c.relu)
            exact(from_c8(dev.get(d_y, (Cout * OH * OW,)), Cout, OH, OW), E.maxpool2_ceil(c.want) if pool else c.want,
                  "%s split%s relu=%d" % (c.what, " pool" if pool else "", relu))
        dev.free_since(mark)


@pytest.mark.parametrize("mode", LOWP_MODES)
@pytest.mark.parametrize("H,W,Cin,Cout", E.CONV3)
def test_conv3x3_reduced_precision(dev, tune, mode, H, W, Cin, Cout):
    """mnc_conv3x3_{bf16x3,f16,bf16} on fp32 tensors under the default (CU time) and the PLAN=1 (chip-filling) plans, and the _pk
    entries on mnc_act_pack's output (fp32 output)."""
    nb = _lib.load().mnc_conv3x3_lowp_weight_bytes(E.LOWP[mode], Cout, Cin)
    assert nb > 0
    for family in E.families(mode):
        for relu in relus((H, W, Cin, Cout), E.CONV3) if family == "int" else (0,):
            c = E.conv_case(family, mode, H, W, Cin, Cout, relu=relu)
            d_w = dev.empty((nb // 4,), fill=np.nan)
            dev.call("mnc_pack_conv3x3_" + mode, dev.put(c.w), d_w, Cout, Cin)
            d_x, d_b, n_in, n_out = dev.put(to_c8(c.a)), dev.put(c.b), Cin * H * W, Cout * H * W
            d_y = dev.empty((n_out,), fill=np.nan)
            dev.call("mnc_conv3x3_" + mode, d_x, d_w, d_b, d_y, H, W, Cin, Cout, relu)
            exact(from_c8(dev.get(d_y, (n_out,)), Cout, H, W), c.want, c.what)
            tune("PLAN", "1")                        # the chip-filling plans of test_conv3x3_lowp_plan_switch
            d_y = dev.empty((n_out,), fill=np.nan)
            dev.call("mnc_conv3x3_" + mode, d_x, d_w, d_b, d_y, H, W, Cin, Cout, relu)
            dev.tune("PLAN", None)
            exact(from_c8(dev.get(d_y, (n_out,)), Cout, H, W), c.want, c.what + " PLAN=1")
            d_xp = dev.empty((words(mode, n_in),), fill=np.nan)
            dev.call("mnc_act_pack", d_x, d_xp, n_in, E.LOWP[mode])
            d_o = dev.empty((n_out,), fill=np.nan)
            dev.call("mnc_conv3x3_%s_pk" % mode, d_xp, d_w, d_b, d_o, H, W, Cin, Cout, relu, 1, 0)
            exact(from_c8(dev.get(d_o, (n_out,)), Cout, H, W), c.want, c.what + " packed input")


@pytest.mark.parametrize("mode", LOWP_MODES)
@pytest.mark.parametrize("plan", [0, 1, 2, 3])
def test_conv3x3_lowp_every_plan(dev, mode, plan):
    """mnc_conv3x3_lowp under each (row groups, channel tiles, K ranges) instantiation test_conv3x3_lowp_every_plan enumerates."""
    H, W, Cin, Cout = E.LOWP_PLAN
    m = E.LOWP[mode]
    nb = _lib.load().mnc_conv3x3_lowp_weight_bytes(m, Cout, Cin)
    for family in E.families(mode):
        for relu in (0, 1) if family == "int" else (0,):
            c = E.conv_case(family, mode, H, W, Cin, Cout, relu=relu)
            d_w = dev.empty((nb // 4,), fill=np.nan)
            dev.call("mnc_pack_conv3x3_lowp", m, dev.put(c.w), d_w, Cout, Cin)
            d_xp = dev.empty((words(mode, Cin * H * W),), fill=np.nan)
            dev.call("mnc_act_pack", dev.put(to_c8(c.a)), d_xp, Cin * H * W, m)
            d_y = dev.empty((Cout * H * W,), fill=np.nan)
            dev.tune("CONVX3_TILE", 100 + plan)
            try:
                dev.call("mnc_conv3x3_lowp", m, d_xp, d_w, dev.put(c.b), None, d_y, H, W, Cin, Cout, relu)
            finally:
                dev.tune("CONVX3_TILE", None)
            exact(from_c8(dev.get(d_y, (Cout * H * W,)), Cout, H, W), c.want, "%s plan %d" % (c.what, plan))
            if plan == 0:                            # once: the launcher's own choice under the latency plan
                d_y = dev.empty((Cout * H * W,), fill=np.nan)
                dev.tune("PLAN", 1)
                try:
                    dev.call("mnc_conv3x3_lowp", m, d_xp, d_w, dev.put(c.b), None, d_y, H, W, Cin, Cout, relu)
                finally:
                    dev.tune("PLAN", None)
                exact(from_c8(dev.get(d_y, (Cout * H * W,)), Cout, H, W), c.want, c.what + " PLAN=1")


@pytest.mark.parametrize("H,W,Cout", E.C3)
def test_conv3x3_c3(dev, tune, H, W, Cout):
    """mnc_conv3x3_c3 (3 input channels, NCHW in): the matrix-pipe kernel where the width allows it and the VALU kernel (CONV_COT=-1)."""
    for family in E.families("fp32"):
        for relu in relus((H, W, Cout), E.C3) if family == "int" else (0,):
            c = E.conv_case(family, "fp32", H, W, 3, Cout, relu=relu)
            d_x, d_w, d_b = dev.put(c.a), dev.put(c.w), dev.put(c.b)
            for cot in (None, "-1"):
                if cot:
                    tune("CONV_COT", cot)
                d_y = dev.empty((Cout * H * W,), fill=np.nan)
                dev.call("mnc_conv3x3_c3", d_x, d_w, d_b, d_y, H, W, Cout, relu)
                exact(from_c8(dev.get(d_y, (Cout * H * W,)), Cout, H, W), c.want, "%s CONV_COT=%s" % (c.what, cot))
            dev.tune("CONV_COT", None)


# ---------------------------------------------------------------- 1x1, general and stem convolutions
@pytest.mark.parametrize("H,W,Cin,Cout,stride,residual", E.C11)
def test_conv1x1(dev, tune, H, W, Cin, Cout, stride, residual):
    for family in E.families("fp32"):
        for relu in relus((H, W, Cin, Cout, stride, residual), E.C11) if family == "int" else (0,):
            c = E.conv_case(family, "fp32", H, W, Cin, Cout, K=1, stride=stride, pad=0, residual=residual and family == "int", relu=relu)
            OH, OW = c.want.shape[1:]
            d_w = dev.empty((Cin * ((Cout + 31) // 32) * 32,), fill=np.nan)
            dev.call("mnc_pack_conv1x1", dev.put(c.w), d_w, Cout, Cin, 0)
            d_x, d_b, d_r = dev.put(to_c8(c.a)), dev.put(c.b), dev.put(to_c8(c.res)) if c.res is not None else None
            for tile in (None, "4,2", "1,1", "2,1"):
                if tile:
                    tune("CONV1X1_TILE", tile)
                d_y = dev.empty((Cout * OH * OW,), fill=np.nan)
                dev.call("mnc_conv1x1", d_x, d_w, d_b, d_r, d_y, H, W, Cin, Cout, stride, relu)
                exact(from_c8(dev.get(d_y, (Cout * OH * OW,)), Cout, OH, OW), c.want, "%s tile %s" % (c.what, tile))
            dev.tune("CONV1X1_TILE", None)


@pytest.mark.parametrize("H,W,Cin,Cout,K,stride,pad,residual", E.GEN)
def test_conv2d_general(dev, tune, H, W, Cin, Cout, K, stride, pad, residual):
    """mnc_conv2d (64- and 128-channel workgroup tile) and mnc_conv2d_f16."""
    row = (H, W, Cin, Cout, K, stride, pad, residual)
    for mode in ("fp32", "f16"):
        for family in E.families(mode):
            for relu in relus(row, E.GEN) if family == "int" else (0,):
                c = E.conv_case(family, mode, H, W, Cin, Cout, K=K, stride=stride, pad=pad, residual=residual and family == "int", relu=relu)
                OH, OW = c.want.shape[1:]
                d_x, d_b, d_r = dev.put(to_c8(c.a)), dev.put(c.b), dev.put(to_c8(c.res)) if c.res is not None else None
                if mode == "fp32":
                    d_w = dev.empty((c.w.size,), fill=np.nan)
                    dev.call("mnc_pack_conv_weights", dev.put(c.w), d_w, Cout, Cin, K, K)
                    for wide in (None, "1"):
                        if wide:
                            tune("CONV2D_WIDE", wide)
                        d_y = dev.empty((Cout * OH * OW,), fill=np.nan)
                        dev.call("mnc_conv2d", d_x, d_w, d_b, d_r, d_y, H, W, Cin, Cout, K, K, stride, pad, relu)
                        exact(from_c8(dev.get(d_y, (Cout * OH * OW,)), Cout, OH, OW), c.want, "%s wide=%s" % (c.what, wide))
                    dev.tune("CONV2D_WIDE", None)
                else:
                    d_w = dev.empty((K * K * ((Cin + 31) // 32) * 32 * Cout // 2,), fill=np.nan)
                    dev.call("mnc_pack_conv_weights_f16", dev.put(c.w), d_w, Cout, Cin, K, K)
                    d_y = dev.empty((Cout * OH * OW,), fill=np.nan)
                    dev.call("mnc_conv2d_f16", d_x, d_w, d_b, d_r, d_y, H, W, Cin, Cout, K, K, stride, pad, relu)
                    exact(from_c8(dev.get(d_y, (Cout * OH * OW,)), Cout, OH, OW), c.want, c.what)


@pytest.mark.parametrize("H,W,K,stride,pad,Cout", E.STEM)
def test_conv_stem(dev, H, W, K, stride, pad, Cout):
    """mnc_conv_stem_c3 (fp32, 64 output channels) and mnc_conv_stem_f16 (the stem as a GEMM on the fp16 matrix pipe), NCHW image in."""
    for mode, co in (("fp32", 64), ("f16", Cout)):
        for family in E.families(mode):
            for relu in (0, 1) if family == "int" and K == 3 else (0,):
                c = E.conv_case(family, mode, H, W, 3, co, K=K, stride=stride, pad=pad, relu=relu)
                OH, OW = c.want.shape[1:]
                d_y = dev.empty((co * OH * OW,), fill=np.nan)
                if mode == "fp32":
                    dev.call("mnc_conv_stem_c3", dev.put(c.a), dev.put(c.w), dev.put(c.b), d_y, H, W, co, K, stride, pad, relu)
                else:
                    d_w = dev.empty(((3 * K + 1) // 2 * (co // 32) * 1024,), dtype=np.uint8, fill=0xFF)
                    dev.call("mnc_pack_conv_stem_f16", dev.put(c.w), d_w, co, K)
                    dev.call("mnc_conv_stem_f16", dev.put(c.a), d_w, dev.put(c.b), d_y, H, W, co, K, stride, pad, relu, 0)
                exact(from_c8(dev.get(d_y, (co * OH * OW,)), co, OH, OW), c.want, c.what)


# ---------------------------------------------------------------- InnerProducts
def fc_out(dev, d_o, M, N, ld, want, what):
    got = dev.get(d_o, (M, ld))
    exact(got[:, :N], want, what)
    assert np.isnan(got[:, N:]).all(), what + ": wrote beyond the column slice"


@pytest.mark.parametrize("M,N,K,pad", E.FC + E.FC_MORE)
def test_fc_fp32(dev, tune, M, N, K, pad):
    """mnc_fc: the launcher's own plan; on the shapes of the LDS-DMA kernel (and those test_fc_mfma_lds_dma forces onto it with
    FC_TILE=10) also that kernel against the register-staged one (FC_DMA=1 / 0); column slices (ldc > N)."""
    row, ld = (M, N, K, pad), N + pad
    settings = [()]
    if row in E.FC_DMA + E.FC_MORE or 2.0 * M * N * K >= 2.0e9:
        settings += [(("FC_TILE", "10"), ("FC_DMA", "1")), (("FC_TILE", "10"), ("FC_DMA", "0"))]
    for family in E.families("fp32"):
        for relu in relus(row, E.FC) if family == "int" else (0,):
            c = E.fc_case(family, "fp32", M, N, K, relu=relu)
            d_a, d_w, d_b = dev.put(c.a), dev.put(c.w), dev.put(c.b)
            for s in settings:
                for k, v in s:
                    tune(k, v)
                d_o = dev.empty((M * ld,), fill=np.nan)
                dev.call("mnc_fc", d_a, d_w, d_b, d_o, M, N, K, ld, relu)
                fc_out(dev, d_o, M, N, ld, c.want, "%s %s" % (c.what, s))
                for k, _ in s:
                    dev.tune(k, None)


@pytest.mark.parametrize("M,N,K", E.FC_BATCH)
def test_fc_batch(dev, M, N, K):
    """mnc_fc_batch (fc_mfma_dma16_kernel's BATCH mode: no bias, no activation, no K cut): B = 3 products at strides wider than the
    products, ldc = N + 8.  304 + 19 rows with three column tiles and eight K stages; 320 + 305 rows; 304 + 304 + 68 rows with a
    ragged second column tile.  The gaps between the operands hold NaN (a row or a stage read from there poisons its output); the
    gaps between the results, the columns past N and everything behind the last product still hold the fill."""
    B, ldc = 3, N + 8
    sa, sw, so = M * K + 64, N * K + 128, M * ldc + 32
    for family in E.families("fp32"):
        cs = [E.fc_case(family, "fp32", M, N, K, seed=s) for s in range(B)]
        a, w = np.full((B, sa), np.nan, np.float32), np.full((B, sw), np.nan, np.float32)
        for b, c in enumerate(cs):
            a[b, :M * K], w[b, :N * K] = c.a.reshape(-1), c.w.reshape(-1)
        mark = dev.mark()
        d_o = dev.empty((B + 1, so), fill=np.nan)
        dev.call("mnc_fc_batch", dev.put(a), sa, dev.put(w), sw, d_o, so, B, M, N, K, ldc)
        got = dev.get(d_o, (B + 1, so))
        dev.free_since(mark)
        for b, c in enumerate(cs):
            want = (c.want.astype(np.float64) - c.b.astype(np.float64)).astype(np.float32)      # (exact: multiples of the unit below 2^24)
            o = got[b, :M * ldc].reshape(M, ldc)
            exact(o[:, :N], want, "%s product %d of the batch" % (c.what, b))
            assert np.isnan(o[:, N:]).all(), c.what + ": wrote beyond the column slice"
            assert np.isnan(got[b, M * ldc:]).all(), c.what + ": wrote between the products"
        assert np.isnan(got[B]).all(), cs[0].what + ": wrote behind the last product"


@pytest.mark.parametrize("M,N,K,pad", E.FC_PAIR + E.FC_MORE[1:])
def test_fc_pair_fp32(dev, M, N, K, pad):
    """mnc_fc_pair: one launch of the LDS-DMA kernel where the plan pairs ((640, 512, 8192), (300, 1024, 4096), (300, 520, 8192)),
    two single calls elsewhere; separate output buffers with ldc = N + pad."""
    ld = N + pad
    for family in E.families("fp32"):
        for relu in (0, 1) if family == "int" and M == 300 else (0,):
            cs = [E.fc_case(family, "fp32", M, N, K, relu=relu, seed=s) for s in (0, 1)]
            d = [(dev.put(c.a), dev.put(c.w), dev.put(c.b), dev.empty((M * ld,), fill=np.nan)) for c in cs]
            dev.call("mnc_fc_pair", d[0][0], d[0][1], d[0][2], d[0][3], d[1][0], d[1][1], d[1][2], d[1][3], M, N, K, ld, relu)
            for i in (0, 1):
                fc_out(dev, d[i][3], M, N, ld, cs[i].want, "%s product %d" % (cs[i].what, i))


def lowp_weights(dev, mode, c, N, K):
    d = dev.empty(((N + 127) // 128 * 128 * K // (1 if mode == "bf16x3" else 2),), fill=np.nan)
    dev.call("mnc_pack_fc_" + mode, dev.put(c.w), d, N, K)
    return d


def lowp_panel(dev, mode, a, rows):
    """mnc_fc_pack_act of `a` into a stage-major panel of `rows` >= len(a) rows per stage (the rows past M hold other data)."""
    M, K = a.shape
    full = np.full((rows, K), 3.0, np.float32)
    full[:M] = a
    d_sm = dev.empty((rows * K // (1 if mode == "bf16x3" else 2),), fill=np.nan)
    dev.call("mnc_fc_pack_act", dev.put(full), d_sm, rows, K, {"f16": 1, "bf16x3": 0, "bf16": 2}[mode])
    return d_sm


def fc_pre(dev, mode, d_sm, mstride, d_w, d_b, d_o, M, N, K, ld, act):
    if mode == "bf16":
        dev.call("mnc_fc_bf16_ex", None, d_sm, mstride, d_w, d_b, d_o, M, N, K, ld, act, None, 0)
    else:
        dev.call("mnc_fc_%s_pre" % mode, d_sm, mstride, d_w, d_b, d_o, M, N, K, ld, act)


@pytest.mark.parametrize("mode", LOWP_MODES)
@pytest.mark.parametrize("M,N,K,pad", E.FC + E.FC_MORE + [E.FC_WIDE8, E.FC_WIDE_UNCUT])
def test_fc_reduced_precision(dev, tune, mode, M, N, K, pad):
    """mnc_fc_{bf16x3,f16,bf16}: the launcher's plan, and the 128- / 256-column kernel forced (FCX3_WIDE=0 / 1) where test_fc_bf16x3 and
    test_fc_f16 force it; the forced tile heights of the 128-column kernel (FCX3_TILE) at one shape; the _pre entries on
    mnc_fc_pack_act's panel with m_stride == M and m_stride > M."""
    row, ld = (M, N, K, pad), N + pad
    settings = [()]
    if N % 256 == 0 and N >= 512:
        settings += [(("FCX3_WIDE", "0"),), (("FCX3_WIDE", "1"),)]
    if row == E.FCX3_TILE:
        settings += [(("FCX3_TILE", v),) for v in ("5", "8", "10")]
    for family in E.families(mode, row):
        for relu in relus(row, E.FC) if family == "int" else (0,):
            c = E.fc_case(family, mode, M, N, K, relu=relu)
            d_a, d_w, d_b = dev.put(c.a), lowp_weights(dev, mode, c, N, K), dev.put(c.b)
            for s in settings:
                for k, v in s:
                    tune(k, v)
                d_o = dev.empty((M * ld,), fill=np.nan)
                dev.call("mnc_fc_" + mode, d_a, d_w, d_b, d_o, M, N, K, ld, relu)
                fc_out(dev, d_o, M, N, ld, c.want, "%s %s" % (c.what, s))
                for k, _ in s:
                    dev.tune(k, None)
            if row in E.FC_PRE:
                for rows in (M, M + 20):
                    d_o = dev.empty((M * ld,), fill=np.nan)
                    fc_pre(dev, mode, lowp_panel(dev, mode, c.a, rows), rows, d_w, d_b, d_o, M, N, K, ld, relu)
                    fc_out(dev, d_o, M, N, ld, c.want, "%s pre-packed, m_stride %d" % (c.what, rows))


PAIR_SETTINGS = (None, ("PLAN", "1"), ("FC_SPLIT_DIV", "0"))


def lowp_pair(dev, mode, d_in, mstride, d_w, d_b, M, N, K, act):
    """mnc_fc_lowp_pair as a column slice of one buffer (ldc = 2 N, product 0 in the right half); d_in[i] = ("f32" | "sm", pointer)."""
    ld = 2 * N
    d_o = dev.empty((M * ld,), fill=np.nan)
    f32 = [p if kind == "f32" else None for kind, p in d_in]
    sm = [p if kind == "sm" else None for kind, p in d_in]
    dev.call("mnc_fc_lowp_pair", E.LOWP[mode], f32[0], sm[0], f32[1], sm[1], mstride, d_w[0], d_w[1], d_b[0], d_b[1], d_o + N * 4, d_o,
             M, N, K, ld, act, None, None, 0)
    o = dev.get(d_o, (M, ld))
    return [o[:, N:], o[:, :N]]


@pytest.mark.parametrize("mode", LOWP_MODES)
@pytest.mark.parametrize("M,N,K,pad", E.FC_PAIR[:4] + E.FC_LOWP_PAIRED[1:])
def test_fc_lowp_pair(dev, tune, mode, M, N, K, pad):
    """mnc_fc_lowp_pair with both inputs fp32 and both stage-major: shapes that run as two single calls and shapes that are one
    launch (several 320-row blocks, 256-row blocks, one row block), under the default plan, PLAN=1 and FC_SPLIT_DIV=0 as
    test_fc_lowp_pair forces them: the one-row-block pair has no K ranges by default and 16 under either setting (partial sums +
    the pair reduction); PLAN=1 turns the several-row-block pairs into two singles, FC_SPLIT_DIV=0 keeps them one launch."""
    for family in E.families(mode, (M, N, K, pad)):
        for relu in (0, 1) if family == "int" and M == 640 else (0,):
            cs = [E.fc_case(family, mode, M, N, K, relu=relu, seed=s) for s in (0, 1)]
            d_w, d_b = [lowp_weights(dev, mode, c, N, K) for c in cs], [dev.put(c.b) for c in cs]
            for kind in ("f32", "sm"):
                d_in = [(kind, dev.put(c.a) if kind == "f32" else lowp_panel(dev, mode, c.a, M)) for c in cs]
                for setting in PAIR_SETTINGS:
                    if setting:
                        tune(*setting)
                    got = lowp_pair(dev, mode, d_in, M, d_w, d_b, M, N, K, relu)
                    if setting:
                        dev.tune(setting[0], None)
                    for i in (0, 1):
                        exact(got[i], cs[i].want, "%s pair, inputs %s, %s, product %d" % (cs[i].what, kind, setting, i))


@pytest.mark.parametrize("mode", LOWP_MODES)
@pytest.mark.parametrize("M,N,K,pad", E.FC_MIXED + [E.FC_LOWP_PAIRED[0], E.FC_LOWP_PAIRED[2]])
def test_fc_lowp_pair_mixed_inputs(dev, tune, mode, M, N, K, pad):
    """One product's activations as fp32 rows, the other's stage-major (either way round), with m_stride == M and with a panel
    packed for more rows than are multiplied, under the default plan, PLAN=1 and FC_SPLIT_DIV=0: the integer result -- the bits of the two single calls --, no error left behind, and a
    plain call afterwards succeeds.  (A panel of m_stride > M beside an fp32 input used to be refused AFTER the conversion kernel
    had been enqueued, at the shapes the plan pairs: the last two here.)"""
    cs = [E.fc_case("int", mode, M, N, K, seed=s) for s in (0, 1)]
    d_w, d_b = [lowp_weights(dev, mode, c, N, K) for c in cs], [dev.put(c.b) for c in cs]
    for i in (0, 1):
        d_s = dev.empty((M * N,), fill=np.nan)
        dev.call("mnc_fc_" + mode, dev.put(cs[i].a), d_w[i], d_b[i], d_s, M, N, K, N, 0)
        exact(dev.get(d_s, (M, N)), cs[i].want, cs[i].what + " single call")
    lib = _lib.load()
    for packed in (0, 1):
        for rows in (M, M + 20):
            d_in = [("sm", lowp_panel(dev, mode, c.a, rows)) if i == packed else ("f32", dev.put(c.a)) for i, c in enumerate(cs)]
            for setting in PAIR_SETTINGS:
                before = lib.mnc_last_error()
                if setting:
                    tune(*setting)
                got = lowp_pair(dev, mode, d_in, rows, d_w, d_b, M, N, K, 0)
                if setting:
                    dev.tune(setting[0], None)
                for i in (0, 1):
                    exact(got[i], cs[i].want, "%s pair, product %d stage-major with m_stride %d, %s, product %d" % (
                        cs[i].what, packed, rows, setting, i))
                dev.sync()
                assert lib.mnc_last_error() == before, lib.mnc_last_error()          # no error left behind
            d_s = dev.empty((M * N,), fill=np.nan)
            dev.call("mnc_fc_" + mode, dev.put(cs[0].a), d_w[0], d_b[0], d_s, M, N, K, N, 0)
            exact(dev.get(d_s, (M, N)), cs[0].want, cs[0].what + " plain call afterwards")
