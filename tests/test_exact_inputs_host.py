"""CPU: the exact-input method of tests/exact_inputs.py (what tests/test_gpu_exact_arithmetic.py holds the kernels to).

  * every builder's preconditions (representability, headroom) hold at every shape the GPU file uses -- the builders assert them;
  * the method is sound: a float32 numpy evaluation of each family -- operands split / rounded as the mode does, the K sum forward,
    shuffled, and cut into ranges that are summed afterwards; Winograd from the standard matrices -- gives exactly the reference;
  * the method has teeth: the same evaluation with one defect each is caught at every shape;
  * every plan of fc_plan.h is reached by one of the InnerProduct shapes (through the CPU plan shim);
  * the unfused F(4x4) path (transform passes around one batched InnerProduct launch) has the same one right answer on its cases, in
    the LDS-DMA kernel's K order and in the batched launch's row blocks, and a second block that starts at row 320 under the
    304-row cut is reported.

Defects and the existing range-relative bar (gpu_util.err(...)[1] < 1e-4), as measured here on the exact inputs (each row's test prints
its own figures; this is their summary over all rows): the bar would have passed NONE of the five defects on these inputs --
  * a dropped a_lo*b_hi term: relative error 1.1e-3 .. 3.1e-3 over 22 cases; a dropped a_hi*b_lo term: 1.3e-3 .. 1.7e-3 (22 cases);
  * one operand rounded to fp16 inside the fp32 path: 1.7e-4 .. 2.9e-4 on the 12-bit "int" inputs (48 cases), 2.4e-4 .. 2.5e-4 on the
    24-bit "impulse" inputs (39 cases) -- within a factor of 3 of the bar;
  * one tap shifted at the last column: 0.15 .. 1.4 (56 cases); one K range added twice: 0.41 .. 0.66 (144 cases).
The split inputs carry lo terms of full weight in every operand and the sums do not cancel, so a missing term is 2^-9 of the range;
on the N(0,1) inputs of the tolerance tests the same dropped term is ~1e-5 (x3_split.h) and passes.  What the exact comparison adds
is that a defect confined to ONE element, lane or K range of small values fails too: the bar divides by the tensor's maximum, the
comparison here does not divide.  All five are caught by np.array_equal at every shape."""
import numpy as np
import pytest

import exact_inputs as E
from gpu_util import err
from test_fc_plan import DMA16, FC, FC_PAIR, LOWP, LOWP_PAIR, STAGED, WIDE, X3, shim  # noqa: F401  (shim: the fixture)

LOWP_MODES = ("bf16x3", "f16", "bf16")


def conv_rows():
    """(modes, conv_case keyword arguments) of every convolution the GPU file runs outside the Winograd entries."""
    for H, W, Cin, Cout in E.CONV3 + [E.LOWP_PLAN]:
        yield E.MODES if (H, W, Cin, Cout) != E.LOWP_PLAN else LOWP_MODES, dict(H=H, W=W, Cin=Cin, Cout=Cout)
    for H, W, Cout in E.C3:
        yield ("fp32",), dict(H=H, W=W, Cin=3, Cout=Cout)
    for H, W, Cin, Cout, stride, residual in E.C11:
        yield ("fp32",), dict(H=H, W=W, Cin=Cin, Cout=Cout, K=1, stride=stride, pad=0, residual=residual)
    for H, W, Cin, Cout, K, stride, pad, residual in E.GEN:
        yield ("fp32", "f16"), dict(H=H, W=W, Cin=Cin, Cout=Cout, K=K, stride=stride, pad=pad, residual=residual)
    for H, W, K, stride, pad, Cout in E.STEM:
        yield ("fp32",), dict(H=H, W=W, Cin=3, Cout=64, K=K, stride=stride, pad=pad)
        yield ("f16",), dict(H=H, W=W, Cin=3, Cout=Cout, K=K, stride=stride, pad=pad)


def fc_rows():
    seen = []
    for row in E.FC + E.FC_MORE + E.FC_BIG + [E.FC_WIDE_UNCUT] + E.FC_PAIR + E.FC_LOWP_PAIRED + E.FC_MIXED + E.FC_PRE + [E.FCX3_TILE]:
        if row not in seen:
            seen.append(row)
            yield row


def row_cases(kind, row):
    """Every (mode, family, Case) the GPU file builds for one row (the relu = 1 variants of the "int" family too)."""
    if kind == "conv":
        modes, kw = row
        for mode in modes:
            for family in E.families(mode):
                kw2 = dict(kw, residual=kw.get("residual", False) and family == "int")
                for relu in (0, 1) if family == "int" else (0,):
                    yield mode, family, E.conv_case(family, mode, relu=relu, **kw2)
    else:
        M, N, K, pad = row
        for mode in E.MODES:
            for family in E.families(mode, row):
                for seed in (0, 1) if row in E.FC_PAIR + E.FC_LOWP_PAIRED + E.FC_MIXED and family == "int" else (0,):
                    # (relu = 1 changes the expected output only, not the inputs: the large products are built once)
                    for relu in (0, 1) if family == "int" and seed == 0 and M * N * K < 1e9 else (0,):
                        yield mode, family, E.fc_case(family, mode, M, N, K, relu=relu, seed=seed)


ROWS = [("conv", r) for r in conv_rows()] + [("fc", r) for r in fc_rows()]


def row_id(p):
    kind, row = p
    return kind + "-" + ("-".join(str(int(v)) for v in row[1].values()) + "-" + "+".join(row[0]) if kind == "conv" else "-".join(map(str, row)))


def test_the_rounding_emulation():
    """x3_split.h in numpy: nearest even and truncation to bf16, the staged split (hi truncated, lo half-up) and the packed split."""
    f = lambda *bits: np.array(bits, np.uint32).view(np.float32)
    assert np.array_equal(E.bf16_rne(f(0x3F808000, 0x3F818000, 0x3F808001, 0xBF80FFFF)).view(np.uint32), [0x3F800000, 0x3F820000, 0x3F810000, 0xBF810000])
    assert np.array_equal(E.bf16_trunc(f(0x3F80FFFF)).view(np.uint32), [0x3F800000])
    x = E._mantissa24(np.random.default_rng(0), (4096,))
    for split in (E.split_staged, E.split_rne):
        h, l = split(x)
        assert not (E._u(h) & 0xFFFF).any() and not (E._u(l) & 0xFFFF).any()
        assert np.abs(h + l - x).max() <= 2.0 ** -16 * np.abs(x).max() and (np.abs(h + l - x) <= 2.0 ** -15 * np.abs(x)).all()
    h, l = E.split_staged(x)
    assert (np.abs(h) <= np.abs(x)).all() and not np.array_equal(h, E.split_rne(x)[0])
    y = (np.arange(-65535, 65536) * 0.25).astype(np.float32)           # at most 16 significant bits: hi + lo == x in both splits
    assert np.array_equal(E.operand("bf16x3", y, "staged"), y) and np.array_equal(E.operand("bf16x3", y, "rows"), y)
    assert np.array_equal(E.operand("f16", np.float32([2047, 2049, 0.1]), "rows"), np.float32([2047, 2048, np.float16(0.1)]))


# ---- a float32 evaluation of a case as the kernels organise it: operand terms, K ranges, partial sums added afterwards ----
def matrices(c, shifted_tap=False):
    """-> A [P, K], Wm [N, K] float32 (a convolution as im2col; shifted_tap: the defect 'tap (0, 0) of the last output column reads
    its neighbour's input')."""
    if c.kind == "fc":
        return c.a, c.w
    K, stride, pad = c.geom
    Cin, H, W = c.a.shape
    OH, OW = c.want.shape[1:]
    xp = np.zeros((Cin, H + 2 * pad, W + 2 * pad), np.float32)
    xp[:, pad:pad + H, pad:pad + W] = c.a
    cols = np.empty((Cin, K, K, OH, OW), np.float32)
    for ky in range(K):
        for kx in range(K):
            cols[:, ky, kx] = xp[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride]
    if shifted_tap:
        cols[:, 0, 0, :, -1] = cols[:, 0, 0, :, -2]
    return np.ascontiguousarray(cols.reshape(Cin * K * K, OH * OW).T), c.w.reshape(c.w.shape[0], -1)


def orders(K, rng):
    return {"forward": [np.arange(K)], "shuffled": [rng.permutation(K)], "ranges": np.array_split(np.arange(K), 4 if K >= 4 else 1)}


def eval32(c, mode, order, defect=None):
    A, Wm = matrices(c, shifted_tap=defect == "tap")
    (ah, al), (wh, wl) = E.terms(mode, A, "staged" if c.kind == "conv" else "rows"), E.terms(mode, Wm, "weight")
    if defect == "f16":                                   # one operand through a 2-byte staging path
        ah = ah.astype(np.float16).astype(np.float32)
    if defect == "twice":
        order = list(order) + [order[len(order) // 2]]
    y = None
    for idx in order:
        part = np.matmul(ah[:, idx], wh[:, idx].T)
        if al is not None and defect != "a_lo":
            part = part + np.matmul(al[:, idx], wh[:, idx].T)
        if wl is not None and defect != "b_lo":
            part = part + np.matmul(ah[:, idx], wl[:, idx].T)
        y = part if y is None else y + part
    y = y + c.b
    if c.kind == "conv":
        y = np.ascontiguousarray(y.T).reshape(c.want.shape)
        if c.res is not None:
            y = y + c.res
    return np.maximum(y, 0) if c.relu else y


def test_winograd_in_float32_gives_the_reference_in_any_order():
    rng = np.random.default_rng(2)
    for m in (2, 4):
        for shape in E.CONV3 + [E.WINO4_REDUCE]:
            c = E.wino_case(m, *shape)
            assert c.bits > 0 and E.wino_case(m, *shape, relu=1).bits > 0, c.what
            print(c.what)
            Cin = shape[2]
            for name, order in orders(Cin, rng).items():
                got = E.wino_f32(c.a, c.w, m, order) + c.b[:, None, None]
                assert got.dtype == np.float32 and E.same(got, c.want), (c.what, name)
            # teeth: one channel range added twice
            twice = list(orders(Cin, rng)["ranges"])
            twice.append(twice[len(twice) // 2])
            assert not E.same(E.wino_f32(c.a, c.w, m, twice) + c.b[:, None, None], c.want), c.what


def test_the_dma_kernels_k_order_and_the_batched_launchs_row_blocks():
    assert E.dma_k_order(64)[:9].tolist() == [0, 4, 8, 12, 1, 5, 9, 13, 2] and E.dma_k_order(64)[16:20].tolist() == [16, 20, 24, 28]
    assert sorted(E.dma_k_order(256).tolist()) == list(range(256))
    # the tile counts E.WINO4_SPLIT and E.FC_BATCH are chosen for
    assert E.batch_row_blocks(63) == [(0, 63)] and E.batch_row_blocks(304) == [(0, 304)] and E.batch_row_blocks(320) == [(0, 320)]
    assert E.batch_row_blocks(323) == [(0, 304), (304, 19)] and E.batch_row_blocks(608) == [(0, 304), (304, 304)]
    assert E.batch_row_blocks(625) == [(0, 320), (320, 305)] and E.batch_row_blocks(676) == [(0, 304), (304, 304), (608, 68)]
    assert E.batch_row_blocks(323, first=320) == [(0, 304), (320, 3)]
    tiles = [-(-H // 4) * -(-W // 4) for H, W, _, _ in E.WINO4_SPLIT]
    assert tiles == [6, 323, 323, 625, 676] and sorted(set(tiles[1:])) == [M for M, _, _ in E.FC_BATCH]


@pytest.mark.parametrize("H,W,Cin,Cout", E.WINO4_SPLIT)
def test_split_winograd_in_float32_gives_the_reference(H, W, Cin, Cout):
    """The cases of test_gpu_exact_arithmetic.py::test_conv3x3_wino4_split have one right answer for the unfused decomposition too
    (V and M through memory, M filled in fc_batch_launch's row blocks): in float32, with the channels in natural order and in the
    LDS-DMA kernel's K order, plus the bias it is c.want.  Teeth: the same statement with the second row block of the 304-row cut
    starting at row 320 is reported (at the shapes that have a second block under the cut)."""
    for relu in (0, 1) if (H, W, Cin, Cout) == E.WINO4_SPLIT[1] else (0,):
        c = E.wino_case(4, H, W, Cin, Cout, relu=relu)
        assert c.bits > 0, c.what
        print(c.what)
        finish = lambda y: np.maximum(y + c.b[:, None, None], 0) if relu else y + c.b[:, None, None]
        for name, order in (("natural", [np.arange(Cin)]), ("dma", [E.dma_k_order(Cin)])):
            got = finish(E.wino4_split_f32(c.a, c.w, order))
            assert got.dtype == np.float32 and E.same(got, c.want), (c.what, name)
            assert E.same(finish(E.wino_f32(c.a, c.w, 4, order)), c.want), (c.what, name)
        blocks = E.batch_row_blocks(-(-H // 4) * -(-W // 4))
        if len(blocks) > 1 and blocks[0][1] == 304 and not relu:
            wrong = finish(E.wino4_split_f32(c.a, c.w, [E.dma_k_order(Cin)], first=320))
            assert not E.same(wrong, c.want), c.what
            bad = np.argwhere(~(wrong == c.want))
            print("  second block from row 320: %d of %d values differ, first at %s" % (len(bad), wrong.size, bad[0].tolist()))


@pytest.mark.parametrize("M,N,K", E.FC_BATCH)
def test_fc_batch_cases_hold_their_preconditions(M, N, K):
    """The products of test_gpu_exact_arithmetic.py::test_fc_batch: the builders assert representability and headroom; without the
    bias (mnc_fc_batch adds none) the expected value is still an fp32 value, in the DMA kernel's K order too."""
    for family in E.families("fp32"):
        for seed in (0, 1, 2):
            c = E.fc_case(family, "fp32", M, N, K, seed=seed)
            want = c.want.astype(np.float64) - c.b.astype(np.float64)
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want), c.what
            idx = E.dma_k_order(K)
            assert E.same(np.matmul(c.a[:, idx], c.w[:, idx].T), want), c.what


# defect -> (the families that must catch it, the modes it exists in, convolutions only)
DEFECTS = {"a_lo": (("split_a",), ("bf16x3",), False), "b_lo": (("split_w",), ("bf16x3",), False),
           "f16": (("int", "impulse"), ("fp32",), False), "tap": (("int",), E.MODES, True), "twice": (("int",), E.MODES, False)}


def test_every_defect_has_a_family_that_catches_it():
    for defect, (fams, modes, _) in DEFECTS.items():
        assert any(f in E.families(m) for f in fams for m in modes), defect


@pytest.mark.parametrize("kind,row", ROWS, ids=[row_id(p) for p in ROWS])
def test_preconditions_summation_orders_and_defects(kind, row):
    """Every case the GPU file builds for one row of its shape lists:
      * the builders assert representability and headroom themselves; the headroom reached is printed;
      * forward, shuffled and in K ranges summed afterwards, the float32 evaluation is the reference exactly;
      * each defect is detected by the families named in DEFECTS, and what the range-relative bar makes of it is printed (the
        module docstring has the table over all rows)."""
    rng = np.random.default_rng(3)
    n = 0
    for mode, family, c in row_cases(kind, row):
        if c.bits is not None:
            assert c.bits > 0, c.what
        print(c.what)
        Kdim = c.a.shape[1] if c.kind == "fc" else c.a.shape[0] * c.geom[0] ** 2
        ords = orders(Kdim, rng)
        for name in ords if not c.relu else ("ranges",):
            got = eval32(c, mode, ords[name])
            assert got.dtype == np.float32 and E.same(got, c.want), (c.what, name)
            n += 1
        if c.relu:
            continue
        for defect, (fams, modes, conv_only) in DEFECTS.items():
            if family not in fams or mode not in modes or (conv_only and c.kind != "conv"):
                continue
            got = eval32(c, mode, ords["ranges"], defect)
            assert not E.same(got, c.want), "%s: the defect %r is not detected" % (c.what, defect)
            rel = err(got, c.want)[1]
            print("  defect %-5s detected; relative to the range %.1e: the 1e-4 bar %s it" % (defect, rel, "PASSES" if rel < 1e-4 else "fails"))
    assert n >= 3


def test_every_fc_plan_is_reached(shim):
    """Which plan of fc_plan.h each InnerProduct shape of the GPU file reaches, under the settings the GPU file forces."""
    def kinds(which, rows, tunings=(None,), splits=False, **kw):
        out = set()
        for M, N, K, pad in rows:
            for t in tunings:
                for _, call, p in shim.launches(which, dict(M=M, N=N, K=K, ldc=N + pad, mstride=M, osm_rows=M, **kw), t):
                    out.add((p["kernel"], p["mt"], min(p["tm"], 2), call["ldc"] > N) + ((p["splits"] > 1,) if splits else ()))
        return out
    fp32 = kinds(FC, E.FC + E.FC_MORE, (None, [("FC_TILE", 10), ("FC_DMA", 1)], [("FC_TILE", 10), ("FC_DMA", 0)]))
    for want in ((STAGED, 2, 1, False), (STAGED, 2, 2, False), (STAGED, 2, 2, True), (STAGED, 5, 1, False), (STAGED, 10, 1, False),
                 (STAGED, 10, 2, False), (DMA16, 10, 1, False), (DMA16, 10, 2, False), (DMA16, 10, 1, True)):
        assert want in fp32, want
    assert shim.plan(FC, dict(M=700, N=512, K=4096, ldc=512))["head"] == 640                        # head + tail launches
    pair = {row: shim.plan(FC_PAIR, dict(M=row[0], N=row[1], K=row[2], ldc=row[1] + row[3]))["two_singles"] for row in E.FC_PAIR + E.FC_MORE[1:]}
    assert pair == {(640, 512, 8192, 0): 0, (300, 1024, 4096, 0): 0, (120, 512, 4096, 0): 1, (700, 512, 4096, 0): 1, (300, 520, 4096, 8): 1,
                    (300, 520, 8192, 8): 0}
    for f16 in (0, 1, 2):
        low = kinds(LOWP, E.FC + E.FC_MORE + [E.FC_WIDE8], (None, ("FCX3_WIDE", 0), ("FCX3_WIDE", 1)), f16=f16)
        # (the 256-column kernel alone: with K ranges at one and at several row blocks, and without any)
        wide = kinds(LOWP, E.FC + E.FC_MORE + [E.FC_WIDE8, E.FC_WIDE_UNCUT], splits=True, f16=f16)
        for want in ((WIDE, 10, 1, False, True), (WIDE, 10, 1, False, False), (WIDE, 8, 2, False, True)):
            assert want in wide, (f16, want)
        low |= kinds(LOWP, [E.FCX3_TILE], (("FCX3_TILE", 5), ("FCX3_TILE", 8), ("FCX3_TILE", 10)), f16=f16)
        for want in ((X3, 2, 1, False), (X3, 2, 2, False), (X3, 2, 2, True), (X3, 5, 1, False), (X3, 5, 2, False), (X3, 8, 2, False),
                     (X3, 8, 2, True), (X3, 10, 1, True), (WIDE, 10, 1, False), (WIDE, 8, 2, False)):
            assert want in low, (f16, want)
        # the paired launches with their K ranges (splits > 1: partial sums + the pair reduction), under the settings the GPU file runs:
        # the one-row-block pair is cut only under PLAN=1 / FC_SPLIT_DIV=0, the several-row-block pairs stay paired under FC_SPLIT_DIV=0
        pairs = {}
        for M, N, K, pad in E.FC_PAIR[:4] + E.FC_LOWP_PAIRED:
            for t in (None, ("PLAN", 1), ("FC_SPLIT_DIV", 0)):
                p = shim.plan(LOWP_PAIR, dict(M=M, N=N, K=K, ldc=2 * N, mstride=M, f16=f16), t)
                if not p["two_singles"]:
                    pairs[(M, N, K, t[0] if t else None)] = (p["kernel"], p["mt"], p["tm"], p["splits"])
        assert pairs == {(640, 512, 8192, None): (WIDE, 10, 2, 16), (640, 512, 8192, "FC_SPLIT_DIV"): (WIDE, 10, 2, 16),
                         (700, 512, 8192, None): (WIDE, 8, 3, 10), (700, 512, 8192, "FC_SPLIT_DIV"): (WIDE, 8, 3, 10),
                         (290, 2048, 8192, None): (WIDE, 10, 1, 1), (290, 2048, 8192, "PLAN"): (WIDE, 10, 1, 16),
                         (290, 2048, 8192, "FC_SPLIT_DIV"): (WIDE, 10, 1, 16)}, f16
        assert any(v[2] == 1 and v[3] > 1 for v in pairs.values())          # a one-row-block pair WITH K ranges is among them
        # mixed inputs: one launch while the strides agree, the two single calls when the pre-packed panel has its own
        for M, N, K, pad in E.FC_MIXED + [E.FC_LOWP_PAIRED[0], E.FC_LOWP_PAIRED[2]]:
            for pre in ((1, 0), (0, 1)):
                call = dict(M=M, N=N, K=K, ldc=2 * N, f16=f16, pre0=pre[0], pre1=pre[1])
                same_stride = shim.plan(LOWP_PAIR, dict(call, mstride=M))["two_singles"]
                assert same_stride == (1 if (M, N, K, pad) in E.FC_MIXED else 0), (f16, M, N, K, pre)
                assert shim.plan(LOWP_PAIR, dict(call, mstride=M + 20))["two_singles"] == 1, (f16, M, N, K, pre)
