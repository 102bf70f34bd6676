"""GPU: the LDS-DMA, split-K and cooperating kernels on a context stream while three other streams share the CUs, the caches and
the memory system (tests/contention.py: a twin of the case on another input, mnc_fc 300 x 4096 x 4096, mnc_add over 3 x 256 MB).
Round 4's F(4x4) race passed every unit test -- back-to-back launches of one kernel keep the waves in step -- and showed only in a
whole pipeline with other images in flight; this module is the seconds-long unit test under that condition.

Every case: 16 launches alone, then 16 under the schedule, two inputs alternating through the same scratch, slabs and tickets, each
launch into its own NaN-filled output.  Every contended result is compared by value, element for element (np.array_equal's rule, as exact() of
tests/test_gpu_exact_arithmetic.py: -0.0 equals +0.0), with the independent reference (the integer
answer of tests/exact_inputs.py for the matrix-pipe kernels, oracle.host for the rest) and with the kernel's own solo result; the
twin's last output with its own reference.  At least half of the contended launches must have taken longer than the slowest solo
launch (measured with mnc_prof_enable on the context under test only), or the test fails: the contention was not real.

Plans, as the launchers read (wino4_plan, wino_impl, sw_plan, fc_plan.h through the CPU shim):
  F(4x4) 37x63 256->512     80 workgroups (5 pixel x 16 channel tiles) in 4 uniform K ranges, finished inside the launch
  F(4x4) 78x250 128->512    the tail plan: 40 x 16 = 640 workgroups, 32 pixel tiles whole, 8 cut into 4 ranges = 128 cut tiles with
                            tickets and slabs.  (150x250 128->512 is 76 x 16 = 1216 workgroups -- the workgroup is 8 rows high -- whose
                            192 tail workgroups the plan leaves whole; this is the nearest shape that takes the tail plan.)
  F(4x4) 38x63 64->128 and 13x33 128->256   by default 2 and 4 uniform ranges; the unsplit kernel is forced with CONV_KSPLIT=1
  F(2x2) 37x63 256->512     tail plan: 160 tail workgroups in 3 ranges + wino_section_reduce_kernel
  lowp 38x63 256->256       plan 2 = (1, 1, 4): four K ranges per workgroup
  lowp 75x125 128->128      plan 0 = (2, 2, 1) (64 workgroups reach P0MIN); (2, 2, 2) is the launcher's choice only under PLAN=1 with
                            128 .. 383 workgroups: 75x125 128->256 under PLAN=1 is the nearest shape and runs beside it
  mnc_fc 300x1024x25088     DMA16 kernel, 32 K ranges, in-launch slab reduction; FC_DMA's shapes under FC_TILE=10, FC_DMA=1: 16 / 8 ranges
  mnc_fc_pair 300x1024x4096 one paired DMA16 launch, 16 ranges
  lowp fc 300x4096x4096     256-column kernel, 2 ranges; the pair there one launch without ranges; 640x512x8192 paired with 16 ranges
  F(4x4) split 76x68 256->384   input transform, 36 positions x (304 + 19 rows) x 3 column tiles = 216 workgroups of the DMA16
                            kernel's BATCH build with 8 K stages each, output transform; 102x103 32->64: 36 x 3 row blocks, one stage
  fc_f8 300x256x4480        quantiser, product kernel in 2 K ranges (18 + 17 stages), f8_reduce_kernel; 321x256x1024: two row blocks
                            by two ranges; 300x441x512: one range, fused epilogue (two launches)

The bandwidth disturber is mnc_add (with it and the other two every case below reaches the share; mnc_roi_warp was not needed).
Measured on an MI355X, one run (disturbed launches of 16, median contended / median solo duration, wall time of the test, which
where it exceeds a second is the CPU's for the exact cases; fp32 / bf16x3 / f16 side by side where a test has them):
  case                                              disturbed        stretch              seconds
  wino4 37x63 256->512, _pool                       16, 16           2.71x, 3.10x         1.11, 0.07
  wino4 78x250 128->512 (tail plan), _pool          16, 16           4.65x, 4.57x         5.77, 0.41
  wino4 unsplit 38x63 64->128, 13x33 128->256       16, 16           3.82x, 3.06x         0.13, 0.13
  wino4_pool unsplit, the same two shapes           16, 16           3.99x, 3.80x         (below 1.7 each: a later run, in which
                                                                                          only the 25 slowest tests were listed)
  wino4 FC_REDUCE=0 37x63 256->512                  16               3.81x                0.06
  wino F(2x2) 37x63 256->512                        16               3.76x                1.99
  conv lowp 38x63 256->256 (bf16x3, f16)            14, 15           4.30x, 5.17x         0.14, 0.16
  conv lowp 75x125 128->128                         16, 16           3.09x, 4.38x         0.23, 0.24
  conv lowp 75x125 128->256 PLAN=1                  16, 16           4.63x, 7.36x         0.39, 0.38
  conv lowp 23x70 64->128 plan 0                    16, 16           4.89x, 7.33x         0.05, 0.05
  conv lowp 23x70 64->128 plan 1                    15, 15           5.73x, 8.10x         0.02, 0.03
  conv lowp 23x70 64->128 plan 2                    16, 16           7.06x, 8.63x         0.02, 0.02
  conv lowp 23x70 64->128 plan 3                    16, 15           5.54x, 7.31x         0.02, 0.02
  fc fp32 300x1024x25088                            16               2.67x                0.93
  fc fp32 300x520x4096 ldc+8, 290x1024x2112 (DMA)   16, 16           4.04x, 3.49x         0.10, 0.11
  fc_pair fp32 300x1024x4096                        16               3.83x                0.40
  fc 300x4096x4096 (f16, bf16x3)                    16, 16           2.68x, 1.99x         0.91, 1.04
  fc_lowp_pair f16 300x4096x4096                    16               2.47x                0.97
  fc_lowp_pair bf16x3 300x4096x4096                 16               1.64x                (below 1.7, the same later run)
  fc_lowp_pair 640x512x8192 (f16, bf16x3)           16, 16           4.80x, 3.70x         0.76, 1.19
  wino4_split 76x68 256->384, _pool                 16, 16           2.86x, 3.20x         1.90, 0.10   (these six: a later run)
  wino4_split 102x103 32->64                        16               8.94x                0.22
  fc_f8 300x256x4480, 321x256x1024, 300x441x512     16, 16, 16       4.69x, 6.17x, 2.53x  0.81, 0.21, 0.17
  proposal 38x63 (wide, single-workgroup top-K)     16, 16           4.43x, 1.82x         0.22, 0.03
  vote_instances 600 @ 600x1000                     15               1.29x                1.96
The shares of the small kernels move from run to run (launches of 10 .. 20 us against a bar that is the slowest of sixteen): the
lowest seen in six runs were 11 of 16 (conv lowp plan 2, both modes), 12 of 16 (vote_instances, whose chain of small dependent
launches stretches least) and 13 of 16 (conv lowp f16 under PLAN=1); every other case stayed at 14 or more.  The launches that
were not disturbed lie scattered among the sixteen, not at the end: the disturbers did not run dry.  Each case prints its line (share, stretch, which launches were
disturbed, the solo durations, the pre-roll): run with -s or -rA to see them.
On a scratch build without the barrier "every wave has read halo 0 before anybody's first copies" of conv_wino4.hip the seven
F(4x4) cases above that are not wino4_pool unsplit (those two were not run on it) fail: five at the first contended launch after sixteen correct solo launches, the two tail-plan cases already
alone; test_gpu_ops.py::test_conv3x3_winograd_f4_is_bit_reproducible fails one of its seven shapes on that build.
"""
import numpy as np
import pytest

import contention as CT
import exact_inputs as E
import f8_inputs as F8
import golden_inputs as GI
import mnc_amd
from gpu_util import Dev, from_c8, to_c8
from mnc_amd import _lib

mnc_amd.install_paths()

pytestmark = pytest.mark.gpu

WINO4_TAIL = (78, 250, 128, 512)
_CASES = {}


def case(kind, *args, **kw):
    """The exact case of tests/exact_inputs.py, made once per module and left unchanged."""
    key = (kind, args, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = getattr(E, kind)(*args, **kw)
    return _CASES[key]


@pytest.fixture(scope="module")
def dev():
    d = Dev(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def disturbers():
    d = CT.Disturbers(3)
    yield d
    d.close()


def running(dev, n_slots, outs, launch, wants, post):
    """outs: [(shape, dtype)] of one slot's buffers, n_slots of them pre-filled with NaN (-1 for integers); launch(i, buffers);
    post(arrays) -> the list compared with wants[i]."""
    nan = [np.full(s, np.nan if np.dtype(t).kind == "f" else -1, t) for s, t in outs]
    slots = [[dev.put(a, a.dtype) for a in nan] for _ in range(n_slots)]

    def fill(k):
        for p, a in zip(slots[k], nan):
            dev.put_into(p, a)
    return CT.Running(lambda i, k: launch(i, slots[k]), lambda k: post([dev.get(p, s, t) for p, (s, t) in zip(slots[k], outs)]), fill,
                      wants, slots)


# ---------------------------------------------------------------- builders: build(dev, seeds, slots) -> Running
def wino(m, shape, pool=False):
    H, W, Cin, Cout = shape
    fn = ("mnc_conv3x3_wino4" if m == 4 else "mnc_conv3x3_wino") + ("_pool" if pool else "")
    OH, OW = ((H + 1) // 2, (W + 1) // 2) if pool else (H, W)

    def build(dev, seeds, slots):
        cs = [case("wino_case", m, H, W, Cin, Cout, seed=s) for s in seeds]
        ins = []
        for c in cs:
            d_w = dev.empty((Cin * Cout * (36 if m == 4 else 17),), fill=np.nan)
            dev.call("mnc_pack_conv3x3_wino4" if m == 4 else "mnc_pack_conv3x3_wino", dev.put(c.w), d_w, Cout, Cin)
            ins.append((dev.put(to_c8(c.a)), d_w, dev.put(c.b)))
        wants = [[E.maxpool2_ceil(c.want) if pool else c.want] for c in cs]
        return running(dev, slots, [((Cout * OH * OW,), np.float32)],
                       lambda i, o: dev.call(fn, ins[i][0], ins[i][1], ins[i][2], o[0], H, W, Cin, Cout, 0), wants,
                       lambda a: [from_c8(a[0], Cout, OH, OW)])
    return build


def wino4_split(shape, pool=False):
    """mnc_conv3x3_wino4_split / _split_pool: every context has ONE workspace (V and M of conv_wino4_split.hip), which both
    alternating inputs go through, as a net's layers do; it starts NaN-filled."""
    H, W, Cin, Cout = shape
    fn = "mnc_conv3x3_wino4_split" + ("_pool" if pool else "")
    OH, OW = ((H + 1) // 2, (W + 1) // 2) if pool else (H, W)

    def build(dev, seeds, slots):
        cs = [case("wino_case", 4, H, W, Cin, Cout, seed=s) for s in seeds]
        ins = []
        for c in cs:
            d_u = dev.empty((36 * Cout * Cin,), fill=np.nan)
            dev.call("mnc_pack_conv3x3_wino4_split", dev.put(c.w), d_u, Cout, Cin)
            ins.append((dev.put(to_c8(c.a)), d_u, dev.put(c.b)))
        nb = int(_lib.load().mnc_conv3x3_wino4_split_ws_bytes(H, W, Cin, Cout))
        assert nb > 0
        d_ws = dev.empty((nb // 4,), fill=np.nan)
        wants = [[E.maxpool2_ceil(c.want) if pool else c.want] for c in cs]
        return running(dev, slots, [((Cout * OH * OW,), np.float32)],
                       lambda i, o: dev.call(fn, ins[i][0], ins[i][1], ins[i][2], o[0], d_ws, H, W, Cin, Cout, 0), wants,
                       lambda a: [from_c8(a[0], Cout, OH, OW)])
    return build


def fc_f8(row):
    """mnc_fc_f8 on fp32 rows with ldc = N + 2 (weights packed once per input): the row quantiser, the product kernel and, with K
    ranges, f8_reduce_kernel, chained through the context's scratch.  Compared as bits with f8_inputs.exact_case's integer answer."""
    M, N, K = row
    ld = N + 2

    def build(dev, seeds, slots):
        cs = [f8_case(M, N, K, s) for s in seeds]
        nb, tiles = _lib.load().mnc_pack_fc_f8_bytes(N, K), -(-N // 256)
        assert nb == tiles * 256 * K
        ins = []
        for c in cs:
            d_q, d_e = dev.alloc(nb), dev.alloc(tiles * 256 * 4)
            dev.call("mnc_pack_fc_f8", dev.put(c.w), d_q, d_e, N, K)
            ins.append((dev.put(c.a), d_q, d_e, dev.put(c.bias)))
        wants = [[c.want.astype(np.float32).view(np.uint32), np.ones((M, 2), bool)] for c in cs]
        return running(dev, slots, [((M, ld), np.float32)],
                       lambda i, o: dev.call("mnc_fc_f8", ins[i][0], ins[i][1], ins[i][2], ins[i][3], o[0], M, N, K, ld, 0), wants,
                       lambda a: [a[0].view(np.uint32)[:, :N], np.isnan(a[0][:, N:])])
    return build


def f8_case(M, N, K, seed):
    key = ("f8", M, N, K, seed)
    if key not in _CASES:
        _CASES[key] = F8.exact_case(M, N, K, seed=seed, small=True)
    return _CASES[key]


def words(mode, n):
    return n if mode == "bf16x3" else n // 2


def lowp_conv(mode, shape):
    H, W, Cin, Cout = shape
    m = E.LOWP[mode]

    def build(dev, seeds, slots):
        nb = _lib.load().mnc_conv3x3_lowp_weight_bytes(m, Cout, Cin)
        assert nb > 0
        cs = [case("conv_case", "int", mode, H, W, Cin, Cout, seed=s) for s in seeds]
        ins = []
        for c in cs:
            d_w = dev.empty((nb // 4,), fill=np.nan)
            dev.call("mnc_pack_conv3x3_lowp", m, dev.put(c.w), d_w, Cout, Cin)
            d_xp = dev.empty((words(mode, Cin * H * W),), fill=np.nan)
            dev.call("mnc_act_pack", dev.put(to_c8(c.a)), d_xp, Cin * H * W, m)
            ins.append((d_xp, d_w, dev.put(c.b)))
        return running(dev, slots, [((Cout * H * W,), np.float32)],
                       lambda i, o: dev.call("mnc_conv3x3_lowp", m, ins[i][0], ins[i][1], ins[i][2], None, o[0], H, W, Cin, Cout, 0),
                       [[c.want] for c in cs], lambda a: [from_c8(a[0], Cout, H, W)])
    return build


def slice_and_rest(N):
    """An [M, ld] output -> (the N result columns, the columns behind them, which must still hold the NaN fill)."""
    return lambda a: [x for o in a for x in (o[:, :N], np.isnan(o[:, N:]))]


def lowp_weights(dev, mode, c, N, K):
    d = dev.empty(((N + 127) // 128 * 128 * K // (1 if mode == "bf16x3" else 2),), fill=np.nan)
    dev.call("mnc_pack_fc_" + mode, dev.put(c.w), d, N, K)
    return d


def fc(mode, row):
    """mnc_fc (mode "fp32") / mnc_fc_<mode> with ldc = N + pad."""
    M, N, K, pad = row
    ld = N + pad

    def build(dev, seeds, slots):
        cs = [case("fc_case", "int", mode, M, N, K, seed=s) for s in seeds]
        ins = [(dev.put(c.a), dev.put(c.w) if mode == "fp32" else lowp_weights(dev, mode, c, N, K), dev.put(c.b)) for c in cs]
        fn = "mnc_fc" if mode == "fp32" else "mnc_fc_" + mode
        return running(dev, slots, [((M, ld), np.float32)], lambda i, o: dev.call(fn, ins[i][0], ins[i][1], ins[i][2], o[0], M, N, K, ld, 0),
                       [[c.want, np.ones((M, pad), bool)] for c in cs], slice_and_rest(N))
    return build


def fc_pair(mode, row):
    """mnc_fc_pair (mode "fp32": two output buffers) / mnc_fc_lowp_pair on fp32 rows (column slices of one buffer, ldc = 2 N, product 0
    in the right half); input i is the pair of seeds (2 i, 2 i + 1)."""
    M, N, K, pad = row

    def build(dev, seeds, slots):
        cs = [[case("fc_case", "int", mode, M, N, K, seed=2 * s + j) for j in (0, 1)] for s in seeds]
        if mode == "fp32":
            ld = N + pad
            ins = [[(dev.put(c.a), dev.put(c.w), dev.put(c.b)) for c in pair] for pair in cs]

            def launch(i, o):
                (a0, w0, b0), (a1, w1, b1) = ins[i]
                dev.call("mnc_fc_pair", a0, w0, b0, o[0], a1, w1, b1, o[1], M, N, K, ld, 0)
            return running(dev, slots, [((M, ld), np.float32)] * 2, launch,
                           [[p[0].want, np.ones((M, pad), bool), p[1].want, np.ones((M, pad), bool)] for p in cs], slice_and_rest(N))
        ins = [[(dev.put(c.a), lowp_weights(dev, mode, c, N, K), dev.put(c.b)) for c in pair] for pair in cs]

        def launch(i, o):
            (a0, w0, b0), (a1, w1, b1) = ins[i]
            dev.call("mnc_fc_lowp_pair", E.LOWP[mode], a0, None, a1, None, M, w0, w1, b0, b1, o[0] + N * 4, o[0], M, N, K, 2 * N, 0,
                     None, None, 0)
        return running(dev, slots, [((M, 2 * N), np.float32)], launch, [[p[0].want, p[1].want] for p in cs], lambda a: [a[0][:, N:], a[0][:, :N]])
    return build


def proposal_inputs(seed):
    key = ("proposal", seed)
    if key not in _CASES:
        from oracle import host as ohost
        pc = GI.proposal_case(38, 63, seed)
        prob, bbox, info = pc["cls_prob"].copy(), pc["bbox_pred"].copy(), pc["im_info"]
        prob = (np.round(prob * 64) / 64).astype(np.float32)       # thousands of exact ties
        bbox[:, 2::4] -= 2.5                                       # many boxes shrink below RPN_MIN_SIZE and are filtered
        rois = ohost.proposal_forward(prob, bbox, info)
        want = np.zeros((300, 5), np.float32)                      # rows past the row count are zero
        want[:len(rois)] = rois
        _CASES[key] = (prob, bbox, info, want)
    return _CASES[key]


def proposal(dev, seeds, slots):
    from transform.anchors import generate_anchors
    anchors = np.ascontiguousarray(generate_anchors(), np.float32)
    cs = [proposal_inputs(5 + s) for s in seeds]
    ins = [(dev.put(c[0]), dev.put(c[1]), c[2]) for c in cs]

    def launch(i, o):
        info = ins[i][2]
        dev.call("mnc_proposal", ins[i][0], ins[i][1], 9, 38, 63, _lib.ptr(anchors), 16, float(info[0, 0]), float(info[0, 1]),
                 float(info[0, 2]), 6000, 300, 0.7, 16.0, o[0], None)
    run = running(dev, slots, [((300, 5), np.float32)], launch, [[c[3]] for c in cs], lambda a: a)
    run.anchors = anchors                                          # (the launches read it: kept alive with the case)
    return run


VOTE_CAP = 128


def voting_inputs(seed):
    key = ("voting", seed)
    if key not in _CASES:
        from mnc_amd.instances import records_from_lists
        from oracle import host as ohost
        vc = GI.voting_case(600, 600, 1000, seed)
        om, ob = ohost.gpu_mask_voting(vc["masks"], vc["boxes"], vc["scores"], 21, 100, 1000, 600)
        rec, total = records_from_lists(om, ob, VOTE_CAP)
        assert total <= VOTE_CAP
        counts = np.array([total] + [len(b) for b in ob], np.int32)
        _CASES[key] = (vc, rec, counts)
    return _CASES[key]


def voting(dev, seeds, slots):
    from oracle import host as ohost
    cs = [voting_inputs(23 + s) for s in seeds]
    ins = [(dev.put(c[0]["boxes"]), dev.put(c[0]["masks"]), dev.put(c[0]["scores"])) for c in cs]

    def launch(i, o):
        dev.call("mnc_vote_instances", ins[i][0], ins[i][1], ins[i][2], 600, 21, 21, 100, float(ohost.MASK_MERGE_NMS_THRESH),
                 float(ohost.MASK_MERGE_IOU_THRESH), 600, 1000, o[0], VOTE_CAP, o[1])
    return running(dev, slots, [((VOTE_CAP, 6 + 21 * 21), np.float32), ((21,), np.int32)], launch, [[c[1], c[2]] for c in cs], lambda a: a)


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", [E.WINO4_REDUCE, WINO4_TAIL])
def test_wino4_in_launch_reduction(dev, disturbers, shape, pool):
    """mnc_conv3x3_wino4 / _wino4_pool with K ranges finished inside the launch (uniform ranges; the tail plan's cut tiles).  Hazard:
    cross-workgroup publication inside a launch -- slabs and arrival tickets (slab_last_arriver) with workgroups that are not
    co-resident -- and the intra-workgroup refill of the halo buffers against a slow reader."""
    CT.contended_kernel(dev, disturbers, wino(4, shape, pool), "wino4%s %dx%d %d->%d" % (("_pool" if pool else "",) + tuple(shape)))


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", [E.CONV3[5], E.CONV3[3]])
def test_wino4_unsplit_kernel(dev, disturbers, shape, pool):
    """mnc_conv3x3_wino4 / _wino4_pool unsplit (CONV_KSPLIT=1): many short workgroups.  Hazard: the intra-workgroup refill of an LDS
    buffer (halo refill, half-panel pipeline) against a slow reader -- round 4's race."""
    CT.contended_kernel(dev, disturbers, wino(4, shape, pool), "wino4%s unsplit %dx%d %d->%d" % (("_pool" if pool else "",) + tuple(shape)),
                        [("CONV_KSPLIT", "1")])


def test_wino4_separate_reduction_kernel(dev, disturbers):
    """mnc_conv3x3_wino4 with FC_REDUCE=0: the separate reduction kernel reads slabs.  Hazard: per-context scratch beside another
    context's (the twin runs the same plan on its own scratch)."""
    CT.contended_kernel(dev, disturbers, wino(4, E.WINO4_REDUCE), "wino4 FC_REDUCE=0 %dx%d %d->%d" % E.WINO4_REDUCE, [("FC_REDUCE", "0")])


@pytest.mark.parametrize("shape,pool", [(E.WINO4_SPLIT[2], False), (E.WINO4_SPLIT[2], True), (E.WINO4_SPLIT[4], False)])
def test_wino4_split(dev, disturbers, shape, pool):
    """mnc_conv3x3_wino4_split / _split_pool: three dependent launches through one workspace per context, the middle one
    fc_mfma_dma16_kernel's BATCH instantiation.  Hazards: the steady-state loop's waits and barriers of that instantiation (eight K
    stages at 256 input channels) against slow waves; the next launch's input transform overwriting V, and its batched launch M,
    behind the previous launch's readers (stream order is all that separates them); per-context workspace beside another's."""
    CT.contended_kernel(dev, disturbers, wino4_split(shape, pool), "wino4_split%s %dx%d %d->%d" % (("_pool" if pool else "",) + tuple(shape)))


@pytest.mark.parametrize("row", [(300, 256, 4480), (321, 256, 1024), (300, 441, 512)])
def test_fc_f8(dev, disturbers, row):
    """mnc_fc_f8: K ranges of 18 and 17 stages plus the reduction; two row blocks by two ranges; one range with the fused epilogue.
    Hazards: the quantised rows, their exponents and the partial sums live in the context's scratch and are re-used by the next
    launch (stream order alone separates the quantiser, the product kernel and the reduction); the product kernel's pipelined LDS
    stages against slow waves; per-context scratch beside another context's."""
    CT.contended_kernel(dev, disturbers, fc_f8(row), "fc_f8 %dx%dx%d ldc+2" % tuple(row))


def test_wino2_tail_plan_reduce(dev, disturbers):
    """mnc_conv3x3_wino (F(2x2)): its tail plan and wino_section_reduce_kernel.  Hazard: per-context scratch beside another
    context's, and the intra-workgroup LDS refill of the two-row-group kernel."""
    CT.contended_kernel(dev, disturbers, wino(2, E.WINO4_REDUCE), "wino F(2x2) %dx%d %d->%d" % E.WINO4_REDUCE)


@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
@pytest.mark.parametrize("shape,tunes", [((38, 63, 256, 256), ()), ((75, 125, 128, 128), ()), ((75, 125, 128, 256), (("PLAN", "1"),))])
def test_conv_lowp_own_plan(dev, disturbers, mode, shape, tunes):
    """mnc_conv3x3_lowp under the launcher's own plan: (1, 1, 4), (2, 2, 1) and, under PLAN=1, (2, 2, 2).  Hazard: intra-workgroup --
    two or four K ranges per workgroup with per-wave waits and no workgroup barrier per pass, summed through LDS."""
    CT.contended_kernel(dev, disturbers, lowp_conv(mode, shape), "conv lowp %s %dx%d %d->%d %s" % ((mode,) + tuple(shape) + (dict(tunes),)), tunes)


@pytest.mark.parametrize("mode", ["bf16x3", "f16"])
@pytest.mark.parametrize("plan", [0, 1, 2, 3])
def test_conv_lowp_every_plan(dev, disturbers, mode, plan):
    """mnc_conv3x3_lowp, every instantiation (CONVX3_TILE=100..103) at E.LOWP_PLAN.  Hazard: as test_conv_lowp_own_plan."""
    CT.contended_kernel(dev, disturbers, lowp_conv(mode, E.LOWP_PLAN), "conv lowp %s plan %d" % (mode, plan), [("CONVX3_TILE", 100 + plan)])


@pytest.mark.parametrize("row,tunes", [((300, 1024, 25088, 0), ()), (E.FC_DMA[0], (("FC_TILE", "10"), ("FC_DMA", "1"))),
                                       (E.FC_DMA[1], (("FC_TILE", "10"), ("FC_DMA", "1")))])
def test_fc_fp32(dev, disturbers, row, tunes):
    """mnc_fc: the LDS-DMA kernel with K ranges and the slab reduction (default plan at head size; forced on FC_DMA's shapes).
    Hazard: cross-workgroup publication inside a launch, per-context scratch and tickets beside another context's."""
    CT.contended_kernel(dev, disturbers, fc("fp32", row), "fc fp32 %dx%dx%d+%d %s" % (tuple(row) + (dict(tunes),)), tunes)


def test_fc_pair_fp32(dev, disturbers):
    """mnc_fc_pair at E.FC_PAIR[1]: one paired DMA16 launch with 16 K ranges.  Hazard: cross-workgroup publication inside a launch."""
    CT.contended_kernel(dev, disturbers, fc_pair("fp32", E.FC_PAIR[1]), "fc_pair fp32 %dx%dx%d" % E.FC_PAIR[1][:3])


@pytest.mark.parametrize("mode", ["f16", "bf16x3"])
def test_fc_reduced_precision(dev, disturbers, mode):
    """mnc_fc_f16 / mnc_fc_bf16x3 at 300 x 4096 x 4096 (K ranges, partial sums in the context's scratch).  Hazard: per-context
    scratch beside another context's; intra-workgroup LDS staging."""
    CT.contended_kernel(dev, disturbers, fc(mode, (300, 4096, 4096, 0)), "fc %s 300x4096x4096" % mode)


@pytest.mark.parametrize("mode,row", [("f16", (300, 4096, 4096, 0)), ("bf16x3", (300, 4096, 4096, 0)), ("f16", E.FC_LOWP_PAIRED[0]),
                                      ("bf16x3", E.FC_LOWP_PAIRED[0])])
def test_fc_lowp_pair(dev, disturbers, mode, row):
    """mnc_fc_lowp_pair on fp32 rows: one launch without K ranges (300 x 4096 x 4096) and the paired launch with 16 ranges and the
    pair reduction (E.FC_LOWP_PAIRED[0]).  Hazard: per-context scratch (the converted panels, the partial sums) beside another
    context's."""
    CT.contended_kernel(dev, disturbers, fc_pair(mode, row), "fc_lowp_pair %s %dx%dx%d" % ((mode,) + tuple(row[:3])))


@pytest.mark.parametrize("single", [False, True])
def test_proposal(dev, disturbers, single):
    """mnc_proposal (asynchronous form) on 38 x 63 with scores quantised to 1/64: the multi-workgroup top-K (sorted runs + rank merge)
    and the single-workgroup radix select.  Hazard: cross-launch state in the context's proposal arena beside another context's;
    the NMS scan's flags."""
    CT.contended_kernel(dev, disturbers, proposal, "proposal 38x63 %s top-K" % ("single-workgroup" if single else "wide"),
                        [("TOPK_SINGLE_WG", "1")] if single else [])


def test_vote_instances(dev, disturbers):
    """mnc_vote_instances on 600 instances, 600 x 1000: order, per-class NMS, threshold, result rows and voting as one asynchronous
    sequence.  Hazard: per-context voting scratch beside another context's; kernels that hand counts to the next launch."""
    CT.contended_kernel(dev, disturbers, voting, "vote_instances 600 @ 600x1000")
