"""Inputs on which the dense kernels have exactly one right answer, in every math mode.

If every operand is exactly representable in the form a mode feeds the matrix pipe and every product and partial sum is a whole
multiple of one unit below 2^24 units, then fp32 MFMA, Winograd, split-K with slabs, the bf16x3 split, f16 and bf16 all give the
same bits in any summation order: the integer result.  Each builder returns a Case (inputs + the expected output, computed in
float64 from the plain definition of the operation on integer-valued data, where float64 is exact) and asserts its own
preconditions on the CPU: representability (the rounding rules of mnc_amd/csrc/x3_split.h, emulated here) and headroom (the largest
sum |a||w| over any output element, in units, below 2^24; the achieved headroom in bits is in the assert message and in Case.bits).

Families: "int" (small integers x a power of two), "wino" (weights a multiple of 576 x 2^e / 4 x 2^e, so that G g G^T is whole),
"split_a" / "split_w" / "split_0" (bf16x3: which operand carries a non-zero lo term), "impulse" (one-hot weights select one input
of 24 random mantissa bits), "onehot" (one-hot inputs select one weight).  tests/test_exact_inputs_host.py checks the method on
the CPU, tests/test_gpu_exact_arithmetic.py runs the kernels; both take their shapes from the lists below."""
import functools

import numpy as np

MODES = ("fp32", "bf16x3", "f16", "bf16")
LOWP = {"bf16x3": 0, "f16": 1, "bf16": 2}                 # mode number of mnc_conv3x3_lowp / mnc_act_pack / mnc_fc_lowp_pair

# ---- shapes (the smallest at which each plan is still reached; none is the workload's own) ----
CONV3 = [(5, 3, 8, 32), (6, 37, 16, 64), (9, 70, 8, 32), (13, 33, 128, 256), (4, 32, 8, 512), (38, 63, 64, 128)]      # H, W, Cin, Cout
WINO4_REDUCE = (37, 63, 256, 512)                         # F(4x4)'s in-launch reduction (five uneven K ranges)
# mnc_conv3x3_wino4_split (conv_wino4_split.hip: the 36 transform positions as ONE batched launch of the LDS-DMA InnerProduct kernel,
# whose rows are the 4x4 tiles): ragged tiles both ways, one K stage | 19 x 17 = 323 tiles = 304 + 19 under the 304-row cut, two
# column tiles | the same cut with 8 K stages (the loop's steady state) and three column tiles | 25 x 25 = 625 tiles: the cut is
# off, 320 + 305 rows, Cout below one column tile | 26 x 26 = 676 tiles: three blocks under the cut, 304 + 304 + 68
WINO4_SPLIT = [(7, 9, 32, 128), (76, 68, 64, 256), (76, 68, 256, 384), (97, 99, 32, 32), (102, 103, 32, 64)]
FC_BATCH = [(323, 384, 256), (625, 96, 32), (676, 130, 64)]            # M, N, K of mnc_fc_batch: the row counts above
LOWP_PLAN = (23, 70, 64, 128)                             # test_conv3x3_lowp_every_plan's shape, plans 0..3
C3 = [(20, 33, 64), (20, 33, 16), (20, 33, 48), (20, 33, 8), (20, 33, 72)]      # H, W, Cout of mnc_conv3x3_c3
# H, W, Cin, Cout, stride, residual: the rows of test_gpu_ops.C11 below the 800 x 1333 ResNet grids (H >= 100)
C11 = [(13, 17, 16, 8, 1, False), (13, 17, 16, 24, 1, True), (20, 33, 32, 72, 2, True), (31, 45, 48, 64, 1, False),
       (31, 45, 80, 160, 2, True), (50, 84, 256, 1024, 1, True)]
# H, W, Cin, Cout, K, stride, pad, residual: test_gpu_ops.GEN_CONV without its two "large grids" rows
GEN = [(37, 53, 64, 256, 1, 1, 0, False), (37, 53, 256, 64, 1, 1, 0, True), (40, 54, 256, 128, 1, 2, 0, False),
       (33, 47, 64, 64, 3, 2, 1, False), (21, 30, 128, 72, 3, 1, 1, True), (12, 9, 8, 8, 5, 1, 2, False), (50, 84, 1024, 256, 1, 1, 0, False)]
STEM = [(31, 45, 3, 1, 1, 32), (64, 64, 7, 2, 3, 64)]     # H, W, K, stride, pad, Cout
# M, N, K, ldc - N
FC = [(45, 150, 64, 0), (37, 130, 512, 0), (321, 128, 512, 0), (300, 126, 8192, 0), (290, 1024, 2112, 0), (300, 520, 4096, 8),
      (640, 512, 8192, 0), (300, 1024, 4096, 0), (120, 512, 4096, 0), (700, 512, 4096, 0)]
FC_DMA = [(300, 520, 4096, 8), (290, 1024, 2112, 0)]      # under FC_TILE=10 with FC_DMA=1 / 0 (test_fc_mfma_lds_dma)
FC_PAIR = [(640, 512, 8192, 0), (300, 1024, 4096, 0), (120, 512, 4096, 0), (700, 512, 4096, 0), (300, 520, 4096, 8)]
# plans of fc_plan.h none of FC reaches (confirmed with the plan shim, test_exact_inputs_host.py): the 256-row blocks of the
# reduced-precision kernels and the paired launches are further down
# (the fp32 160-row block, and the fp32 LDS-DMA kernel with ldc > N: (300, 520, 4096) is below the 2 GFLOP bar of both)
FC_MORE = [(130, 1024, 8192, 0), (300, 520, 8192, 8)]
FC_MIXED = [(300, 1024, 4096, 0), (120, 512, 4096, 0)]    # mnc_fc_lowp_pair with one fp32 and one stage-major input: the issue's shapes ...
FC_PRE = [(300, 1024, 4096, 0), (37, 130, 512, 0), (640, 512, 8192, 0)]
# ... which both plan as two single calls whatever the inputs; the shapes at which mnc_fc_lowp_pair really is ONE launch: several
# 320-row blocks, 256-row blocks (M = 700), one row block (needs >= 8 / 16 stages per K range at 2 x N / 256 column tiles)
FC_LOWP_PAIRED = [(640, 512, 8192, 0), (700, 512, 8192, 0), (290, 2048, 8192, 0)]
FC_WIDE8 = (500, 2048, 8192, 0)                           # a single reduced-precision call on the 256-column kernel with 256-row blocks
FC_WIDE_UNCUT = (300, 2048, 2048, 0)                      # ... and with one row block and NO K ranges (its epilogue writes the result itself)
FC_BIG = [FC_WIDE8, (290, 2048, 8192, 0)]                 # (>= 9 GFLOP: the "int" and split families only)
FCX3_TILE = (300, 520, 4096, 8)                           # the 128-column kernel's 160- / 256- / 320-row builds, forced (FCX3_TILE)


# ---- the rounding rules of x3_split.h ----
def _u(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def bf16_rne(x):
    """x3_rne / v_cvt_pk_bf16_f32: nearest even."""
    u = _u(x).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def bf16_trunc(x):
    return (_u(x) & np.uint32(0xFFFF0000)).view(np.float32)


def split_staged(x):
    """x3_split (activations of the convolutions, mnc_act_pack): hi truncated, lo = x - hi rounded half-up."""
    x = np.ascontiguousarray(x, np.float32)
    h = bf16_trunc(x)
    l = ((_u(x - h).astype(np.uint64) + 0x8000) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return h, l


def split_rne(x):
    """x3_split8_rne / sm_store4 (packed weights, the InnerProducts' activation panels): both terms nearest even."""
    x = np.ascontiguousarray(x, np.float32)
    h = bf16_rne(x)
    return h, bf16_rne(x - h)


def f16_rne(x):
    with np.errstate(over="raise"):
        return np.ascontiguousarray(x, np.float32).astype(np.float16).astype(np.float32)


def terms(mode, x, role):
    """The terms a mode feeds the matrix pipe for operand x; role: "staged" (conv activations), "rows" (InnerProduct activations),
    "weight".  -> (hi, lo) with lo None outside bf16x3."""
    x = np.ascontiguousarray(x, np.float32)
    if mode == "fp32":
        return x, None
    if mode == "f16":
        return f16_rne(x), None
    if mode == "bf16":
        return bf16_rne(x), None
    return split_staged(x) if role == "staged" else split_rne(x)


def operand(mode, x, role):
    """What the pipe multiplies for x: the value after the mode's operand rounding."""
    h, l = terms(mode, x, role)
    return h if l is None else h + l


class Case(object):
    """One exact case.  a: activations ([Cin, H, W] or [M, K]); w: weights (OIHW or [N, K]); b: bias; res: residual or None;
    want: the expected fp32 output before any layout change; bits: headroom in bits (None: single-term families)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---- plain definitions, float64 ----
def conv_f64(x, w, b=None, stride=1, pad=1, res=None, relu=0):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    Cin, H, W = x.shape
    Cout, _, KH, KW = w.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    xp = np.zeros((Cin, H + 2 * pad, W + 2 * pad))
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((Cout, OH, OW))
    for ky in range(KH):
        for kx in range(KW):
            patch = xp[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride]
            y += np.tensordot(w[:, :, ky, kx], patch, axes=(1, 0))
    if b is not None:
        y += np.asarray(b, np.float64)[:, None, None]
    if res is not None:
        y += res
    return np.maximum(y, 0) if relu else y


def fc_f64(a, w, b=None, relu=0):
    y = np.asarray(a, np.float64) @ np.asarray(w, np.float64).T
    if b is not None:
        y += np.asarray(b, np.float64)
    return np.maximum(y, 0) if relu else y


def maxpool2_ceil(y):
    """Pooling MAX 2x2/2 with Caffe's ceil output size on [C, H, W]."""
    C, H, W = y.shape
    p = np.full((C, (H + 1) // 2 * 2, (W + 1) // 2 * 2), -np.inf, y.dtype)
    p[:, :H, :W] = y
    return p.reshape(C, (H + 1) // 2, 2, (W + 1) // 2, 2).max(axis=(2, 4))


def _finish(kind, want64, abs64, unit, what, **kw):
    """Headroom and exactness of the expected output itself, then the Case."""
    peak = float(abs64.max()) / unit
    bits = 24.0 - np.log2(max(peak, 1.0))
    assert peak < 2.0 ** 24, "%s: sum |a||w| reaches 2^%.2f units (headroom %.2f bits)" % (what, np.log2(peak), bits)
    want = want64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64) and np.array_equal(want64 / unit, np.round(want64 / unit)), what
    return Case(kind=kind, want=want, unit=unit, bits=bits, what="%s: headroom %.2f bits" % (what, bits), **kw)


def _representable(mode, x, role, what):
    assert np.array_equal(operand(mode, x, role), np.asarray(x, np.float32)), "%s: an operand is not representable in %s" % (what, mode)


# ---- value generators ----
A_MAX = {"fp32": 4095, "f16": 2047, "bf16": 255, "bf16x3": 255}       # 12 / 11 / 8 significant bits: all the mode's operand holds
                                                                     # (fp32: more than a 2-byte staging path would keep)
W_MAX = 3


def _ints(rng, shape, amax):
    return rng.integers(-amax, amax + 1, size=shape).astype(np.float64)


def _sparse_w(rng, shape, K, per_term, wvals):
    """Weights wvals(shape) thinned so that K_eff * per_term stays below 2^23 units (one bit left for bias and residual): at large K
    the headroom is kept with sparse weights, not with a smaller shape."""
    dens = min(1.0, 2.0 ** 23 / (float(K) * per_term))
    w = wvals(shape)
    if dens < 1.0:
        w = w * (rng.random(shape) < dens)
    return w


def _family_values(rng, family, mode, a_shape, w_shape, K):
    """-> (a, w, unit) as float64 arrays of whole multiples of unit_a / unit_w."""
    ua, uw = 2.0 ** -2, 2.0 ** -3
    if family == "int":
        amax = A_MAX[mode]
        a = _ints(rng, a_shape, amax)
        w = _sparse_w(rng, w_shape, K, amax * W_MAX, lambda s: _ints(rng, s, W_MAX))
    elif family in ("split_a", "split_w", "split_0"):
        assert mode == "bf16x3"
        # the wide operand: 9..16 significant bits (as many as K leaves room for at a density of at least 512 / K), lo != 0
        dens_k = min(K, 512)
        wide_bits = int(min(16, np.floor(np.log2(2.0 ** 23 / (dens_k * W_MAX)))))
        assert wide_bits >= 9
        wide = lambda s: rng.integers(256, 2 ** wide_bits, size=s) * rng.choice([-1.0, 1.0], size=s)
        if family == "split_a":
            a = wide(a_shape)
            w = _sparse_w(rng, w_shape, K, 2 ** wide_bits * W_MAX, lambda s: _ints(rng, s, W_MAX))
        elif family == "split_w":
            a = _ints(rng, a_shape, W_MAX)
            w = _sparse_w(rng, w_shape, K, 2 ** wide_bits * W_MAX, wide)
        else:
            a = _ints(rng, a_shape, 255)
            w = _sparse_w(rng, w_shape, K, 255 * W_MAX, lambda s: _ints(rng, s, W_MAX))
    else:
        raise ValueError(family)
    return a * ua, w * uw, ua * uw


def _check_split(family, a, w, act_role):
    """The split families exercise the product they are named for: lo of the wide operand is not zero, lo of the other is."""
    if not family.startswith("split"):
        return
    la, lw = terms("bf16x3", a, act_role)[1], terms("bf16x3", w, "weight")[1]
    frac = lambda l, v: float((l != 0).sum()) / max(int((np.asarray(v) != 0).sum()), 1)
    assert (frac(la, a) > 0.5) == (family == "split_a") and (family == "split_a" or not la.any()), family
    assert (frac(lw, w) > 0.5) == (family == "split_w") and (family == "split_w" or not lw.any()), family


def _mantissa24(rng, shape):
    """Full 24-bit random mantissas, exponents spread over 2^-10 .. 2^10, signs mixed: normal in fp32 and within fp16's range."""
    m = (rng.integers(0, 2 ** 23, size=shape, dtype=np.uint32) | np.uint32(0x3F800000)).view(np.float32)     # [1, 2)
    v = np.ldexp(m, rng.integers(-10, 11, size=shape).astype(np.int32)) * rng.choice([-1.0, 1.0], size=shape).astype(np.float32)
    return v.astype(np.float32)


# ---- convolutions ----
@functools.lru_cache(maxsize=6)
def conv_case(family, mode, H, W, Cin, Cout, K=3, stride=1, pad=1, residual=False, relu=0, seed=0):
    """Convolution [Cin, H, W] * [Cout, Cin, K, K] (+ bias, + residual, ReLU) for `mode`'s operand forms."""
    rng = np.random.default_rng([seed, H, W, Cin, Cout, K, stride, pad])
    what = "conv %s/%s %dx%d %d->%d k%d s%d" % (family, mode, H, W, Cin, Cout, K, stride)
    a_shape, w_shape = (Cin, H, W), (Cout, Cin, K, K)
    OH, OW = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    if family in ("impulse", "onehot"):
        a, w = np.zeros(a_shape, np.float32), np.zeros(w_shape, np.float32)
        if family == "impulse":                      # one (channel, tap) per output channel carries 1.0
            a = _mantissa24(rng, a_shape)
            w[np.arange(Cout), rng.integers(0, Cin, Cout), rng.integers(0, K, Cout), rng.integers(0, K, Cout)] = 1.0
        else:                                        # a lattice of period K of one-hot pixels (any channel): one term per output
            w = _mantissa24(rng, w_shape)
            ys, xs = np.meshgrid(np.arange(rng.integers(0, K), H, K), np.arange(rng.integers(0, K), W, K), indexing="ij")
            a[rng.integers(0, Cin, ys.shape), ys, xs] = 1.0
        b = np.zeros(Cout, np.float32)
        want64 = conv_f64(operand(mode, a, "staged"), operand(mode, w, "weight"), None, stride, pad)
        nterms = conv_f64(a != 0, w != 0, None, stride, pad)
        assert nterms.max() == 1 and nterms.sum() > 0, what                    # one term per output element, none at some borders
        want = want64.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), want64), what
        return Case(kind="conv", a=a, w=w, b=b, res=None, want=want, relu=0, bits=None, unit=None, what=what, geom=(K, stride, pad))
    a, w, unit = _family_values(rng, family, mode, a_shape, w_shape, Cin * K * K)
    b = _ints(rng, (Cout,), 1000) * unit
    res = _ints(rng, (Cout, OH, OW), 1000) * unit if residual else None
    a32, w32 = a.astype(np.float32), w.astype(np.float32)
    _representable(mode, a32, "staged", what)
    _representable(mode, w32, "weight", what)
    _check_split(family, a32, w32, "staged")
    want64 = conv_f64(a, w, b, stride, pad, res, relu)
    abs64 = conv_f64(np.abs(a), np.abs(w), np.abs(b), stride, pad, None if res is None else np.abs(res))
    return _finish("conv", want64, abs64, unit, what, a=a32, w=w32, b=b.astype(np.float32),
                   res=None if res is None else res.astype(np.float32), relu=relu, geom=(K, stride, pad))


# ---- Winograd: the standard matrices (Lavin & Gray 2015), F(2x2,3x3) and F(4x4,3x3) ----
WINO = {
    2: (np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),
        np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], float),
        np.array([[1, 1, 1, 0], [0, 1, -1, -1]], float)),
    4: (np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]),
        np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], float),
        np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], float))}
WINO_MULT = {2: 4, 4: 576}                            # clears every denominator of G g G^T (4 = 2^2, 576 = 24^2)


def wino_operands(x, w, m, dtype=np.float32):
    """-> U [t*t, Cout, Cin] = G g G^T (evaluated in double and rounded once, as the pack kernels do), V [t*t, Cin, tiles] = B^T d B
    in `dtype`, (tiles_y, tiles_x); t = m + 2."""
    G, Bt, At = WINO[m]
    Cin, H, W = x.shape
    t, TY, TX = m + 2, -(-H // m), -(-W // m)
    U = np.einsum("ia,ocab,jb->ijoc", G, np.asarray(w, np.float64), G).astype(dtype).reshape(t * t, w.shape[0], Cin)
    xp = np.zeros((Cin, m * TY + 2, m * TX + 2), dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    d = np.stack([np.stack([xp[:, i:i + m * TY:m, j:j + m * TX:m] for j in range(t)]) for i in range(t)])      # [t, t, Cin, TY, TX]
    V = np.einsum("ia,abcyx,jb->ijcyx", Bt.astype(dtype), d, Bt.astype(dtype)).astype(dtype).reshape(t * t, Cin, TY * TX)
    return U, V, (TY, TX)


def wino_output(M, m, tiles, H, W, dtype=np.float32):
    """Y = A^T M A per (output channel, tile), assembled and clipped to the image."""
    At = WINO[m][2].astype(dtype)
    t, (TY, TX) = m + 2, tiles
    Y = np.einsum("ia,aboyx,jb->oyixj", At, M.reshape(t, t, -1, TY, TX), At).astype(dtype)
    return Y.reshape(Y.shape[0], TY * m, TX * m)[:, :H, :W]


def wino_f32(x, w, m, order):
    """F(m x m, 3x3) in float32 from the standard matrices with the channel sum in the given order: a list of index arrays, one
    partial sum each, the partial sums added afterwards in list order."""
    U, V, tiles = wino_operands(x.astype(np.float32), w, m)
    M = None
    for idx in order:
        part = np.matmul(U[:, :, idx], V[:, idx, :])
        M = part if M is None else M + part
    return wino_output(M, m, tiles, x.shape[1], x.shape[2])


def dma_k_order(K):
    """The order in which fc_mfma_dma16_kernel adds the K values of one output (gemm.hip): stages of 32, two groups of 16 per stage,
    MFMA q = 0..3 of a group multiplies k = q, 4 + q, 8 + q, 12 + q -- (k0, k4, k8, k12, k1, ...)."""
    assert K % 32 == 0
    return np.array([32 * s + 16 * G + 4 * g + q for s in range(K // 32) for G in range(2) for q in range(4) for g in range(4)])


def batch_row_blocks(M, first=None):
    """fc_batch_launch's row blocks as (first row, rows): 304 rows each (the last 16-row sub-tile of the 320 dropped) when that needs
    no more blocks than 320-row ones, else 320.  first: the distance between the first rows of neighbouring blocks, when it is
    stated apart from the rows a block owns (a defect: the blocks then leave rows out)."""
    step = 304 if -(-M // 304) == -(-M // 320) else 320
    first = step if first is None else first
    return [(b * first, min(M - b * first, step)) for b in range(-(-M // step)) if b * first < M]


def wino4_split_f32(x, w, order, first=None):
    """conv_wino4_split.hip in float32 from the standard matrices: V[p][tile][ci] and U[p][co][ci], M[p][tile][co] filled row block
    by row block (batch_row_blocks; what no block writes stays NaN, as in the NaN-filled workspace of the GPU test), the channel sum
    in the given order (as wino_f32), the output transform.  Without the bias."""
    U, V, tiles = wino_operands(x.astype(np.float32), w, 4)
    M = np.full((36, w.shape[0], V.shape[2]), np.nan, np.float32)
    for m0, rows in batch_row_blocks(V.shape[2], first):
        acc = None
        for idx in order:
            part = np.matmul(U[:, :, idx], V[:, idx, m0:m0 + rows])
            acc = part if acc is None else acc + part
        M[:, :, m0:m0 + rows] = acc
    return wino_output(M, 4, tiles, x.shape[1], x.shape[2])


@functools.lru_cache(maxsize=6)
def wino_case(m, H, W, Cin, Cout, relu=0, seed=0):
    """3x3 convolution whose F(m x m, 3x3) evaluation is exact in fp32: weights WINO_MULT[m] * {-1, 0, 1} * 2^-10 (thinned above 64
    input channels), inputs integers in [-2, 2]
    (F(4x4): [-1, 1], its transforms multiply by up to 8 each way), bias whole multiples of 2^-10."""
    rng = np.random.default_rng([seed, m, H, W, Cin, Cout])
    what = "conv wino F(%dx%d) %dx%d %d->%d" % (m, m, H, W, Cin, Cout)
    unit = 2.0 ** -10
    n = rng.integers(-1, 2, size=(Cout, Cin, 3, 3)) * (rng.random((Cout, Cin, 1, 1)) < min(1.0, 64.0 / Cin))
    w = WINO_MULT[m] * unit * n
    x = _ints(rng, (Cin, H, W), 2 if m == 2 else 1)
    b = _ints(rng, (Cout,), 512) * unit
    U, V, tiles = wino_operands(x, w, m, np.float64)
    assert np.array_equal(U / unit, np.round(U / unit)), what + ": G g G^T is not whole"
    assert np.array_equal(U.astype(np.float32).astype(np.float64), U)
    s_uv = np.matmul(np.abs(U), np.abs(V))                              # sum |U||V| per frequency
    # The output transform of |M|, where M is the sum over ANY contiguous range of 8-channel blocks (the kernels cut the channel
    # sum into K ranges and transform each range's sum on its own): elementwise, the largest |P_j - P_i| over the prefix sums P
    # is max P - min P with P_0 = 0.
    At, t = WINO[m][2], m + 2
    P = np.zeros((t * t, Cout, V.shape[2]))
    hi, lo = P.copy(), P.copy()
    for c0 in range(0, Cin, 8):
        P += np.matmul(U[:, :, c0:c0 + 8], V[:, c0:c0 + 8, :])
        np.maximum(hi, P, out=hi)
        np.minimum(lo, P, out=lo)
    out_abs = np.einsum("ia,aboyx,jb->oyixj", np.abs(At), (hi - lo).reshape(t, t, Cout, *tiles), np.abs(At))
    peak_uv, peak_out = float(s_uv.max()) / unit, float(out_abs.max()) / unit + 512
    bits_uv, bits_out = 24 - np.log2(peak_uv), 24 - np.log2(peak_out)
    assert peak_uv < 2.0 ** 24 and peak_out < 2.0 ** 24, "%s: headroom sum|U||V| %.2f bits, output transform %.2f bits" % (what, bits_uv, bits_out)
    want64 = conv_f64(x, w, b, 1, 1, None, relu)
    abs64 = conv_f64(np.abs(x), np.abs(w), np.abs(b), 1, 1)
    c = _finish("conv", want64, abs64, unit, what, a=x.astype(np.float32), w=w.astype(np.float32), b=b.astype(np.float32), res=None, relu=relu, geom=(3, 1, 1))
    c.bits = min(c.bits, bits_uv, bits_out)
    c.what = "%s: headroom direct %.2f, sum|U||V| %.2f, output transform %.2f bits" % (what, 24 - np.log2(float(abs64.max()) / unit), bits_uv, bits_out)
    return c


# ---- InnerProducts ----
@functools.lru_cache(maxsize=6)
def fc_case(family, mode, M, N, K, relu=0, seed=0):
    """out[M, N] = a[M, K] w[N, K]^T + bias (ReLU) for `mode`'s operand forms."""
    rng = np.random.default_rng([seed, M, N, K])
    what = "fc %s/%s %dx%dx%d" % (family, mode, M, N, K)
    if family in ("impulse", "onehot"):
        a, w = np.zeros((M, K), np.float32), np.zeros((N, K), np.float32)
        if family == "impulse":                      # one k per output column carries 1.0
            a = _mantissa24(rng, (M, K))
            w[np.arange(N), rng.integers(0, K, N)] = 1.0
        else:                                        # a one-hot activation row
            w = _mantissa24(rng, (N, K))
            a[np.arange(M), rng.integers(0, K, M)] = 1.0
        want64 = fc_f64(operand(mode, a, "rows"), operand(mode, w, "weight"))
        want = want64.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), want64) and (fc_f64(a != 0, w != 0) == 1).all(), what
        return Case(kind="fc", a=a, w=w, b=np.zeros(N, np.float32), res=None, want=want, relu=0, bits=None, unit=None, what=what)
    a, w, unit = _family_values(rng, family, mode, (M, K), (N, K), K)
    b = _ints(rng, (N,), 1000) * unit
    a32, w32 = a.astype(np.float32), w.astype(np.float32)
    _representable(mode, a32, "rows", what)
    _representable(mode, a32, "staged", what)
    _representable(mode, w32, "weight", what)
    _check_split(family, a32, w32, "rows")
    return _finish("fc", fc_f64(a, w, b, relu), fc_f64(np.abs(a), np.abs(w), np.abs(b)), unit, what, a=a32, w=w32,
                   b=b.astype(np.float32), res=None, relu=relu)


def families(mode, shape=None):
    """The families an entry point of `mode` runs (the Winograd entries run wino_case alone: their transforms round anything else)."""
    if shape in FC_BIG:
        return ["int"] + (["split_a", "split_w"] if mode == "bf16x3" else [])
    return ["int", "impulse", "onehot"] + (["split_a", "split_w", "split_0"] if mode == "bf16x3" else [])


def same(got, want):
    """The comparison of every exact test: by value (-0.0 == +0.0), nothing else."""
    return np.array_equal(got, want)
