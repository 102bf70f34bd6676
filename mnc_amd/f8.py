"""The numerics of the "f8" math mode, stated in plain numpy (no GPU): OCP e4m3fn codes, one power-of-two scale per row, fp32-class
accumulation.  mnc_amd/csrc/gemm_f8.hip follows this statement bit for bit except for the summation order inside a product: the
statement sums in float64, the device in fp32 in the MFMA's and the K ranges' order.

  codec     e4m3_encode / e4m3_decode: OCP e4m3fn (bias 7, largest finite value 448, subnormals in steps of 2^-9, round to nearest
            even, the sign of zero kept, 0x7F / 0xFF = NaN -- never produced for a finite input: values past 448 saturate).  NOT the
            e4m3fnuz of gfx942 (bias 8, no negative zero): the two are different encodings of the same eight bits.
  rows      quantise_rows: per row amax = max |x| = f * 2^p with f in [0.5, 1) (frexp of the fp32 value); the row's exponent is
            e = p - 9 when f <= 0.875, else p - 8 -- the smallest integer with amax * 2^-e <= 448 -- clamped to [-64, 64], 0 for a zero
            row; codes = e4m3_encode(x * 2^-e).  The scale is a power of two, so scaling and un-scaling are exact and the scaled row's
            maximum lies in (224, 448]: at most one of e4m3's eighteen binades is lost.  Non-finite values take no part in amax
            (a row without a finite non-zero value has e = 0); an infinity then saturates at +-448 and a NaN encodes as NaN.
  product   fc_f8_numpy: acc[m][n] = sum_k dec(qa[m][k]) * dec(qw[n][k]); out = act(ldexp(acc, ea[m] + ew[n]) + bias[n]).
            Weights are quantised per output row once at load, activations per RoI row on every call.
"""
import numpy as np

E4M3_MAX = 448.0
EXP_CLAMP = 64


def e4m3_decode(codes):
    """uint8 codes -> float32 values (0x7F and 0xFF -> NaN)."""
    c = np.asarray(codes, np.uint8).astype(np.int32)
    sign = np.where(c & 0x80, -1.0, 1.0)
    ex, man = (c >> 3) & 15, c & 7
    mag = np.where(ex == 0, man * 2.0 ** -9, (8 + man) * 2.0 ** (ex.astype(np.float64) - 10))
    out = (sign * mag).astype(np.float32)
    out[(c & 0x7F) == 0x7F] = np.nan
    return out


def e4m3_encode(x):
    """float32 values -> uint8 codes, round to nearest even; |x| >= 448 (and infinities) saturate at +-448, NaN -> 0x7F | sign."""
    x = np.ascontiguousarray(x, np.float32)
    bits = x.view(np.uint32)
    sign = ((bits >> 24) & 0x80).astype(np.uint8)
    a = np.abs(x)
    ab = (bits & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    # normal codes: round the 23 mantissa bits to 3 on the fp32 bits (carry into the exponent included), then re-bias 127 -> 7
    rounded = (ab + np.uint32(0x7FFFF) + ((ab >> 20) & np.uint32(1))) >> 20
    normal = rounded.astype(np.int64) - ((127 - 7) << 3)
    # subnormal codes (|x| < 2^-6): multiples of 2^-9; rint rounds ties to even, and 8 is the code of the smallest normal value
    with np.errstate(invalid="ignore"):
        sub = np.rint(a.astype(np.float64) * 512.0)
    code = np.where(a < np.float32(2.0 ** -6), np.nan_to_num(sub), normal)
    code = np.where(a >= np.float32(E4M3_MAX), 0x7E, code)
    code = np.where(np.isnan(x), 0x7F, code)
    return (code.astype(np.uint8) | sign).astype(np.uint8)


def row_exponent(amax):
    """The exponent e of rows whose largest magnitude is amax (float32, >= 0): see the module docstring."""
    amax = np.asarray(amax, np.float32)
    f, p = np.frexp(amax)
    e = np.where(f <= np.float32(0.875), p - 9, p - 8)
    e = np.clip(e, -EXP_CLAMP, EXP_CLAMP)
    return np.where(amax == 0, 0, e).astype(np.int32)


def quantise_rows(x):
    """x [R][K] (fp32, or fp16 values widened) -> (codes uint8 [R][K], e int32 [R])."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2
    mag = np.where(np.isfinite(x), np.abs(x), np.float32(0))          # amax over the finite values only
    amax = mag.max(axis=1) if x.shape[1] else np.zeros(x.shape[0], np.float32)
    e = row_exponent(amax)
    scale = np.ldexp(np.float32(1.0), -e).astype(np.float32)          # 2^-e: a normal fp32 for every e in the clamp
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = (x * scale[:, None]).astype(np.float32)              # exact (a result below fp32's normal range encodes as zero)
    return e4m3_encode(scaled), e


def apply_act(v, act):
    """x3_act of the kernels: 0 none, 1 ReLU, 2 sigmoid."""
    if act == 1:
        return np.maximum(v, 0)
    if act == 2:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def fc_f8_parts(a, w):
    """-> (acc float64 [M][N] of the decoded codes, |acc| bound float64 [M][N] = sum |qa||qw|, ea [M], ew [N])."""
    qa, ea = quantise_rows(a)
    qw, ew = quantise_rows(w)
    da, dw = e4m3_decode(qa).astype(np.float64), e4m3_decode(qw).astype(np.float64)
    return da @ dw.T, np.abs(da) @ np.abs(dw).T, ea, ew


def fc_f8_numpy(a, w, bias, act=0):
    """The InnerProduct of the f8 mode: a [M][K], w [N][K], bias [N] -> float64 [M][N]."""
    acc, _, ea, ew = fc_f8_parts(a, w)
    out = np.ldexp(acc, ea[:, None] + ew[None, :]) + np.asarray(bias, np.float64)[None, :]
    return apply_act(out, act)
