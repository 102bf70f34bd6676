"""Inputs of the f8 tests (tests/test_f8_host.py on the CPU, tests/test_gpu_fc_f8.py on the GPU), made once per shape and shared.

exact_case: operands with exactly one right answer.  Every operand is an integer of at most 4 significant bits (|i| <= 15) times a
power of two of its row, and every row holds a +-14 or a +-15, so the row's exponent is known (14 = 0.875 * 2^4 -> e = p - 5, the codes
are 32 i; 15 = 0.9375 * 2^4 -> e = p - 4, the codes are 16 i) and quantisation is exact.  Every product of two codes is a multiple
of 2^8 and the sum of their magnitudes over a row pair stays below 2^28 (asserted), so every partial sum, in any order, is an fp32
value: the device must return the integer product, bit for bit.  The bias is a multiple of the coarsest output unit of its column,
so adding it is exact too."""
import numpy as np

from mnc_amd import f8


class ExactCase(object):
    pass


def exact_case(M, N, K, seed=0, identity=False, small=False):
    """-> case with a [M][K], w [N][K], bias [N] (all fp32) and want [M][N] float64 = the value before the activation.
    identity: A has one non-zero per row (+-14 or +-15, in varying columns) against an asymmetric W (w[n][k] depends on n and k
    differently), the operand-map check.  small: |i| <= 7 besides the row's 14 / 15 (long K: keeps the sums below 2^28)."""
    rng = np.random.RandomState(1234 + seed)
    c = ExactCase()
    hi = 7 if small else 15
    top = rng.choice([14, 15], size=M) * rng.choice([-1, 1], size=M)
    if identity:
        ia = np.zeros((M, K), np.int64)
        ia[np.arange(M), (np.arange(M) * 37 + 5) % K] = top
        iw = ((np.arange(N)[:, None] * 3 + np.arange(K)[None, :] * 5) % 13 - 6).astype(np.int64)      # asymmetric in (n, k)
    else:
        ia = rng.randint(-hi, hi + 1, size=(M, K)).astype(np.int64)
        ia[np.arange(M), rng.randint(0, K, size=M)] = top
        iw = rng.randint(-hi, hi + 1, size=(N, K)).astype(np.int64)
    iw[np.arange(N), rng.randint(0, K, size=N)] = rng.choice([14, 15], size=N) * rng.choice([-1, 1], size=N)
    pa, pw = rng.randint(-3, 1, size=M), rng.randint(-12, -8, size=N)
    c.a = np.ldexp(ia.astype(np.float64), pa[:, None]).astype(np.float32)
    c.w = np.ldexp(iw.astype(np.float64), pw[:, None]).astype(np.float32)
    # the exponents the row rule must find, and the codes as integers
    c.ea = np.where(np.abs(ia).max(1) == 14, pa - 5, pa - 4).astype(np.int32)
    c.ew = np.where(np.abs(iw).max(1) == 14, pw - 5, pw - 4).astype(np.int32)
    qa = ia << (pa - c.ea)[:, None]
    qw = iw << (pw - c.ew)[:, None]
    assert np.abs(qa).max() <= 448 and np.abs(qw).max() <= 448
    acc = qa @ qw.T
    assert (np.abs(qa) @ np.abs(qw).T).max() < 2 ** 28 and (acc % 256 == 0).all()
    # bias: a small multiple of 2^(8 + max ea + ew[n]), the coarsest unit of the column's sums
    c.bias = np.ldexp(rng.randint(-16, 17, size=N).astype(np.float64), 8 + int(c.ea.max()) + c.ew).astype(np.float32)
    c.want = np.ldexp(acc.astype(np.float64), c.ea[:, None] + c.ew[None, :]) + c.bias.astype(np.float64)[None, :]
    assert (c.want.astype(np.float32).astype(np.float64) == c.want).all()
    return c


def quantiser_rows(M, K, seed=0, fp16=False):
    """[M][K] fp32 rows for the quantiser tests: random rows of widely different magnitudes and, as far as M allows, the special rows
    -- a zero row, a row whose amax sits in the last stage, a row with values far below amax (subnormal codes and zeros), a row of
    ties (scaled values on the midpoints between neighbouring codes), a row of all +-amax.  fp16: every value is an fp16 value."""
    rng = np.random.RandomState(99 + seed)
    x = (rng.randn(M, K) * np.exp2(rng.randint(-10, 8, size=(M, 1)))).astype(np.float32)
    special = []
    special.append(np.zeros(K, np.float32))
    r = (rng.randn(K) * 0.01).astype(np.float32)
    r[K - 3] = 7.5                                                   # amax in the last stage
    special.append(r)
    r = (rng.randn(K) * np.exp2(rng.randint(-20, 0, size=K))).astype(np.float32)
    r[1] = 300.0                                                     # values down to 2^-20 of amax: subnormal codes, zeros
    special.append(r)
    codes = np.arange(0, 127, dtype=np.uint8)                        # ties: the midpoints between neighbouring codes, both signs
    vals = f8.e4m3_decode(codes).astype(np.float64)
    mids = (vals[:-1] + vals[1:]) / 2
    r = np.resize(np.concatenate([mids, -mids]), K).astype(np.float32)
    r[0] = 448.0                                                     # amax = 448 -> e = 0: the values are their own scaled form
    special.append(r * np.float32(0.25))                             # (times a power of two: e = -2, the same codes)
    special.append((rng.choice([-1.0, 1.0], size=K) * 3.3).astype(np.float32))
    for i, r in enumerate(special):
        row = i * 7 if M > 28 else i
        if row < M - 1 or (M == 1 and i == 1):                       # (the last row stays random; one row: the last-stage row)
            x[min(row, M - 1)] = r
    if fp16:
        with np.errstate(over="ignore"):
            x = x.astype(np.float16).astype(np.float32)
    return x


def random_case(M, N, K, seed=0):
    """ReLU'd normal activations, weights 0.01 * normal, a normal bias."""
    rng = np.random.RandomState(7 + seed)
    a = np.maximum(rng.randn(M, K), 0).astype(np.float32)
    w = (0.01 * rng.randn(N, K)).astype(np.float32)
    b = (0.1 * rng.randn(N)).astype(np.float32)
    return a, w, b


def sum_bound(a, w, bias, K):
    """(ref float64 before the activation, per-element bound): |fp32 sum in any order - exact sum| <= 2 K 2^-24 sum |qa||qw|
    (first order: every one of at most K additions rounds a partial sum that is at most sum |qa||qw| to relative 2^-24; the factor 2
    covers the second-order terms for K < 2^20), scaled by 2^(ea + ew), plus one ulp of the result for the rounding of + bias."""
    acc, mag, ea, ew = f8.fc_f8_parts(a, w)
    scale = np.ldexp(1.0, ea[:, None] + ew[None, :])
    ref = acc * scale + np.asarray(bias, np.float64)[None, :]
    bound = 2.0 * K * 2.0 ** -24 * mag * scale + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return ref, bound
