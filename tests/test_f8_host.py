"""CPU: the numerics statement of the "f8" math mode (mnc_amd/f8.py) against torch.float8_e4m3fn and against exact arithmetic, the
launch plan of the e4m3 InnerProduct (mnc_amd/csrc/fc_f8_plan.h, compiled for the host), and the mode's names."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import f8_inputs as F
from mnc_amd import f8

HERE = os.path.dirname(os.path.abspath(__file__))
FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)


def torch_decode(codes):
    import torch
    return torch.from_numpy(np.asarray(codes, np.uint8).copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy()


def torch_encode(x):
    import torch
    return torch.from_numpy(np.asarray(x, np.float32).copy()).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_every_finite_code_decodes_as_torch_does():
    assert len(FINITE) == 254
    got, want = f8.e4m3_decode(FINITE), torch_decode(FINITE)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()          # bits: the sign of zero included
    assert np.abs(got).max() == 448.0 and np.abs(got[got != 0]).min() == 2.0 ** -9
    assert np.isnan(f8.e4m3_decode(np.array([0x7F, 0xFF], np.uint8))).all()


def test_encoding_is_torchs_on_values_midpoints_and_the_ends():
    vals = f8.e4m3_decode(FINITE)
    assert (f8.e4m3_encode(vals) == FINITE).all()                       # every finite value is its own code, -0 included
    pos = np.sort(vals[(FINITE & 0x80) == 0].astype(np.float64))
    mids = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)                # exact in fp32: ties, which must go to even
    for x in (mids, -mids, np.array([448.0, -448.0], np.float32), np.nextafter(mids, np.float32(0)), np.nextafter(mids, np.float32(1e9)),
              -np.nextafter(mids, np.float32(0))):
        got = f8.e4m3_encode(x)
        assert (got == torch_encode(x)).all()
        assert ((got & 0x7F) != 0x7F).all()                             # never NaN for a finite |x| <= 448
    even = f8.e4m3_encode(mids)
    assert (even & 1 == 0).all()
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.uniform(-448, 448, 50000), rng.randn(50000) * np.exp2(rng.randint(-14, 8, 50000))]).astype(np.float32)
    x = x[np.abs(x) <= 448]
    assert (f8.e4m3_encode(x) == torch_encode(x)).all()
    # past 448 the statement saturates (torch: NaN above 464); the row rule never sends it such a value
    assert (f8.e4m3_encode(np.array([449.0, 1e9, np.inf, -500.0], np.float32)) == [0x7E, 0x7E, 0x7E, 0xFE]).all()
    assert (f8.e4m3_encode(np.array([np.nan], np.float32)) & 0x7F == 0x7F).all()


def test_the_scaled_row_maximum_lies_in_224_448():
    j = np.arange(-50, 51)
    base = np.concatenate([np.ldexp(1.0, j), np.ldexp(448.0, j), [7, 224, 448, 449, 3.3, 1e-3]]).astype(np.float32)
    amax = np.concatenate([base, np.nextafter(base, np.float32(0)), np.nextafter(base, np.float32(np.inf))])
    e = f8.row_exponent(amax)
    scaled = np.ldexp(amax.astype(np.float64), -e)
    assert (scaled > 224).all() and (scaled <= 448).all()
    assert (np.ldexp(amax.astype(np.float64), -(e - 1)) > 448).all()    # e is the SMALLEST such integer
    codes, e2 = f8.quantise_rows(amax[:, None])
    assert (e2 == e).all() and ((codes & 0x7F) != 0x7F).all()


def test_exponent_edge_cases():
    assert f8.row_exponent(np.float32(0)) == 0
    codes, e = f8.quantise_rows(np.zeros((2, 128), np.float32))
    assert (e == 0).all() and (codes == 0).all()
    big, tiny = np.float32(3e38), np.float32(1e-38)
    assert f8.row_exponent(big) == 64 and f8.row_exponent(tiny) == -64 and f8.row_exponent(np.float32(1e-45)) == -64
    codes, e = f8.quantise_rows(np.array([[big, -big, 1.0], [tiny, 0.0, -0.0]], np.float32))
    assert list(e) == [64, -64]
    assert list(codes[0]) == [0x7E, 0xFE, 0] and list(codes[1]) == [0, 0, 0x80]      # past the clamp: saturation; -0 keeps its sign
    # non-finite values take no part in amax: inf saturates, NaN stays NaN, the finite values keep the exponent they would have alone
    codes, e = f8.quantise_rows(np.array([[np.inf, 7.0, -np.inf, np.nan], [np.nan, 0.0, np.inf, -0.0]], np.float32))
    assert list(e) == [f8.row_exponent(np.float32(7.0)), 0]
    assert list(codes[0]) == [0x7E, f8.e4m3_encode(np.float32([448.0]))[0], 0xFE, 0x7F] and list(codes[1]) == [0x7F, 0, 0x7E, 0x80]


@pytest.mark.parametrize("M,N,K,identity", [(1, 256, 128, False), (33, 272, 384, False), (33, 441, 384, True), (300, 256, 4480, False)])
def test_the_statement_on_exact_inputs_is_the_integer_product(M, N, K, identity):
    c = F.exact_case(M, N, K, identity=identity, small=K > 1024)
    qa, ea = f8.quantise_rows(c.a)
    qw, ew = f8.quantise_rows(c.w)
    assert (ea == c.ea).all() and (ew == c.ew).all()
    assert (np.ldexp(f8.e4m3_decode(qa).astype(np.float64), ea[:, None]) == c.a).all()       # quantisation is exact
    assert (np.ldexp(f8.e4m3_decode(qw).astype(np.float64), ew[:, None]) == c.w).all()
    assert (f8.fc_f8_numpy(c.a, c.w, c.bias, 0) == c.want).all()
    assert (f8.fc_f8_numpy(c.a, c.w, c.bias, 1) == np.maximum(c.want, 0)).all()


# ---- the plan header ----
HEAD_SHAPES = [(4096, 25088), (4096, 4096), (256, 100352)]              # the large InnerProducts of the full-size net: (N, K)
PLAN_FIELDS = ("mt", "tn", "tm", "splits", "kper", "part_bytes", "q_bytes", "exp_bytes", "in_range", "packed_bytes", "exp_count", "decode")


class Shim(object):
    def __init__(self, so):
        self.lib = lib = ctypes.CDLL(so)
        lib.f8_plan_tune_key.argtypes = [ctypes.c_char_p]
        lib.f8_plan_run.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        lib.f8_plan_run.restype = None

    def plan(self, M, N, K, mstride=None, quantise_here=True, tuning=()):
        t = np.full(self.lib.f8_plan_tune_count(), self.lib.f8_plan_tune_unset(), np.int32)
        for name, value in tuning:
            k = self.lib.f8_plan_tune_key(name.encode())
            assert k >= 0, name
            t[k] = value
        out = np.zeros(len(PLAN_FIELDS), np.int64)
        self.lib.f8_plan_run(t.ctypes.data, M, N, K, M if mstride is None else mstride, int(quantise_here), out.ctypes.data)
        return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("f8plan") / "fc_f8_plan_shim.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "fc_f8_plan_shim.cpp"), "-o", so])
    deps = subprocess.check_output([cxx, "-std=c++17", "-M", os.path.join(HERE, "fc_f8_plan_shim.cpp")]).decode()
    assert "fc_f8_plan.h" in deps and "hip_runtime" not in deps and "/hip/" not in deps and "mnc_internal" not in deps
    return Shim(so)


def up256(b):
    return (b + 255) // 256 * 256


def check_plan(p, M, N, K, quantise_here=True):
    # fewer than four stages: the decoding build (fp16 MFMA), 64-row workgroups, one K range
    assert p["decode"] == (1 if K < 512 else 0) and (not p["decode"] or p["splits"] == 1)
    assert p["mt"] == (2 if M <= 64 or K < 512 else 10)
    assert p["tn"] == -(-N // 256) and p["tm"] == -(-M // (32 * p["mt"]))
    # the K ranges cover K in whole stages: every range but the last holds kper values, the last the rest, none is empty
    assert p["kper"] % 128 == 0 and p["kper"] > 0
    assert p["splits"] == -(-K // p["kper"]) and (p["splits"] - 1) * p["kper"] < K
    assert K - (p["splits"] - 1) * p["kper"] >= 128
    # the scratch the launcher asks for: partial sums | codes | exponents
    assert p["part_bytes"] == (up256(p["splits"] * M * N * 4) if p["splits"] > 1 else 0)
    assert p["q_bytes"] == (up256(M * K) if quantise_here else 0) and p["exp_bytes"] == (up256(4 * M) if quantise_here else 0)
    assert p["packed_bytes"] == p["tn"] * 256 * K and p["exp_count"] == p["tn"] * 256
    assert p["in_range"] == 1


def test_every_product_of_the_full_size_net_gets_a_plan(shim):
    for N, K in HEAD_SHAPES:
        for M in (1, 33, 64, 65, 300, 320, 321, 1000):
            for tuning in ((), (("PLAN", 1),)):
                check_plan(shim.plan(M, N, K, tuning=tuning), M, N, K)
            check_plan(shim.plan(M, N, K, mstride=M + 20, quantise_here=False), M, N, K, quantise_here=False)
    # at 300 RoIs: the single-product rule of the reduced-precision kernels (ranges of >= 2048 K values filling at most half the chip)
    assert [shim.plan(300, N, K)["splits"] for N, K in HEAD_SHAPES] == [8, 2, 49]
    p = shim.plan(300, 4096, 25088)
    assert p["kper"] == 25 * 128 and 25088 - 7 * p["kper"] == 21 * 128          # an uneven last range
    # the cases tests/test_gpu_fc_f8.py reaches the plan's branches with
    assert shim.plan(33, 256, 128)["splits"] == 1 and shim.plan(300, 441, 384)["splits"] == 1
    assert (shim.plan(300, 441, 384)["decode"], shim.plan(300, 441, 384)["tm"]) == (1, 5)
    for M in (33, 300):                                                          # the scaled MFMA with the fused epilogue
        p = shim.plan(M, 441, 512)
        assert (p["decode"], p["splits"], p["mt"]) == (0, 1, 2 if M == 33 else 10)
    assert (shim.plan(300, 256, 4480)["splits"], shim.plan(300, 256, 4480)["kper"]) == (2, 18 * 128)
    assert shim.plan(33, 256, 1024, tuning=(("PLAN", 1),))["splits"] == 2
    assert (shim.plan(321, 256, 1024)["tm"], shim.plan(321, 256, 1024)["splits"]) == (2, 2)
    rng = np.random.RandomState(3)
    for _ in range(2000):
        M, N, K = int(rng.randint(1, 2001)), int(rng.randint(1, 5000)), 128 * int(rng.choice([rng.randint(1, 6), rng.randint(1, 800)]))
        check_plan(shim.plan(M, N, K), M, N, K)
    # a K range whose stages x row stride x 128 bytes pass the copies' 32-bit offset is reported, and the launcher refuses it
    assert shim.plan(300, 256, 128 * 1024 * 128, mstride=300000, quantise_here=False)["in_range"] == 0


def test_mode_names():
    from mnc_amd import engine, native_net
    assert native_net.MATH["f8"] == 5 and sorted(native_net.MATH.values()) == list(range(6))
    assert engine.math_modes("f8") == ("f8", "f16", "f8") and engine.math_modes("F8")[0] == "f8"
    assert engine.math_modes("mixed") == ("mixed", "bf16x3", "f16") and engine.math_modes("fp32") == ("fp32", "fp32", "fp32")
    with pytest.raises(ValueError):
        engine.math_modes("fp8")
    old = os.environ.get("MNC_MATH")
    try:
        os.environ["MNC_MATH"] = "f8"
        assert engine.math_modes(None)[2] == "f8"
    finally:
        if old is None:
            del os.environ["MNC_MATH"]
        else:
            os.environ["MNC_MATH"] = old
