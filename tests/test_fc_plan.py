"""mnc_amd/csrc/fc_plan.h holds the launch plans of the four InnerProduct launchers (mnc_fc, mnc_fc_pair, fc_lowp, fc_lowp_pair) as pure
functions: kernel, tile height, K ranges, block order, scratch bytes.  The number of K ranges fixes how partial sums are grouped, so
a plan is part of the numerical contract.  The header has no HIP include; it is compiled for the host here and held to

  * PLANS (at the end of the file), a literal table of what the launchers planned BEFORE the plans were separated from them: the listing
    profiles/fc_plan_parent.txt, printed by the previous revision's launchers themselves on an MI355X (never by this header), and
  * invariants over that grid and a few thousand random shapes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("head", "two_singles", "small", "kernel", "mt", "sk", "tn", "tm", "tm_arg", "splits", "kper", "slab", "buf", "drop",
          "part_bytes", "conv_bytes")
STAGED, DMA16, X3, WIDE = range(4)
FC, FC_PAIR, LOWP, LOWP_PAIR = range(4)
PRECISIONS = ("fp32", "bf16x3", "f16", "bf16")            # -> FcCall::f16 of the reduced-precision launchers: 0, 1, 2

# (N, K) of every InnerProduct of the graphs the project runs at full width
HEAD_SHAPES = [(4096, 25088), (4096, 4096), (256, 100352), (441, 256), (126, 8192)]     # mnc_5stage test.prototxt (126 = 21 + 21 + 84)
# the resnet50 benchmark configuration (1024-channel trunk: fc6 over 7 x 7 x 1024, fc6_maskest over 14 x 14 x 1024); the CFM test
# graph's InnerProducts (fc6 / fc6_mask 4096 x 25088, fc7 4096 x 4096, fc6_maskest 256 x 100352, mask_pred, the heads) are HEAD_SHAPES
RESNET_SHAPES = [(4096, 50176), (256, 200704)]
SHAPES = HEAD_SHAPES + RESNET_SHAPES
# the row counts at which a decision flips: one or several row blocks, tail <= 160 or > 160, the dropped sub-tile window 289..304,
# 256- against 320-row blocks
ROWS = [1, 160, 161, 288, 289, 304, 305, 320, 321, 480, 481, 640, 760, 960, 1000, 2000]
TUNINGS = [("PLAN", 1), ("FC_TILE", 5), ("FC_TILE", 10), ("FCX3_TILE", 2), ("FCX3_TILE", 5), ("FCX3_TILE", 8), ("FCX3_TILE", 10),
           ("FC_DMA", 0), ("FC_EVEN", 1), ("FC_NOTAIL", 1), ("FC_NO256", 1), ("FC_SPLIT_DIV", 0), ("FC_SPLIT_DIV", 2),
           ("FC_SPLIT_DIV", 21), ("FC_RANGE_K", 4096), ("FC_SLOTS", 64), ("FC_SLOTS", 256), ("FC_ORDER", 0), ("FC_ORDER", 1),
           ("FCX3_WIDE", 0), ("FCX3_WIDE", 1), ("FUSE_SMALL", 0)]
# call variants: name -> (pre-packed activations, second stage-major output, ldc = a * N + b)
VARIANTS = {"plain": (0, 0, 1, 0), "pre": (1, 0, 1, 0), "osm": (0, 1, 1, 0), "pre+osm": (1, 1, 1, 0), "ld2": (0, 0, 2, 0),
            "pre+ld2": (1, 0, 2, 0), "osm+ld2": (0, 1, 2, 0), "pre+osm+ld2": (1, 1, 2, 0), "ld+2": (0, 0, 1, 2)}


# keys only the fp32 launchers read, and keys only the reduced-precision ones read (every other key: all four)
FP32_KEYS, LOWP_KEYS = ("FC_TILE", "FC_DMA", "FC_EVEN"), ("PLAN", "FCX3_TILE", "FC_NO256", "FC_RANGE_K", "FC_SLOTS", "FC_ORDER", "FCX3_WIDE",
                                                         "FUSE_SMALL")


def grid():
    """(precision, pair, variant, tuning or None, M, N, K) of every row of PLANS.  The full row grid runs in all four precisions; the
    call and tuning variants leave out plain bf16 (its plans are fp16's: test_invariants_of_every_plan) and the keys a launcher
    does not read."""
    for prec in PRECISIONS:
        for pair in (0, 1):
            for N, K in SHAPES:
                for M in ROWS:
                    yield prec, pair, "plain", None, M, N, K
            # one product on each side of the 2 GFLOP bar, at M <= 160 and at one 320-row block
            for M, N, K in [(59, 4096, 4096), (60, 4096, 4096), (238, 256, 16384), (239, 256, 16384)]:
                yield prec, pair, "plain", None, M, N, K
            if prec == "bf16":
                continue
            for name in VARIANTS:
                if name == "plain" or (prec == "fp32" and name not in ("ld2", "ld+2")) or (prec != "fp32" and name == "ld+2"):
                    continue
                for N, K in [(4096, 25088), (4096, 4096)]:
                    for M in (300, 640, 1000):
                        yield prec, pair, name, None, M, N, K
            for t in TUNINGS:
                if t[0] in (LOWP_KEYS if prec == "fp32" else FP32_KEYS):
                    continue
                for N, K in [(4096, 25088), (4096, 4096), (256, 100352)]:
                    for M in (300, 760, 1000):
                        yield prec, pair, "plain", t, M, N, K


def key(prec, pair, variant, tuning, M, N, K):
    return "%s %s %s %s %d %d %d" % (prec, "pair" if pair else "single", variant, "%s=%d" % tuning if tuning else "-", M, N, K)


def plan_text(launches):
    """The kernel launches of one call, [(M, plan)], as PLANS writes them: FIELDS kernel .. drop per launch, "M: " in front when there are
    several, "2x" for a pair that runs as two singles with the same launches."""
    parts = [("%d: " % M if len(launches) > 1 else "") + " ".join(str(p[f]) for f in FIELDS[3:14]) for M, p in launches]
    half = len(parts) // 2
    if half and len(parts) % 2 == 0 and parts[:half] == parts[half:]:
        return "2x " + " / ".join(parts[:half])
    return " / ".join(parts)


def encode(texts, sums=None):
    """{grid row: plan_text} -> the lines of PLANS: one per (precisions, single|pair, variant, tuning, N, K), the row counts with one text
    joined, the precisions with the same line joined.  sums ({grid row: str}): a digest of the line's rows is appended (the listing)."""
    import hashlib
    groups = {}
    for r in grid():
        prec, pair, variant, tuning, M, N, K = r
        byprec = groups.setdefault(("pair" if pair else "single", variant, "%s=%d" % tuning if tuning else "-", N, K), {})
        byprec.setdefault(prec, []).append((M, texts[r], sums[r] if sums else ""))
    lines = []
    for gk, byprec in groups.items():
        bodies = {}
        for prec, ent in byprec.items():
            runs = []
            for M, text, _ in ent:
                if runs and runs[-1][1] == text:
                    runs[-1][0].append(M)
                else:
                    runs.append([[M], text])
            bodies.setdefault(" | ".join("%s = %s" % (",".join(map(str, Ms)), text) for Ms, text in runs), []).append(prec)
        for body, precs in bodies.items():
            line = "%s %s %s %s %d %d | %s" % ((",".join(precs),) + gk + (body,))
            if sums:
                line += " # " + hashlib.sha1("\n".join(x for prec in precs for _, _, x in byprec[prec]).encode()).hexdigest()[:12]
            lines.append(line)
    return lines


class Shim(object):
    def __init__(self, so):
        self.lib = lib = ctypes.CDLL(so)
        lib.fc_plan_tune_key.argtypes = [ctypes.c_char_p]
        lib.fc_plan_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.fc_plan_run.restype = None
        self.count, self.unset = lib.fc_plan_tune_count(), lib.fc_plan_tune_unset()

    def tune_array(self, tuning=None):
        t = np.full(self.count, self.unset, np.int32)
        for name, value in ([tuning] if tuning and isinstance(tuning[0], str) else tuning or []):
            k = self.lib.fc_plan_tune_key(name.encode())
            assert k >= 0, name
            t[k] = value
        return t

    def plan(self, which, call, tuning=None, tuning_build=0):
        """call: dict of M, N, K, ldc and, where they are not zero, f16, osm0, osm1, osm_rows, osm_row0, pre0, pre1, mstride,
        defer_reduce, unaligned -> dict of FIELDS."""
        t = self.tune_array(tuning)
        c = np.array([call["M"], call["N"], call["K"], call["ldc"], call.get("f16", 0), call.get("osm0", 0), call.get("osm1", 0),
                      call.get("osm_rows", 0), call.get("osm_row0", 0), call.get("pre0", 0), call.get("pre1", 0), call.get("mstride", 0),
                      call.get("defer_reduce", 0), 0 if call.get("unaligned") else 1], np.int64)
        out = np.zeros(len(FIELDS), np.int64)
        self.lib.fc_plan_run(which, tuning_build, t.ctypes.data, c.ctypes.data, out.ctypes.data)
        return dict(zip(FIELDS, (int(v) for v in out)))

    @staticmethod
    def single_call(call, i):
        """The single call a pair entry point makes for product i when it runs the pair as two singles."""
        return dict(call, osm0=call.get("osm%d" % i, 0), osm1=0, osm_rows=call["M"], osm_row0=0, pre0=call.get("pre%d" % i, 0), pre1=0,
                    mstride=call.get("mstride", 0) if call.get("pre%d" % i, 0) else call["M"])

    def launches(self, which, call, tuning=None, tuning_build=0):
        """The plans of the kernel launches one entry-point call makes, in order, as the launchers carry them out: a plan with head
        rows is the launcher calling itself on the head and on the tail, a pair plan of two singles the two single calls.
        -> [(which, call, plan)]."""
        p = self.plan(which, call, tuning, tuning_build)
        if p["two_singles"]:
            return sum((self.launches(which - 1, self.single_call(call, i), tuning, tuning_build) for i in (0, 1)), [])
        if p["head"]:
            h = p["head"]
            return (self.launches(which, dict(call, M=h), tuning, tuning_build) +
                    self.launches(which, dict(call, M=call["M"] - h, osm_row0=call.get("osm_row0", 0) + h), tuning, tuning_build))
        return [(which, call, p)]

    def text(self, which, call, tuning=None, tuning_build=0):
        return plan_text([(c["M"], p) for _, c, p in self.launches(which, call, tuning, tuning_build)])


def make_call(prec, pair, variant, M, N, K):
    """(which, call) of a grid row, as the entry points mnc_fc / mnc_fc_pair / mnc_fc_<mode>_ex / mnc_fc_lowp_pair pass it on."""
    pre, osm, ld, ld_add = VARIANTS[variant]
    call = {"M": M, "N": N, "K": K, "ldc": ld * N + ld_add}
    if prec == "fp32":
        return (FC_PAIR if pair else FC), call
    call.update(f16=PRECISIONS.index(prec) - 1, pre0=pre, pre1=pre if pair else 0, osm0=osm, osm1=osm if pair else 0, mstride=M)
    if not pair:
        call.update(osm_rows=M)
    return (LOWP_PAIR if pair else LOWP), call


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("fcplan") / "fc_plan_shim.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "fc_plan_shim.cpp"), "-o", so])
    return Shim(so)


def test_the_header_reaches_no_hip_include():
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    deps = subprocess.check_output([cxx, "-std=c++17", "-M", os.path.join(HERE, "fc_plan_shim.cpp")]).decode()
    assert "fc_plan.h" in deps and "tune.h" in deps and "hip_runtime" not in deps and "/hip/" not in deps and "mnc_internal" not in deps


def test_plans_are_those_of_the_launchers_before_the_separation(shim):
    texts = {}
    for r in grid():
        which, call = make_call(r[0], r[1], r[2], *r[4:])
        texts[r] = shim.text(which, call, r[3])
        # without an ablation or superseded-kernel key the tuning build plans what the product build plans
        assert shim.launches(which, call, r[3], 1) == shim.launches(which, call, r[3], 0), key(*r)
    assert len(texts) > 1500
    got, want = encode(texts), PLANS.strip().split("\n")
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # PLANS is the listing of the previous revision: profiles/fc_plan_parent.txt holds a digest of every line of it
    import hashlib
    listed = [l.split(" | ") for l in open(os.path.join(HERE, "..", "profiles", "fc_plan_parent.txt")).read().split("\n") if l and l[0] != "#"]
    assert [(label, d.split()[1]) for label, d, _ in listed] == [(w.split(" | ", 1)[0], hashlib.sha1(w.split(" | ", 1)[1].encode()).hexdigest()[:12])
                                                                 for w in want]


def test_the_plans_the_comments_quote(shim):
    """The sentences of fc_plan.h and DESIGN.md, as assertions (all of these rows are in PLANS too)."""
    fc = lambda M, N, K, **kw: shim.plan(FC, dict(M=M, N=N, K=K, ldc=N), **kw)
    lowp = lambda which, f16, M, N, K, **kw: shim.plan(which, dict(M=M, N=N, K=K, ldc=N, f16=f16, mstride=M, osm_rows=M), **kw)
    # fc6_maskest at 300 rows on the fp32 LDS-DMA kernel: 126 ranges of 25 stages (FC_EVEN=1: rounds 3-5's 121 of 26), last sub-tile dropped
    p = fc(300, 256, 100352)
    assert (p["kernel"], p["mt"], p["splits"], p["kper"], p["slab"], p["buf"], p["drop"]) == (DMA16, 10, 126, 25 * 32, 1, 1, 1)
    p = fc(300, 256, 100352, tuning=("FC_EVEN", 1))
    assert (p["splits"], p["kper"]) == (121, 26 * 32)
    # the f16 fc6 pair: 2 ranges, the fc7 pair: 1, in the throughput plan; the latency plan keeps the full cut
    assert lowp(LOWP_PAIR, 1, 300, 4096, 25088)["splits"] == 2 and lowp(LOWP_PAIR, 1, 300, 4096, 4096)["splits"] == 1
    assert lowp(LOWP_PAIR, 1, 300, 4096, 25088, tuning=("PLAN", 1))["splits"] == 8
    # fc6_maskest in reduced precision: one 256-column tile x 49 ranges of 2048 K values
    p = lowp(LOWP, 1, 300, 256, 100352)
    assert (p["kernel"], p["tn"], p["splits"], p["kper"]) == (WIDE, 1, 49, 2048)
    # M = 1000: 4 x 256-row blocks in one launch; M = 960 and 2000 stay on 320-row blocks
    for f16 in (0, 1, 2):
        p = lowp(LOWP, f16, 1000, 4096, 25088)
        assert (p["head"], p["mt"], p["tm"]) == (0, 8, 4)
        assert lowp(LOWP, f16, 960, 4096, 25088)["mt"] == 10 and lowp(LOWP, f16, 2000, 4096, 25088)["head"] == 1920
    # fp32, M = 760: 640 + 120 as two launches, 2 x 320 + one 160-row block (reduced precision: 3 x 256 rows in one launch)
    p, a, b = fc(760, 4096, 25088), fc(640, 4096, 25088), fc(120, 4096, 25088)
    assert p["head"] == 640 and (a["mt"], a["tm"], b["mt"], b["tm"]) == (10, 2, 5, 1)
    p = lowp(LOWP, 1, 760, 4096, 25088)
    assert (p["head"], p["mt"], p["tm"]) == (0, 8, 3)
    assert fc(760, 4096, 25088, tuning=("FC_NOTAIL", 1))["head"] == 0


def test_what_keeps_an_fp32_pair_two_singles(shim):
    call = dict(M=300, N=4096, K=4096, ldc=4096)
    assert not shim.plan(FC_PAIR, call)["two_singles"]
    for change in (dict(defer_reduce=1), dict(unaligned=1), dict(ldc=4098), dict(N=4094, ldc=4096), dict(M=160), dict(K=4096 + 32),
                   dict(M=760), dict(K=1600000)):      # (the last: 320 rows of K floats beyond the buffer descriptor's range)
        assert shim.plan(FC_PAIR, dict(call, **change))["two_singles"], change
    for t in (("FC_TILE", 10), ("FC_TILE", 5), ("FC_DMA", 0), ("FC_ABL", 0)):
        assert shim.plan(FC_PAIR, call, tuning=t)["two_singles"], t
    # tuning builds: the superseded 32x32x2 kernels leave rows, not slabs, and are never paired; the product build ignores the keys
    for t in (("FC_MFMA16", 0), ("FC_DMA_WAVES", 4), ("FC_DMA_ABL", 1)):
        assert shim.plan(FC, call, tuning=t, tuning_build=1)["slab"] == 0 and shim.plan(FC, call, tuning=t)["slab"] == 1
        assert shim.plan(FC_PAIR, call, tuning=t, tuning_build=1)["two_singles"] and not shim.plan(FC_PAIR, call, tuning=t)["two_singles"]
    assert shim.plan(FC, call, tuning=("FC_DMA_ABL", 16), tuning_build=1)["slab"] == 1
    assert shim.plan(FC_PAIR, call, tuning=("FC_DMA_ABL", 16), tuning_build=1)["two_singles"]


def test_a_mixed_reduced_precision_pair_of_two_row_strides_is_two_singles(shim):
    """One fp32 input and one stage-major input (include/mnc_hip.h: each product takes either form): the paired launch reads both
    panels with one row stride and the panel converted in the launcher has M rows per stage, so a pre-packed panel of m_stride > M
    beside an fp32 one is planned as the two single calls -- in the plan, before anything is enqueued -- and each single keeps its own
    stride.  m_stride == M, or both inputs of one form, stay one launch."""
    for f16 in (0, 1, 2):
        for M, N, K in ((290, 2048, 8192), (300, 4096, 25088), (640, 512, 8192)):
            base = dict(M=M, N=N, K=K, ldc=2 * N, f16=f16)
            for pre in ((1, 0), (0, 1)):
                call = dict(base, pre0=pre[0], pre1=pre[1])
                assert not shim.plan(LOWP_PAIR, dict(call, mstride=M))["two_singles"], (f16, M, pre)
                assert shim.plan(LOWP_PAIR, dict(call, mstride=M + 20))["two_singles"], (f16, M, pre)
                ls = shim.launches(LOWP_PAIR, dict(call, mstride=M + 20))
                assert [(c["pre0"], c["mstride"]) for _, c, _ in ls] == [(pre[0], M + 20 if pre[0] else M), (pre[1], M + 20 if pre[1] else M)]
            assert not shim.plan(LOWP_PAIR, dict(base, pre0=1, pre1=1, mstride=M + 20))["two_singles"]
            assert not shim.plan(LOWP_PAIR, dict(base, mstride=0))["two_singles"]


def _shapes():
    for r in grid():
        yield r
    rng = np.random.default_rng(7)
    for i in range(3000):
        M = int(rng.choice([rng.integers(1, 2200), rng.choice(ROWS)]))
        N = int(rng.choice([rng.integers(1, 5000), 256 * rng.integers(1, 17), 128 * rng.integers(1, 33)]))
        K = 64 * int(rng.choice([rng.integers(1, 64), rng.integers(1, 3200)]))
        t = TUNINGS[int(rng.integers(len(TUNINGS)))] if rng.random() < 0.5 else None
        yield PRECISIONS[i % 4], (i // 4) % 2, list(VARIANTS)[int(rng.integers(len(VARIANTS)))], t, M, N, K


def test_invariants_of_every_plan(shim):
    cdiv = lambda a, b: -(-a // b)
    up256 = lambda b: cdiv(b, 256) * 256
    n = 0
    for r in _shapes():
        prec, pair, variant, tuning, M, N, K = r
        which, call = make_call(prec, pair, variant, M, N, K)
        if prec == "bf16":                             # plain bf16 plans as fp16 does
            assert shim.launches(which, call, tuning) == [(w, dict(c, f16=2), p) for w, c, p in shim.launches(which, dict(call, f16=1), tuning)], r
        if tuning and tuning[0] in (LOWP_KEYS if prec == "fp32" else FP32_KEYS):      # a key the launcher does not read
            assert shim.launches(which, call, tuning) == shim.launches(which, call), r
        for tb in (0, 1):
            p = shim.plan(which, call, tuning, tb)
            single = shim.plan(which - 1, shim.single_call(call, 0), tuning, tb) if pair else None
            if p["two_singles"]:                       # precisely the two single plans
                singles = [shim.launches(which - 1, shim.single_call(call, i), tuning, tb) for i in (0, 1)]
                assert shim.launches(which, call, tuning, tb) == singles[0] + singles[1] and singles[0] and singles[1], r
                continue
            if p["head"]:                              # head rows + tail rows = M, the head a multiple of 320
                assert not pair and 0 < p["head"] < M and p["head"] % 320 == 0 and M - p["head"] <= 160, r
                continue
            n += 1
            assert p["splits"] >= 1 and p["kper"] % p["sk"] == 0 and cdiv(K, p["kper"]) == p["splits"], r
            assert p["tm"] == cdiv(M, 32 * p["mt"]) and abs(p["tm_arg"]) == p["tm"], r
            width = 256 if p["kernel"] == WIDE else 128
            assert p["tn"] == (2 if pair else 1) * cdiv(N, width), r
            if pair:                                   # twice the column tiles of the kernel family; where the single plan is of it too, of that plan
                assert p["kernel"] in (DMA16, WIDE) and (single["kernel"] != p["kernel"] or single["head"] or p["tn"] == 2 * single["tn"]), r
                assert prec != "fp32" or (single["kernel"] == DMA16 and not single["head"] and single["buf"]), r
            want = 0
            if p["splits"] > 1:
                want = p["tn"] * p["tm"] * p["splits"] * 163840 if p["slab"] else (2 if pair else 1) * p["splits"] * M * N * 4
                if prec != "fp32":
                    want = up256(want)
            assert p["part_bytes"] == want, r
            assert p["slab"] == (p["kernel"] == DMA16 and not (tb and p["slab"] == 0)), r
            stages = K // p["sk"]
            if p["kernel"] == WIDE:                    # a stage of the activations within the 32-bit scalar offset
                assert stages * (call["mstride"] if call["pre0"] or call["pre1"] else M) * 128 < 4e9 and N % 256 == 0, r
            assert not p["buf"] or (p["kernel"] == DMA16 and 320 * K * 4 < 1.8e9), r
            assert p["drop"] == (1 if p["kernel"] == DMA16 and p["tm"] == 1 and 288 < M <= 304 else 0), r
    assert n > 4000
    # beyond the grid: the two address-range bars (the shapes exist only as plans)
    big = dict(M=300, N=512, K=1600000, ldc=512)
    assert 320 * big["K"] * 4 >= 1.8e9 and shim.plan(FC, big)["kernel"] == DMA16 and shim.plan(FC, big)["buf"] == 0
    far = dict(M=300, N=512, K=64 * 400000, ldc=512, f16=1, pre0=1, mstride=300)
    assert shim.plan(LOWP, dict(far, K=64 * 4096))["kernel"] == WIDE and shim.plan(LOWP, far)["kernel"] == X3



# What the launchers of the previous revision planned: their own PLAN lines on an MI355X (profiles/fc_plan_parent.txt says how they were
# made and holds a digest of every line), grouped by encode().  A plan is FIELDS kernel .. drop:
#   kernel (0 fc_mfma_kernel, 1 fc_mfma_dma16_kernel, 2 fc_x3_kernel, 3 fc_lowp_dma_kernel) mt sk tn tm tm_arg splits kper slab buf drop
PLANS = """
fp32 single plain - 4096 25088 | 1 = 0 2 32 32 1 1 16 1568 0 0 0 | 160 = 0 5 16 32 1 1 16 1568 0 0 0 | 161,288 = 1 10 32 32 1 1 8 3136 1 1 0 | 289,304 = 1 10 32 32 1 1 8 3136 1 1 1 | 305,320 = 1 10 32 32 1 1 8 3136 1 1 0 | 321 = 320: 1 10 32 32 1 1 8 3136 1 1 0 / 1: 0 2 32 32 1 1 16 1568 0 0 0 | 480 = 320: 1 10 32 32 1 1 8 3136 1 1 0 / 160: 0 5 16 32 1 1 16 1568 0 0 0 | 481,640 = 1 10 32 32 2 2 4 6272 1 1 0 | 760 = 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 960 = 1 10 32 32 3 3 8 3136 1 1 0 | 1000 = 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0 | 2000 = 1920: 1 10 32 32 6 6 4 6272 1 1 0 / 80: 0 5 16 32 1 1 16 1568 0 0 0
bf16x3 single plain - 4096 25088 | 1 = 2 2 32 32 1 1 16 1568 0 0 0 | 160 = 2 5 32 32 1 1 4 6272 0 0 0 | 161,288,289,304,305,320 = 3 10 32 16 1 1 8 3136 0 0 0 | 321 = 320: 3 10 32 16 1 1 8 3136 0 0 0 / 1: 2 2 32 32 1 1 16 1568 0 0 0 | 480 = 320: 3 10 32 16 1 1 8 3136 0 0 0 / 160: 2 5 32 32 1 1 4 6272 0 0 0 | 481 = 3 8 32 16 2 -2 4 6272 0 0 0 | 640 = 3 10 32 16 2 -2 4 6272 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 960 = 3 10 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0 | 2000 = 1920: 3 10 32 16 6 -6 4 6272 0 0 0 / 80: 2 5 32 32 1 1 4 6272 0 0 0
f16,bf16 single plain - 4096 25088 | 1 = 2 2 64 32 1 1 16 1600 0 0 0 | 160 = 2 5 64 32 1 1 4 6272 0 0 0 | 161,288,289,304,305,320 = 3 10 64 16 1 1 8 3136 0 0 0 | 321 = 320: 3 10 64 16 1 1 8 3136 0 0 0 / 1: 2 2 64 32 1 1 16 1600 0 0 0 | 480 = 320: 3 10 64 16 1 1 8 3136 0 0 0 / 160: 2 5 64 32 1 1 4 6272 0 0 0 | 481 = 3 8 64 16 2 -2 4 6272 0 0 0 | 640 = 3 10 64 16 2 -2 4 6272 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 960 = 3 10 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0 | 2000 = 1920: 3 10 64 16 6 -6 4 6272 0 0 0 / 80: 2 5 64 32 1 1 4 6272 0 0 0
fp32 single plain - 4096 4096 | 1 = 0 2 32 32 1 1 16 256 0 0 0 | 160 = 0 5 16 32 1 1 16 256 0 0 0 | 161,288 = 1 10 32 32 1 1 8 512 1 1 0 | 289,304 = 1 10 32 32 1 1 8 512 1 1 1 | 305,320 = 1 10 32 32 1 1 8 512 1 1 0 | 321 = 320: 1 10 32 32 1 1 8 512 1 1 0 / 1: 0 2 32 32 1 1 16 256 0 0 0 | 480 = 320: 1 10 32 32 1 1 8 512 1 1 0 / 160: 0 5 16 32 1 1 16 256 0 0 0 | 481,640 = 1 10 32 32 2 2 4 1024 1 1 0 | 760 = 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 960 = 1 10 32 32 3 3 5 832 1 1 0 | 1000 = 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0 | 2000 = 1920: 1 10 32 32 6 6 4 1024 1 1 0 / 80: 0 5 16 32 1 1 16 256 0 0 0 | 59 = 0 2 32 32 1 1 16 256 0 0 0 | 60 = 0 5 16 32 1 1 16 256 0 0 0
bf16x3 single plain - 4096 4096 | 1 = 2 2 32 32 1 1 16 256 0 0 0 | 160 = 2 5 32 32 1 1 2 2048 0 0 0 | 161,288,289,304,305,320 = 3 10 32 16 1 1 2 2048 0 0 0 | 321 = 320: 3 10 32 16 1 1 2 2048 0 0 0 / 1: 2 2 32 32 1 1 16 256 0 0 0 | 480 = 320: 3 10 32 16 1 1 2 2048 0 0 0 / 160: 2 5 32 32 1 1 2 2048 0 0 0 | 481 = 3 8 32 16 2 -2 4 1024 0 0 0 | 640 = 2 5 32 32 4 -4 1 4096 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 960 = 2 5 32 32 6 -6 2 2048 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0 | 2000 = 1920: 3 10 32 16 6 -6 4 1024 0 0 0 / 80: 2 5 32 32 1 1 2 2048 0 0 0 | 59 = 2 2 32 32 1 1 16 256 0 0 0 | 60 = 2 5 32 32 1 1 2 2048 0 0 0
f16,bf16 single plain - 4096 4096 | 1 = 2 2 64 32 1 1 16 256 0 0 0 | 160 = 2 5 64 32 1 1 2 2048 0 0 0 | 161,288,289,304,305,320 = 3 10 64 16 1 1 2 2048 0 0 0 | 321 = 320: 3 10 64 16 1 1 2 2048 0 0 0 / 1: 2 2 64 32 1 1 16 256 0 0 0 | 480 = 320: 3 10 64 16 1 1 2 2048 0 0 0 / 160: 2 5 64 32 1 1 2 2048 0 0 0 | 481 = 3 8 64 16 2 -2 4 1024 0 0 0 | 640 = 2 5 64 32 4 -4 1 4096 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 960 = 2 5 64 32 6 -6 2 2048 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0 | 2000 = 1920: 3 10 64 16 6 -6 1 4096 0 0 0 / 80: 2 5 64 32 1 1 2 2048 0 0 0 | 59 = 2 2 64 32 1 1 16 256 0 0 0 | 60 = 2 5 64 32 1 1 2 2048 0 0 0
fp32 single plain - 256 100352 | 1 = 0 2 32 2 1 1 242 416 0 0 0 | 160 = 0 5 16 2 1 1 251 400 0 0 0 | 161,288 = 1 10 32 2 1 1 126 800 1 1 0 | 289,304 = 1 10 32 2 1 1 126 800 1 1 1 | 305,320 = 1 10 32 2 1 1 126 800 1 1 0 | 321 = 320: 1 10 32 2 1 1 126 800 1 1 0 / 1: 0 2 32 2 1 1 242 416 0 0 0 | 480 = 320: 1 10 32 2 1 1 126 800 1 1 0 / 160: 0 5 16 2 1 1 251 400 0 0 0 | 481,640 = 1 10 32 2 2 2 64 1568 1 1 0 | 760 = 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 960 = 1 10 32 2 3 3 42 2400 1 1 0 | 1000 = 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 0 5 16 2 1 1 251 400 0 0 0 | 2000 = 1920: 1 10 32 2 6 6 21 4800 1 1 0 / 80: 0 5 16 2 1 1 251 400 0 0 0
bf16x3 single plain - 256 100352 | 1 = 2 2 32 2 1 1 242 416 0 0 0 | 160 = 2 5 32 2 1 1 49 2048 0 0 0 | 161,288,289,304,305,320 = 3 10 32 1 1 1 49 2048 0 0 0 | 321 = 320: 3 10 32 1 1 1 49 2048 0 0 0 / 1: 2 2 32 2 1 1 242 416 0 0 0 | 480 = 320: 3 10 32 1 1 1 49 2048 0 0 0 / 160: 2 5 32 2 1 1 49 2048 0 0 0 | 481 = 3 8 32 1 2 2 64 1568 0 0 0 | 640 = 2 5 32 2 4 4 16 6272 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 960 = 3 10 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0 | 2000 = 1920: 3 10 32 1 6 6 21 4800 0 0 0 / 80: 2 5 32 2 1 1 49 2048 0 0 0
f16,bf16 single plain - 256 100352 | 1 = 2 2 64 2 1 1 224 448 0 0 0 | 160 = 2 5 64 2 1 1 49 2048 0 0 0 | 161,288,289,304,305,320 = 3 10 64 1 1 1 49 2048 0 0 0 | 321 = 320: 3 10 64 1 1 1 49 2048 0 0 0 / 1: 2 2 64 2 1 1 224 448 0 0 0 | 480 = 320: 3 10 64 1 1 1 49 2048 0 0 0 / 160: 2 5 64 2 1 1 49 2048 0 0 0 | 481 = 3 8 64 1 2 2 63 1600 0 0 0 | 640 = 2 5 64 2 4 4 16 6272 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 960 = 3 10 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0 | 2000 = 1920: 3 10 64 1 6 6 21 4800 0 0 0 / 80: 2 5 64 2 1 1 49 2048 0 0 0
fp32 single plain - 441 256 | 1 = 0 2 32 4 1 1 1 256 0 0 0 | 160,161 = 0 2 32 4 3 3 1 256 0 0 0 | 288,289,304,305,320 = 0 2 32 4 5 5 1 256 0 0 0 | 321 = 0 2 32 4 6 6 1 256 0 0 0 | 480,481 = 0 2 32 4 8 8 1 256 0 0 0 | 640 = 0 2 32 4 10 10 1 256 0 0 0 | 760 = 0 2 32 4 12 12 1 256 0 0 0 | 960 = 0 2 32 4 15 15 1 256 0 0 0 | 1000 = 0 2 32 4 16 16 1 256 0 0 0 | 2000 = 0 2 32 4 32 32 1 256 0 0 0
bf16x3 single plain - 441 256 | 1 = 2 2 32 4 1 1 4 64 0 0 0 | 160,161 = 2 2 32 4 3 3 4 64 0 0 0 | 288,289,304,305,320 = 2 2 32 4 5 5 4 64 0 0 0 | 321 = 2 2 32 4 6 6 4 64 0 0 0 | 480,481 = 2 2 32 4 8 8 4 64 0 0 0 | 640 = 2 2 32 4 10 10 4 64 0 0 0 | 760 = 2 2 32 4 12 12 4 64 0 0 0 | 960 = 2 2 32 4 15 15 4 64 0 0 0 | 1000 = 2 2 32 4 16 16 4 64 0 0 0 | 2000 = 2 2 32 4 32 32 4 64 0 0 0
f16,bf16 single plain - 441 256 | 1 = 2 2 64 4 1 1 4 64 0 0 0 | 160,161 = 2 2 64 4 3 3 4 64 0 0 0 | 288,289,304,305,320 = 2 2 64 4 5 5 4 64 0 0 0 | 321 = 2 2 64 4 6 6 4 64 0 0 0 | 480,481 = 2 2 64 4 8 8 4 64 0 0 0 | 640 = 2 2 64 4 10 10 4 64 0 0 0 | 760 = 2 2 64 4 12 12 4 64 0 0 0 | 960 = 2 2 64 4 15 15 4 64 0 0 0 | 1000 = 2 2 64 4 16 16 4 64 0 0 0 | 2000 = 2 2 64 4 32 32 4 64 0 0 0
fp32 single plain - 126 8192 | 1 = 0 2 32 1 1 1 32 256 0 0 0 | 160,161 = 0 2 32 1 3 3 32 256 0 0 0 | 288,289,304,305,320 = 0 2 32 1 5 5 32 256 0 0 0 | 321 = 0 2 32 1 6 6 32 256 0 0 0 | 480,481 = 0 2 32 1 8 8 32 256 0 0 0 | 640 = 0 2 32 1 10 10 32 256 0 0 0 | 760 = 0 2 32 1 12 12 32 256 0 0 0 | 960 = 0 2 32 1 15 15 32 256 0 0 0 | 1000 = 960: 0 2 32 1 15 15 32 256 0 0 0 / 40: 0 2 32 1 1 1 32 256 0 0 0 | 2000 = 1920: 1 10 32 1 6 6 32 256 1 1 0 / 80: 0 2 32 1 2 2 32 256 0 0 0
bf16x3 single plain - 126 8192 | 1 = 2 2 32 1 1 1 128 64 0 0 0 | 160,161 = 2 2 32 1 3 3 128 64 0 0 0 | 288,289,304,305,320 = 2 2 32 1 5 5 86 96 0 0 0 | 321 = 2 2 32 1 6 6 86 96 0 0 0 | 480,481 = 2 2 32 1 8 8 64 128 0 0 0 | 640 = 2 2 32 1 10 10 52 160 0 0 0 | 760 = 2 2 32 1 12 12 43 192 0 0 0 | 960 = 2 2 32 1 15 15 32 256 0 0 0 | 1000 = 2 8 32 1 4 4 32 256 0 0 0 | 2000 = 1920: 2 5 32 1 12 12 10 832 0 0 0 / 80: 2 2 32 1 2 2 128 64 0 0 0
f16,bf16 single plain - 126 8192 | 1 = 2 2 64 1 1 1 128 64 0 0 0 | 160,161 = 2 2 64 1 3 3 128 64 0 0 0 | 288,289,304,305,320 = 2 2 64 1 5 5 64 128 0 0 0 | 321 = 2 2 64 1 6 6 64 128 0 0 0 | 480,481 = 2 2 64 1 8 8 64 128 0 0 0 | 640 = 2 2 64 1 10 10 43 192 0 0 0 | 760 = 2 2 64 1 12 12 43 192 0 0 0 | 960 = 2 2 64 1 15 15 32 256 0 0 0 | 1000 = 2 8 64 1 4 4 32 256 0 0 0 | 2000 = 1920: 2 5 64 1 12 12 10 832 0 0 0 / 80: 2 2 64 1 2 2 128 64 0 0 0
fp32 single plain - 4096 50176 | 1 = 0 2 32 32 1 1 16 3136 0 0 0 | 160 = 0 5 16 32 1 1 16 3136 0 0 0 | 161,288 = 1 10 32 32 1 1 8 6272 1 1 0 | 289,304 = 1 10 32 32 1 1 8 6272 1 1 1 | 305,320 = 1 10 32 32 1 1 8 6272 1 1 0 | 321 = 320: 1 10 32 32 1 1 8 6272 1 1 0 / 1: 0 2 32 32 1 1 16 3136 0 0 0 | 480 = 320: 1 10 32 32 1 1 8 6272 1 1 0 / 160: 0 5 16 32 1 1 16 3136 0 0 0 | 481,640 = 1 10 32 32 2 2 4 12544 1 1 0 | 760 = 640: 1 10 32 32 2 2 4 12544 1 1 0 / 120: 0 5 16 32 1 1 16 3136 0 0 0 | 960 = 1 10 32 32 3 3 8 6272 1 1 0 | 1000 = 960: 1 10 32 32 3 3 8 6272 1 1 0 / 40: 0 5 16 32 1 1 16 3136 0 0 0 | 2000 = 1920: 1 10 32 32 6 6 4 12544 1 1 0 / 80: 0 5 16 32 1 1 16 3136 0 0 0
bf16x3 single plain - 4096 50176 | 1 = 2 2 32 32 1 1 16 3136 0 0 0 | 160 = 2 5 32 32 1 1 4 12544 0 0 0 | 161,288,289,304,305,320 = 3 10 32 16 1 1 8 6272 0 0 0 | 321 = 320: 3 10 32 16 1 1 8 6272 0 0 0 / 1: 2 2 32 32 1 1 16 3136 0 0 0 | 480 = 320: 3 10 32 16 1 1 8 6272 0 0 0 / 160: 2 5 32 32 1 1 4 12544 0 0 0 | 481 = 3 8 32 16 2 -2 4 12544 0 0 0 | 640 = 3 10 32 16 2 -2 4 12544 0 0 0 | 760 = 3 8 32 16 3 -3 8 6272 0 0 0 | 960 = 3 10 32 16 3 -3 8 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 2 25088 0 0 0 | 2000 = 1920: 3 10 32 16 6 -6 4 12544 0 0 0 / 80: 2 5 32 32 1 1 4 12544 0 0 0
f16,bf16 single plain - 4096 50176 | 1 = 2 2 64 32 1 1 16 3136 0 0 0 | 160 = 2 5 64 32 1 1 4 12544 0 0 0 | 161,288,289,304,305,320 = 3 10 64 16 1 1 8 6272 0 0 0 | 321 = 320: 3 10 64 16 1 1 8 6272 0 0 0 / 1: 2 2 64 32 1 1 16 3136 0 0 0 | 480 = 320: 3 10 64 16 1 1 8 6272 0 0 0 / 160: 2 5 64 32 1 1 4 12544 0 0 0 | 481 = 3 8 64 16 2 -2 4 12544 0 0 0 | 640 = 3 10 64 16 2 -2 4 12544 0 0 0 | 760 = 3 8 64 16 3 -3 8 6272 0 0 0 | 960 = 3 10 64 16 3 -3 8 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 2 25088 0 0 0 | 2000 = 1920: 3 10 64 16 6 -6 4 12544 0 0 0 / 80: 2 5 64 32 1 1 4 12544 0 0 0
fp32 single plain - 256 200704 | 1 = 0 2 32 2 1 1 251 800 0 0 0 | 160 = 0 5 16 2 1 1 256 784 0 0 0 | 161,288 = 1 10 32 2 1 1 128 1568 1 1 0 | 289,304 = 1 10 32 2 1 1 128 1568 1 1 1 | 305,320 = 1 10 32 2 1 1 128 1568 1 1 0 | 321 = 320: 1 10 32 2 1 1 128 1568 1 1 0 / 1: 0 2 32 2 1 1 251 800 0 0 0 | 480 = 320: 1 10 32 2 1 1 128 1568 1 1 0 / 160: 0 5 16 2 1 1 256 784 0 0 0 | 481,640 = 1 10 32 2 2 2 64 3136 1 1 0 | 760 = 640: 1 10 32 2 2 2 64 3136 1 1 0 / 120: 0 5 16 2 1 1 256 784 0 0 0 | 960 = 1 10 32 2 3 3 42 4800 1 1 0 | 1000 = 960: 1 10 32 2 3 3 42 4800 1 1 0 / 40: 0 5 16 2 1 1 256 784 0 0 0 | 2000 = 1920: 1 10 32 2 6 6 21 9568 1 1 0 / 80: 0 5 16 2 1 1 256 784 0 0 0
bf16x3 single plain - 256 200704 | 1 = 2 2 32 2 1 1 251 800 0 0 0 | 160 = 2 5 32 2 1 1 64 3136 0 0 0 | 161,288,289,304,305,320 = 3 10 32 1 1 1 98 2048 0 0 0 | 321 = 320: 3 10 32 1 1 1 98 2048 0 0 0 / 1: 2 2 32 2 1 1 251 800 0 0 0 | 480 = 320: 3 10 32 1 1 1 98 2048 0 0 0 / 160: 2 5 32 2 1 1 64 3136 0 0 0 | 481 = 3 8 32 1 2 2 64 3136 0 0 0 | 640 = 3 10 32 1 2 2 64 3136 0 0 0 | 760 = 3 8 32 1 3 3 42 4800 0 0 0 | 960 = 3 10 32 1 3 3 42 4800 0 0 0 | 1000 = 3 8 32 1 4 4 32 6272 0 0 0 | 2000 = 1920: 3 10 32 1 6 6 21 9568 0 0 0 / 80: 2 5 32 2 1 1 64 3136 0 0 0
f16,bf16 single plain - 256 200704 | 1 = 2 2 64 2 1 1 242 832 0 0 0 | 160 = 2 5 64 2 1 1 64 3136 0 0 0 | 161,288,289,304,305,320 = 3 10 64 1 1 1 98 2048 0 0 0 | 321 = 320: 3 10 64 1 1 1 98 2048 0 0 0 / 1: 2 2 64 2 1 1 242 832 0 0 0 | 480 = 320: 3 10 64 1 1 1 98 2048 0 0 0 / 160: 2 5 64 2 1 1 64 3136 0 0 0 | 481 = 3 8 64 1 2 2 64 3136 0 0 0 | 640 = 3 10 64 1 2 2 64 3136 0 0 0 | 760 = 3 8 64 1 3 3 42 4800 0 0 0 | 960 = 3 10 64 1 3 3 42 4800 0 0 0 | 1000 = 3 8 64 1 4 4 32 6272 0 0 0 | 2000 = 1920: 3 10 64 1 6 6 21 9600 0 0 0 / 80: 2 5 64 2 1 1 64 3136 0 0 0
fp32 single plain - 256 16384 | 238 = 0 2 32 2 4 4 64 256 0 0 0 | 239 = 1 10 32 2 1 1 64 256 1 1 0
bf16x3 single plain - 256 16384 | 238 = 2 2 32 2 4 4 64 256 0 0 0 | 239 = 3 10 32 1 1 1 8 2048 0 0 0
f16,bf16 single plain - 256 16384 | 238 = 2 2 64 2 4 4 64 256 0 0 0 | 239 = 3 10 64 1 1 1 8 2048 0 0 0
fp32 single ld2 - 4096 25088 | 300 = 1 10 32 32 1 1 8 3136 1 1 1 | 640 = 1 10 32 32 2 2 4 6272 1 1 0 | 1000 = 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
bf16x3 single ld2 - 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 640 = 3 10 32 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single ld2 - 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 640 = 3 10 64 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
fp32 single ld2 - 4096 4096 | 300 = 1 10 32 32 1 1 8 512 1 1 1 | 640 = 1 10 32 32 2 2 4 1024 1 1 0 | 1000 = 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
bf16x3 single ld2 - 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 640 = 2 5 32 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single ld2 - 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 640 = 2 5 64 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
fp32 single ld+2 - 4096 25088 | 300 = 1 10 32 32 1 1 8 3136 1 1 1 | 640 = 1 10 32 32 2 2 4 6272 1 1 0 | 1000 = 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
fp32 single ld+2 - 4096 4096 | 300 = 1 10 32 32 1 1 8 512 1 1 1 | 640 = 1 10 32 32 2 2 4 1024 1 1 0 | 1000 = 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 single plain FC_TILE=5 4096 25088 | 300 = 0 5 16 32 2 2 8 3136 0 0 0 | 760 = 640: 0 5 16 32 4 4 4 6272 0 0 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 960: 0 5 16 32 6 6 8 3136 0 0 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
fp32 single plain FC_TILE=5 4096 4096 | 300 = 0 5 16 32 2 2 8 512 0 0 0 | 760 = 640: 0 5 16 32 4 4 4 1024 0 0 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 1000 = 960: 0 5 16 32 6 6 5 832 0 0 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 single plain FC_TILE=5 256 100352 | 300 = 0 5 16 2 2 2 128 784 0 0 0 | 760 = 640: 0 5 16 2 4 4 64 1568 0 0 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 960: 0 5 16 2 6 6 42 2400 0 0 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
fp32 single plain FC_TILE=10 4096 25088 | 300 = 1 10 32 32 1 1 8 3136 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 1 10 32 32 1 1 8 3136 1 1 0 | 1000 = 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 1 10 32 32 1 1 8 3136 1 1 0
fp32 single plain FC_TILE=10 4096 4096 | 300 = 1 10 32 32 1 1 8 512 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 1 10 32 32 1 1 8 512 1 1 0 | 1000 = 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 single plain FC_TILE=10 256 100352 | 300 = 1 10 32 2 1 1 126 800 1 1 1 | 760 = 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 1 10 32 2 1 1 126 800 1 1 0 | 1000 = 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 1 10 32 2 1 1 126 800 1 1 0
fp32 single plain FC_DMA=0 4096 25088 | 300 = 0 10 32 32 1 1 8 3136 0 0 0 | 760 = 640: 0 10 32 32 2 2 4 6272 0 0 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 960: 0 10 32 32 3 3 8 3136 0 0 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
fp32 single plain FC_DMA=0 4096 4096 | 300 = 0 5 16 32 2 2 8 512 0 0 0 | 760 = 640: 0 5 16 32 4 4 4 1024 0 0 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 1000 = 960: 0 5 16 32 6 6 5 832 0 0 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 single plain FC_DMA=0 256 100352 | 300 = 0 5 16 2 2 2 128 784 0 0 0 | 760 = 640: 0 5 16 2 4 4 64 1568 0 0 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 960: 0 10 32 2 3 3 42 2400 0 0 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
fp32 single plain FC_EVEN=1 4096 25088 | 300 = 1 10 32 32 1 1 8 3136 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
fp32 single plain FC_EVEN=1 4096 4096 | 300 = 1 10 32 32 1 1 8 512 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 1000 = 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 single plain FC_EVEN=1 256 100352 | 300 = 1 10 32 2 1 1 121 832 1 1 1 | 760 = 640: 1 10 32 2 2 2 63 1600 1 1 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 960: 1 10 32 2 3 3 42 2432 1 1 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
fp32 single plain FC_NOTAIL=1 4096 25088 | 300 = 1 10 32 32 1 1 8 3136 1 1 1 | 760 = 1 10 32 32 3 3 8 3136 1 1 0 | 1000 = 1 10 32 32 4 4 2 12544 1 1 0
bf16x3 single plain FC_NOTAIL=1 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FC_NOTAIL=1 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
fp32 single plain FC_NOTAIL=1 4096 4096 | 300 = 1 10 32 32 1 1 8 512 1 1 1 | 760 = 1 10 32 32 3 3 5 832 1 1 0 | 1000 = 1 10 32 32 4 4 2 2048 1 1 0
bf16x3 single plain FC_NOTAIL=1 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FC_NOTAIL=1 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
fp32 single plain FC_NOTAIL=1 256 100352 | 300 = 1 10 32 2 1 1 126 800 1 1 1 | 760 = 1 10 32 2 3 3 42 2400 1 1 0 | 1000 = 1 10 32 2 4 4 32 3136 1 1 0
bf16x3 single plain FC_NOTAIL=1 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FC_NOTAIL=1 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
fp32 single plain FC_SPLIT_DIV=0 4096 25088 | 300 = 1 10 32 32 1 1 8 3136 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
bf16x3 single plain FC_SPLIT_DIV=0 4096 25088 | 300 = 2 10 32 32 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FC_SPLIT_DIV=0 4096 25088 | 300 = 3 10 64 16 1 1 16 1600 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
fp32 single plain FC_SPLIT_DIV=0 4096 4096 | 300 = 1 10 32 32 1 1 8 512 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 1000 = 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
bf16x3 single plain FC_SPLIT_DIV=0 4096 4096 | 300 = 2 5 32 32 2 -2 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FC_SPLIT_DIV=0 4096 4096 | 300 = 2 5 64 32 2 -2 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
fp32 single plain FC_SPLIT_DIV=0 256 100352 | 300 = 1 10 32 2 1 1 126 800 1 1 1 | 760 = 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
bf16x3 single plain FC_SPLIT_DIV=0 256 100352 | 300 = 2 5 32 2 2 2 32 3136 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FC_SPLIT_DIV=0 256 100352 | 300 = 2 5 64 2 2 2 32 3136 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
fp32 single plain FC_SPLIT_DIV=2 4096 25088 | 300 = 1 10 32 32 1 1 4 6272 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 8 3136 0 0 0 | 1000 = 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 8 3136 0 0 0
bf16x3 single plain FC_SPLIT_DIV=2 4096 25088 | 300 = 2 10 32 32 1 1 4 6272 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FC_SPLIT_DIV=2 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
fp32 single plain FC_SPLIT_DIV=2 4096 4096 | 300 = 1 10 32 32 1 1 4 1024 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 8 512 0 0 0 | 1000 = 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
bf16x3 single plain FC_SPLIT_DIV=2 4096 4096 | 300 = 2 5 32 32 2 -2 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FC_SPLIT_DIV=2 4096 4096 | 300 = 2 5 64 32 2 -2 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
fp32 single plain FC_SPLIT_DIV=2 256 100352 | 300 = 1 10 32 2 1 1 64 1568 1 1 1 | 760 = 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 0 5 16 2 1 1 128 784 0 0 0 | 1000 = 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 0 5 16 2 1 1 128 784 0 0 0
bf16x3 single plain FC_SPLIT_DIV=2 256 100352 | 300 = 3 10 32 1 1 1 126 800 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FC_SPLIT_DIV=2 256 100352 | 300 = 3 10 64 1 1 1 121 832 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
fp32 single plain FC_SPLIT_DIV=21 4096 25088 | 300 = 1 10 32 32 1 1 8 3136 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
bf16x3 single plain FC_SPLIT_DIV=21 4096 25088 | 300 = 2 10 32 32 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FC_SPLIT_DIV=21 4096 25088 | 300 = 3 10 64 16 1 1 16 1600 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
fp32 single plain FC_SPLIT_DIV=21 4096 4096 | 300 = 1 10 32 32 1 1 4 1024 1 1 1 | 760 = 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 8 512 0 0 0 | 1000 = 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
bf16x3 single plain FC_SPLIT_DIV=21 4096 4096 | 300 = 2 5 32 32 2 -2 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FC_SPLIT_DIV=21 4096 4096 | 300 = 2 5 64 32 2 -2 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
fp32 single plain FC_SPLIT_DIV=21 256 100352 | 300 = 1 10 32 2 1 1 126 800 1 1 1 | 760 = 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
bf16x3 single plain FC_SPLIT_DIV=21 256 100352 | 300 = 2 5 32 2 2 2 32 3136 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FC_SPLIT_DIV=21 256 100352 | 300 = 2 5 64 2 2 2 32 3136 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
fp32 pair plain - 4096 25088 | 1 = 2x 1: 0 2 32 32 1 1 16 1568 0 0 0 | 160 = 2x 160: 0 5 16 32 1 1 16 1568 0 0 0 | 161,288 = 1 10 32 64 1 1 4 6272 1 1 0 | 289,304 = 1 10 32 64 1 1 4 6272 1 1 1 | 305,320 = 1 10 32 64 1 1 4 6272 1 1 0 | 321 = 2x 320: 1 10 32 32 1 1 8 3136 1 1 0 / 1: 0 2 32 32 1 1 16 1568 0 0 0 | 480 = 2x 320: 1 10 32 32 1 1 8 3136 1 1 0 / 160: 0 5 16 32 1 1 16 1568 0 0 0 | 481,640 = 1 10 32 64 2 2 2 12544 1 1 0 | 760 = 2x 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 960 = 1 10 32 64 3 3 4 6272 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0 | 2000 = 2x 1920: 1 10 32 32 6 6 4 6272 1 1 0 / 80: 0 5 16 32 1 1 16 1568 0 0 0
bf16x3 pair plain - 4096 25088 | 1 = 2x 1: 2 2 32 32 1 1 16 1568 0 0 0 | 160 = 2x 160: 2 5 32 32 1 1 4 6272 0 0 0 | 161,288,289,304,305,320 = 3 10 32 32 1 1 2 12544 0 0 0 | 321 = 2x 320: 3 10 32 16 1 1 8 3136 0 0 0 / 1: 2 2 32 32 1 1 16 1568 0 0 0 | 480 = 2x 320: 3 10 32 16 1 1 8 3136 0 0 0 / 160: 2 5 32 32 1 1 4 6272 0 0 0 | 481 = 3 8 32 32 2 -2 2 12544 0 0 0 | 640 = 3 10 32 32 2 -2 2 12544 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 960 = 3 10 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0 | 2000 = 2x 1920: 3 10 32 16 6 -6 4 6272 0 0 0 / 80: 2 5 32 32 1 1 4 6272 0 0 0
f16,bf16 pair plain - 4096 25088 | 1 = 2x 1: 2 2 64 32 1 1 16 1600 0 0 0 | 160 = 2x 160: 2 5 64 32 1 1 4 6272 0 0 0 | 161,288,289,304,305,320 = 3 10 64 32 1 1 2 12544 0 0 0 | 321 = 2x 320: 3 10 64 16 1 1 8 3136 0 0 0 / 1: 2 2 64 32 1 1 16 1600 0 0 0 | 480 = 2x 320: 3 10 64 16 1 1 8 3136 0 0 0 / 160: 2 5 64 32 1 1 4 6272 0 0 0 | 481 = 3 8 64 32 2 -2 2 12544 0 0 0 | 640 = 3 10 64 32 2 -2 2 12544 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 960 = 3 10 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0 | 2000 = 2x 1920: 3 10 64 16 6 -6 4 6272 0 0 0 / 80: 2 5 64 32 1 1 4 6272 0 0 0
fp32 pair plain - 4096 4096 | 1 = 2x 1: 0 2 32 32 1 1 16 256 0 0 0 | 160 = 2x 160: 0 5 16 32 1 1 16 256 0 0 0 | 161,288 = 1 10 32 64 1 1 4 1024 1 1 0 | 289,304 = 1 10 32 64 1 1 4 1024 1 1 1 | 305,320 = 1 10 32 64 1 1 4 1024 1 1 0 | 321 = 2x 320: 1 10 32 32 1 1 8 512 1 1 0 / 1: 0 2 32 32 1 1 16 256 0 0 0 | 480 = 2x 320: 1 10 32 32 1 1 8 512 1 1 0 / 160: 0 5 16 32 1 1 16 256 0 0 0 | 481,640 = 1 10 32 64 2 2 2 2048 1 1 0 | 760 = 2x 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 960 = 1 10 32 64 3 3 4 1024 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0 | 2000 = 2x 1920: 1 10 32 32 6 6 4 1024 1 1 0 / 80: 0 5 16 32 1 1 16 256 0 0 0 | 59 = 2x 59: 0 2 32 32 1 1 16 256 0 0 0 | 60 = 2x 60: 0 5 16 32 1 1 16 256 0 0 0
bf16x3 pair plain - 4096 4096 | 1 = 2x 1: 2 2 32 32 1 1 16 256 0 0 0 | 160 = 2x 160: 2 5 32 32 1 1 2 2048 0 0 0 | 161,288,289,304,305,320 = 3 10 32 32 1 1 1 4096 0 0 0 | 321 = 2x 320: 3 10 32 16 1 1 2 2048 0 0 0 / 1: 2 2 32 32 1 1 16 256 0 0 0 | 480 = 2x 320: 3 10 32 16 1 1 2 2048 0 0 0 / 160: 2 5 32 32 1 1 2 2048 0 0 0 | 481 = 3 8 32 32 2 -2 2 2048 0 0 0 | 640 = 3 10 32 32 2 -2 2 2048 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 960 = 3 10 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0 | 2000 = 2x 1920: 3 10 32 16 6 -6 4 1024 0 0 0 / 80: 2 5 32 32 1 1 2 2048 0 0 0 | 59 = 2x 59: 2 2 32 32 1 1 16 256 0 0 0 | 60 = 2x 60: 2 5 32 32 1 1 2 2048 0 0 0
f16,bf16 pair plain - 4096 4096 | 1 = 2x 1: 2 2 64 32 1 1 16 256 0 0 0 | 160 = 2x 160: 2 5 64 32 1 1 2 2048 0 0 0 | 161,288,289,304,305,320 = 3 10 64 32 1 1 1 4096 0 0 0 | 321 = 2x 320: 3 10 64 16 1 1 2 2048 0 0 0 / 1: 2 2 64 32 1 1 16 256 0 0 0 | 480 = 2x 320: 3 10 64 16 1 1 2 2048 0 0 0 / 160: 2 5 64 32 1 1 2 2048 0 0 0 | 481 = 3 8 64 32 2 -2 2 2048 0 0 0 | 640 = 3 10 64 32 2 -2 2 2048 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 960 = 3 10 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0 | 2000 = 2x 1920: 3 10 64 16 6 -6 1 4096 0 0 0 / 80: 2 5 64 32 1 1 2 2048 0 0 0 | 59 = 2x 59: 2 2 64 32 1 1 16 256 0 0 0 | 60 = 2x 60: 2 5 64 32 1 1 2 2048 0 0 0
fp32 pair plain - 256 100352 | 1 = 2x 1: 0 2 32 2 1 1 242 416 0 0 0 | 160 = 2x 160: 0 5 16 2 1 1 251 400 0 0 0 | 161,288 = 1 10 32 4 1 1 63 1600 1 1 0 | 289,304 = 1 10 32 4 1 1 63 1600 1 1 1 | 305,320 = 1 10 32 4 1 1 63 1600 1 1 0 | 321 = 2x 320: 1 10 32 2 1 1 126 800 1 1 0 / 1: 0 2 32 2 1 1 242 416 0 0 0 | 480 = 2x 320: 1 10 32 2 1 1 126 800 1 1 0 / 160: 0 5 16 2 1 1 251 400 0 0 0 | 481,640 = 1 10 32 4 2 2 32 3136 1 1 0 | 760 = 2x 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 960 = 1 10 32 4 3 3 21 4800 1 1 0 | 1000 = 2x 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 0 5 16 2 1 1 251 400 0 0 0 | 2000 = 2x 1920: 1 10 32 2 6 6 21 4800 1 1 0 / 80: 0 5 16 2 1 1 251 400 0 0 0
bf16x3 pair plain - 256 100352 | 1 = 2x 1: 2 2 32 2 1 1 242 416 0 0 0 | 160 = 2x 160: 2 5 32 2 1 1 49 2048 0 0 0 | 161 = 2x 161: 3 10 32 1 1 1 49 2048 0 0 0 | 288 = 2x 288: 3 10 32 1 1 1 49 2048 0 0 0 | 289 = 2x 289: 3 10 32 1 1 1 49 2048 0 0 0 | 304 = 2x 304: 3 10 32 1 1 1 49 2048 0 0 0 | 305 = 2x 305: 3 10 32 1 1 1 49 2048 0 0 0 | 320 = 2x 320: 3 10 32 1 1 1 49 2048 0 0 0 | 321 = 2x 320: 3 10 32 1 1 1 49 2048 0 0 0 / 1: 2 2 32 2 1 1 242 416 0 0 0 | 480 = 2x 320: 3 10 32 1 1 1 49 2048 0 0 0 / 160: 2 5 32 2 1 1 49 2048 0 0 0 | 481 = 2x 481: 3 8 32 1 2 2 64 1568 0 0 0 | 640 = 2x 640: 2 5 32 2 4 4 16 6272 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 960 = 2x 960: 3 10 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0 | 2000 = 2x 1920: 3 10 32 1 6 6 21 4800 0 0 0 / 80: 2 5 32 2 1 1 49 2048 0 0 0
f16,bf16 pair plain - 256 100352 | 1 = 2x 1: 2 2 64 2 1 1 224 448 0 0 0 | 160 = 2x 160: 2 5 64 2 1 1 49 2048 0 0 0 | 161 = 2x 161: 3 10 64 1 1 1 49 2048 0 0 0 | 288 = 2x 288: 3 10 64 1 1 1 49 2048 0 0 0 | 289 = 2x 289: 3 10 64 1 1 1 49 2048 0 0 0 | 304 = 2x 304: 3 10 64 1 1 1 49 2048 0 0 0 | 305 = 2x 305: 3 10 64 1 1 1 49 2048 0 0 0 | 320 = 2x 320: 3 10 64 1 1 1 49 2048 0 0 0 | 321 = 2x 320: 3 10 64 1 1 1 49 2048 0 0 0 / 1: 2 2 64 2 1 1 224 448 0 0 0 | 480 = 2x 320: 3 10 64 1 1 1 49 2048 0 0 0 / 160: 2 5 64 2 1 1 49 2048 0 0 0 | 481 = 2x 481: 3 8 64 1 2 2 63 1600 0 0 0 | 640 = 2x 640: 2 5 64 2 4 4 16 6272 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 960 = 2x 960: 3 10 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0 | 2000 = 2x 1920: 3 10 64 1 6 6 21 4800 0 0 0 / 80: 2 5 64 2 1 1 49 2048 0 0 0
fp32 pair plain - 441 256 | 1 = 2x 1: 0 2 32 4 1 1 1 256 0 0 0 | 160 = 2x 160: 0 2 32 4 3 3 1 256 0 0 0 | 161 = 2x 161: 0 2 32 4 3 3 1 256 0 0 0 | 288 = 2x 288: 0 2 32 4 5 5 1 256 0 0 0 | 289 = 2x 289: 0 2 32 4 5 5 1 256 0 0 0 | 304 = 2x 304: 0 2 32 4 5 5 1 256 0 0 0 | 305 = 2x 305: 0 2 32 4 5 5 1 256 0 0 0 | 320 = 2x 320: 0 2 32 4 5 5 1 256 0 0 0 | 321 = 2x 321: 0 2 32 4 6 6 1 256 0 0 0 | 480 = 2x 480: 0 2 32 4 8 8 1 256 0 0 0 | 481 = 2x 481: 0 2 32 4 8 8 1 256 0 0 0 | 640 = 2x 640: 0 2 32 4 10 10 1 256 0 0 0 | 760 = 2x 760: 0 2 32 4 12 12 1 256 0 0 0 | 960 = 2x 960: 0 2 32 4 15 15 1 256 0 0 0 | 1000 = 2x 1000: 0 2 32 4 16 16 1 256 0 0 0 | 2000 = 2x 2000: 0 2 32 4 32 32 1 256 0 0 0
bf16x3 pair plain - 441 256 | 1 = 2x 1: 2 2 32 4 1 1 4 64 0 0 0 | 160 = 2x 160: 2 2 32 4 3 3 4 64 0 0 0 | 161 = 2x 161: 2 2 32 4 3 3 4 64 0 0 0 | 288 = 2x 288: 2 2 32 4 5 5 4 64 0 0 0 | 289 = 2x 289: 2 2 32 4 5 5 4 64 0 0 0 | 304 = 2x 304: 2 2 32 4 5 5 4 64 0 0 0 | 305 = 2x 305: 2 2 32 4 5 5 4 64 0 0 0 | 320 = 2x 320: 2 2 32 4 5 5 4 64 0 0 0 | 321 = 2x 321: 2 2 32 4 6 6 4 64 0 0 0 | 480 = 2x 480: 2 2 32 4 8 8 4 64 0 0 0 | 481 = 2x 481: 2 2 32 4 8 8 4 64 0 0 0 | 640 = 2x 640: 2 2 32 4 10 10 4 64 0 0 0 | 760 = 2x 760: 2 2 32 4 12 12 4 64 0 0 0 | 960 = 2x 960: 2 2 32 4 15 15 4 64 0 0 0 | 1000 = 2x 1000: 2 2 32 4 16 16 4 64 0 0 0 | 2000 = 2x 2000: 2 2 32 4 32 32 4 64 0 0 0
f16,bf16 pair plain - 441 256 | 1 = 2x 1: 2 2 64 4 1 1 4 64 0 0 0 | 160 = 2x 160: 2 2 64 4 3 3 4 64 0 0 0 | 161 = 2x 161: 2 2 64 4 3 3 4 64 0 0 0 | 288 = 2x 288: 2 2 64 4 5 5 4 64 0 0 0 | 289 = 2x 289: 2 2 64 4 5 5 4 64 0 0 0 | 304 = 2x 304: 2 2 64 4 5 5 4 64 0 0 0 | 305 = 2x 305: 2 2 64 4 5 5 4 64 0 0 0 | 320 = 2x 320: 2 2 64 4 5 5 4 64 0 0 0 | 321 = 2x 321: 2 2 64 4 6 6 4 64 0 0 0 | 480 = 2x 480: 2 2 64 4 8 8 4 64 0 0 0 | 481 = 2x 481: 2 2 64 4 8 8 4 64 0 0 0 | 640 = 2x 640: 2 2 64 4 10 10 4 64 0 0 0 | 760 = 2x 760: 2 2 64 4 12 12 4 64 0 0 0 | 960 = 2x 960: 2 2 64 4 15 15 4 64 0 0 0 | 1000 = 2x 1000: 2 2 64 4 16 16 4 64 0 0 0 | 2000 = 2x 2000: 2 2 64 4 32 32 4 64 0 0 0
fp32 pair plain - 126 8192 | 1 = 2x 1: 0 2 32 1 1 1 32 256 0 0 0 | 160 = 2x 160: 0 2 32 1 3 3 32 256 0 0 0 | 161 = 2x 161: 0 2 32 1 3 3 32 256 0 0 0 | 288 = 2x 288: 0 2 32 1 5 5 32 256 0 0 0 | 289 = 2x 289: 0 2 32 1 5 5 32 256 0 0 0 | 304 = 2x 304: 0 2 32 1 5 5 32 256 0 0 0 | 305 = 2x 305: 0 2 32 1 5 5 32 256 0 0 0 | 320 = 2x 320: 0 2 32 1 5 5 32 256 0 0 0 | 321 = 2x 321: 0 2 32 1 6 6 32 256 0 0 0 | 480 = 2x 480: 0 2 32 1 8 8 32 256 0 0 0 | 481 = 2x 481: 0 2 32 1 8 8 32 256 0 0 0 | 640 = 2x 640: 0 2 32 1 10 10 32 256 0 0 0 | 760 = 2x 760: 0 2 32 1 12 12 32 256 0 0 0 | 960 = 2x 960: 0 2 32 1 15 15 32 256 0 0 0 | 1000 = 2x 960: 0 2 32 1 15 15 32 256 0 0 0 / 40: 0 2 32 1 1 1 32 256 0 0 0 | 2000 = 2x 1920: 1 10 32 1 6 6 32 256 1 1 0 / 80: 0 2 32 1 2 2 32 256 0 0 0
bf16x3 pair plain - 126 8192 | 1 = 2x 1: 2 2 32 1 1 1 128 64 0 0 0 | 160 = 2x 160: 2 2 32 1 3 3 128 64 0 0 0 | 161 = 2x 161: 2 2 32 1 3 3 128 64 0 0 0 | 288 = 2x 288: 2 2 32 1 5 5 86 96 0 0 0 | 289 = 2x 289: 2 2 32 1 5 5 86 96 0 0 0 | 304 = 2x 304: 2 2 32 1 5 5 86 96 0 0 0 | 305 = 2x 305: 2 2 32 1 5 5 86 96 0 0 0 | 320 = 2x 320: 2 2 32 1 5 5 86 96 0 0 0 | 321 = 2x 321: 2 2 32 1 6 6 86 96 0 0 0 | 480 = 2x 480: 2 2 32 1 8 8 64 128 0 0 0 | 481 = 2x 481: 2 2 32 1 8 8 64 128 0 0 0 | 640 = 2x 640: 2 2 32 1 10 10 52 160 0 0 0 | 760 = 2x 760: 2 2 32 1 12 12 43 192 0 0 0 | 960 = 2x 960: 2 2 32 1 15 15 32 256 0 0 0 | 1000 = 2x 1000: 2 8 32 1 4 4 32 256 0 0 0 | 2000 = 2x 1920: 2 5 32 1 12 12 10 832 0 0 0 / 80: 2 2 32 1 2 2 128 64 0 0 0
f16,bf16 pair plain - 126 8192 | 1 = 2x 1: 2 2 64 1 1 1 128 64 0 0 0 | 160 = 2x 160: 2 2 64 1 3 3 128 64 0 0 0 | 161 = 2x 161: 2 2 64 1 3 3 128 64 0 0 0 | 288 = 2x 288: 2 2 64 1 5 5 64 128 0 0 0 | 289 = 2x 289: 2 2 64 1 5 5 64 128 0 0 0 | 304 = 2x 304: 2 2 64 1 5 5 64 128 0 0 0 | 305 = 2x 305: 2 2 64 1 5 5 64 128 0 0 0 | 320 = 2x 320: 2 2 64 1 5 5 64 128 0 0 0 | 321 = 2x 321: 2 2 64 1 6 6 64 128 0 0 0 | 480 = 2x 480: 2 2 64 1 8 8 64 128 0 0 0 | 481 = 2x 481: 2 2 64 1 8 8 64 128 0 0 0 | 640 = 2x 640: 2 2 64 1 10 10 43 192 0 0 0 | 760 = 2x 760: 2 2 64 1 12 12 43 192 0 0 0 | 960 = 2x 960: 2 2 64 1 15 15 32 256 0 0 0 | 1000 = 2x 1000: 2 8 64 1 4 4 32 256 0 0 0 | 2000 = 2x 1920: 2 5 64 1 12 12 10 832 0 0 0 / 80: 2 2 64 1 2 2 128 64 0 0 0
fp32 pair plain - 4096 50176 | 1 = 2x 1: 0 2 32 32 1 1 16 3136 0 0 0 | 160 = 2x 160: 0 5 16 32 1 1 16 3136 0 0 0 | 161,288 = 1 10 32 64 1 1 4 12544 1 1 0 | 289,304 = 1 10 32 64 1 1 4 12544 1 1 1 | 305,320 = 1 10 32 64 1 1 4 12544 1 1 0 | 321 = 2x 320: 1 10 32 32 1 1 8 6272 1 1 0 / 1: 0 2 32 32 1 1 16 3136 0 0 0 | 480 = 2x 320: 1 10 32 32 1 1 8 6272 1 1 0 / 160: 0 5 16 32 1 1 16 3136 0 0 0 | 481,640 = 1 10 32 64 2 2 2 25088 1 1 0 | 760 = 2x 640: 1 10 32 32 2 2 4 12544 1 1 0 / 120: 0 5 16 32 1 1 16 3136 0 0 0 | 960 = 1 10 32 64 3 3 4 12544 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 6272 1 1 0 / 40: 0 5 16 32 1 1 16 3136 0 0 0 | 2000 = 2x 1920: 1 10 32 32 6 6 4 12544 1 1 0 / 80: 0 5 16 32 1 1 16 3136 0 0 0
bf16x3 pair plain - 4096 50176 | 1 = 2x 1: 2 2 32 32 1 1 16 3136 0 0 0 | 160 = 2x 160: 2 5 32 32 1 1 4 12544 0 0 0 | 161,288,289,304,305,320 = 3 10 32 32 1 1 4 12544 0 0 0 | 321 = 2x 320: 3 10 32 16 1 1 8 6272 0 0 0 / 1: 2 2 32 32 1 1 16 3136 0 0 0 | 480 = 2x 320: 3 10 32 16 1 1 8 6272 0 0 0 / 160: 2 5 32 32 1 1 4 12544 0 0 0 | 481 = 3 8 32 32 2 -2 2 25088 0 0 0 | 640 = 3 10 32 32 2 -2 2 25088 0 0 0 | 760 = 3 8 32 32 3 -3 4 12544 0 0 0 | 960 = 3 10 32 32 3 -3 4 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 1 50176 0 0 0 | 2000 = 2x 1920: 3 10 32 16 6 -6 4 12544 0 0 0 / 80: 2 5 32 32 1 1 4 12544 0 0 0
f16,bf16 pair plain - 4096 50176 | 1 = 2x 1: 2 2 64 32 1 1 16 3136 0 0 0 | 160 = 2x 160: 2 5 64 32 1 1 4 12544 0 0 0 | 161,288,289,304,305,320 = 3 10 64 32 1 1 4 12544 0 0 0 | 321 = 2x 320: 3 10 64 16 1 1 8 6272 0 0 0 / 1: 2 2 64 32 1 1 16 3136 0 0 0 | 480 = 2x 320: 3 10 64 16 1 1 8 6272 0 0 0 / 160: 2 5 64 32 1 1 4 12544 0 0 0 | 481 = 3 8 64 32 2 -2 2 25088 0 0 0 | 640 = 3 10 64 32 2 -2 2 25088 0 0 0 | 760 = 3 8 64 32 3 -3 4 12544 0 0 0 | 960 = 3 10 64 32 3 -3 4 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 1 50176 0 0 0 | 2000 = 2x 1920: 3 10 64 16 6 -6 4 12544 0 0 0 / 80: 2 5 64 32 1 1 4 12544 0 0 0
fp32 pair plain - 256 200704 | 1 = 2x 1: 0 2 32 2 1 1 251 800 0 0 0 | 160 = 2x 160: 0 5 16 2 1 1 256 784 0 0 0 | 161,288 = 1 10 32 4 1 1 64 3136 1 1 0 | 289,304 = 1 10 32 4 1 1 64 3136 1 1 1 | 305,320 = 1 10 32 4 1 1 64 3136 1 1 0 | 321 = 2x 320: 1 10 32 2 1 1 128 1568 1 1 0 / 1: 0 2 32 2 1 1 251 800 0 0 0 | 480 = 2x 320: 1 10 32 2 1 1 128 1568 1 1 0 / 160: 0 5 16 2 1 1 256 784 0 0 0 | 481,640 = 1 10 32 4 2 2 32 6272 1 1 0 | 760 = 2x 640: 1 10 32 2 2 2 64 3136 1 1 0 / 120: 0 5 16 2 1 1 256 784 0 0 0 | 960 = 1 10 32 4 3 3 21 9600 1 1 0 | 1000 = 2x 960: 1 10 32 2 3 3 42 4800 1 1 0 / 40: 0 5 16 2 1 1 256 784 0 0 0 | 2000 = 2x 1920: 1 10 32 2 6 6 21 9568 1 1 0 / 80: 0 5 16 2 1 1 256 784 0 0 0
bf16x3 pair plain - 256 200704 | 1 = 2x 1: 2 2 32 2 1 1 251 800 0 0 0 | 160 = 2x 160: 2 5 32 2 1 1 64 3136 0 0 0 | 161 = 2x 161: 3 10 32 1 1 1 98 2048 0 0 0 | 288 = 2x 288: 3 10 32 1 1 1 98 2048 0 0 0 | 289 = 2x 289: 3 10 32 1 1 1 98 2048 0 0 0 | 304 = 2x 304: 3 10 32 1 1 1 98 2048 0 0 0 | 305 = 2x 305: 3 10 32 1 1 1 98 2048 0 0 0 | 320 = 2x 320: 3 10 32 1 1 1 98 2048 0 0 0 | 321 = 2x 320: 3 10 32 1 1 1 98 2048 0 0 0 / 1: 2 2 32 2 1 1 251 800 0 0 0 | 480 = 2x 320: 3 10 32 1 1 1 98 2048 0 0 0 / 160: 2 5 32 2 1 1 64 3136 0 0 0 | 481 = 2x 481: 3 8 32 1 2 2 64 3136 0 0 0 | 640 = 2x 640: 3 10 32 1 2 2 64 3136 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 4800 0 0 0 | 960 = 2x 960: 3 10 32 1 3 3 42 4800 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 6272 0 0 0 | 2000 = 2x 1920: 3 10 32 1 6 6 21 9568 0 0 0 / 80: 2 5 32 2 1 1 64 3136 0 0 0
f16,bf16 pair plain - 256 200704 | 1 = 2x 1: 2 2 64 2 1 1 242 832 0 0 0 | 160 = 2x 160: 2 5 64 2 1 1 64 3136 0 0 0 | 161 = 2x 161: 3 10 64 1 1 1 98 2048 0 0 0 | 288 = 2x 288: 3 10 64 1 1 1 98 2048 0 0 0 | 289 = 2x 289: 3 10 64 1 1 1 98 2048 0 0 0 | 304 = 2x 304: 3 10 64 1 1 1 98 2048 0 0 0 | 305 = 2x 305: 3 10 64 1 1 1 98 2048 0 0 0 | 320 = 2x 320: 3 10 64 1 1 1 98 2048 0 0 0 | 321 = 2x 320: 3 10 64 1 1 1 98 2048 0 0 0 / 1: 2 2 64 2 1 1 242 832 0 0 0 | 480 = 2x 320: 3 10 64 1 1 1 98 2048 0 0 0 / 160: 2 5 64 2 1 1 64 3136 0 0 0 | 481 = 2x 481: 3 8 64 1 2 2 64 3136 0 0 0 | 640 = 2x 640: 3 10 64 1 2 2 64 3136 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 4800 0 0 0 | 960 = 2x 960: 3 10 64 1 3 3 42 4800 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 6272 0 0 0 | 2000 = 2x 1920: 3 10 64 1 6 6 21 9600 0 0 0 / 80: 2 5 64 2 1 1 64 3136 0 0 0
fp32 pair plain - 256 16384 | 238 = 2x 238: 0 2 32 2 4 4 64 256 0 0 0 | 239 = 1 10 32 4 1 1 64 256 1 1 0
bf16x3 pair plain - 256 16384 | 238 = 2x 238: 2 2 32 2 4 4 64 256 0 0 0 | 239 = 2x 239: 3 10 32 1 1 1 8 2048 0 0 0
f16,bf16 pair plain - 256 16384 | 238 = 2x 238: 2 2 64 2 4 4 64 256 0 0 0 | 239 = 2x 239: 3 10 64 1 1 1 8 2048 0 0 0
fp32 pair ld2 - 4096 25088 | 300 = 1 10 32 64 1 1 4 6272 1 1 1 | 640 = 1 10 32 64 2 2 2 12544 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
bf16x3 pair ld2 - 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 640 = 3 10 32 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair ld2 - 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 640 = 3 10 64 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
fp32 pair ld2 - 4096 4096 | 300 = 1 10 32 64 1 1 4 1024 1 1 1 | 640 = 1 10 32 64 2 2 2 2048 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
bf16x3 pair ld2 - 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 640 = 3 10 32 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair ld2 - 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 640 = 3 10 64 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
fp32 pair ld+2 - 4096 25088 | 300 = 2x 300: 1 10 32 32 1 1 8 3136 1 1 1 | 640 = 2x 640: 1 10 32 32 2 2 4 6272 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
fp32 pair ld+2 - 4096 4096 | 300 = 2x 300: 1 10 32 32 1 1 8 512 1 1 1 | 640 = 2x 640: 1 10 32 32 2 2 4 1024 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 pair plain FC_TILE=5 4096 25088 | 300 = 2x 300: 0 5 16 32 2 2 8 3136 0 0 0 | 760 = 2x 640: 0 5 16 32 4 4 4 6272 0 0 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 2x 960: 0 5 16 32 6 6 8 3136 0 0 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
fp32 pair plain FC_TILE=5 4096 4096 | 300 = 2x 300: 0 5 16 32 2 2 8 512 0 0 0 | 760 = 2x 640: 0 5 16 32 4 4 4 1024 0 0 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 1000 = 2x 960: 0 5 16 32 6 6 5 832 0 0 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 pair plain FC_TILE=5 256 100352 | 300 = 2x 300: 0 5 16 2 2 2 128 784 0 0 0 | 760 = 2x 640: 0 5 16 2 4 4 64 1568 0 0 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 2x 960: 0 5 16 2 6 6 42 2400 0 0 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
fp32 pair plain FC_TILE=10 4096 25088 | 300 = 2x 300: 1 10 32 32 1 1 8 3136 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 1 10 32 32 1 1 8 3136 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 1 10 32 32 1 1 8 3136 1 1 0
fp32 pair plain FC_TILE=10 4096 4096 | 300 = 2x 300: 1 10 32 32 1 1 8 512 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 1 10 32 32 1 1 8 512 1 1 0 | 1000 = 2x 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 pair plain FC_TILE=10 256 100352 | 300 = 2x 300: 1 10 32 2 1 1 126 800 1 1 1 | 760 = 2x 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 1 10 32 2 1 1 126 800 1 1 0 | 1000 = 2x 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 1 10 32 2 1 1 126 800 1 1 0
fp32 pair plain FC_DMA=0 4096 25088 | 300 = 2x 300: 0 10 32 32 1 1 8 3136 0 0 0 | 760 = 2x 640: 0 10 32 32 2 2 4 6272 0 0 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 2x 960: 0 10 32 32 3 3 8 3136 0 0 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
fp32 pair plain FC_DMA=0 4096 4096 | 300 = 2x 300: 0 5 16 32 2 2 8 512 0 0 0 | 760 = 2x 640: 0 5 16 32 4 4 4 1024 0 0 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 1000 = 2x 960: 0 5 16 32 6 6 5 832 0 0 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 pair plain FC_DMA=0 256 100352 | 300 = 2x 300: 0 5 16 2 2 2 128 784 0 0 0 | 760 = 2x 640: 0 5 16 2 4 4 64 1568 0 0 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 2x 960: 0 10 32 2 3 3 42 2400 0 0 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
fp32 pair plain FC_EVEN=1 4096 25088 | 300 = 1 10 32 64 1 1 4 6272 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
fp32 pair plain FC_EVEN=1 4096 4096 | 300 = 1 10 32 64 1 1 4 1024 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 1000 = 2x 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
fp32 pair plain FC_EVEN=1 256 100352 | 300 = 1 10 32 4 1 1 63 1600 1 1 1 | 760 = 2x 640: 1 10 32 2 2 2 63 1600 1 1 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 2x 960: 1 10 32 2 3 3 42 2432 1 1 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
fp32 pair plain FC_NOTAIL=1 4096 25088 | 300 = 1 10 32 64 1 1 4 6272 1 1 1 | 760 = 1 10 32 64 3 3 4 6272 1 1 0 | 1000 = 1 10 32 64 4 4 1 25088 1 1 0
bf16x3 pair plain FC_NOTAIL=1 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FC_NOTAIL=1 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
fp32 pair plain FC_NOTAIL=1 4096 4096 | 300 = 1 10 32 64 1 1 4 1024 1 1 1 | 760 = 1 10 32 64 3 3 4 1024 1 1 0 | 1000 = 1 10 32 64 4 4 1 4096 1 1 0
bf16x3 pair plain FC_NOTAIL=1 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FC_NOTAIL=1 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
fp32 pair plain FC_NOTAIL=1 256 100352 | 300 = 1 10 32 4 1 1 63 1600 1 1 1 | 760 = 1 10 32 4 3 3 21 4800 1 1 0 | 1000 = 1 10 32 4 4 4 16 6272 1 1 0
bf16x3 pair plain FC_NOTAIL=1 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FC_NOTAIL=1 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
fp32 pair plain FC_SPLIT_DIV=0 4096 25088 | 300 = 1 10 32 64 1 1 4 6272 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=0 4096 25088 | 300 = 3 10 32 32 1 1 8 3136 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FC_SPLIT_DIV=0 4096 25088 | 300 = 3 10 64 32 1 1 8 3136 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
fp32 pair plain FC_SPLIT_DIV=0 4096 4096 | 300 = 1 10 32 64 1 1 4 1024 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 16 256 0 0 0 | 1000 = 2x 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=0 4096 4096 | 300 = 3 10 32 32 1 1 8 512 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FC_SPLIT_DIV=0 4096 4096 | 300 = 3 10 64 32 1 1 8 512 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
fp32 pair plain FC_SPLIT_DIV=0 256 100352 | 300 = 1 10 32 4 1 1 63 1600 1 1 1 | 760 = 2x 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 2x 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=0 256 100352 | 300 = 2x 300: 2 5 32 2 2 2 32 3136 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FC_SPLIT_DIV=0 256 100352 | 300 = 2x 300: 2 5 64 2 2 2 32 3136 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
fp32 pair plain FC_SPLIT_DIV=2 4096 25088 | 300 = 1 10 32 64 1 1 2 12544 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 8 3136 0 0 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 8 3136 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=2 4096 25088 | 300 = 3 10 32 32 1 1 4 6272 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FC_SPLIT_DIV=2 4096 25088 | 300 = 3 10 64 32 1 1 4 6272 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
fp32 pair plain FC_SPLIT_DIV=2 4096 4096 | 300 = 1 10 32 64 1 1 2 2048 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 8 512 0 0 0 | 1000 = 2x 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=2 4096 4096 | 300 = 3 10 32 32 1 1 4 1024 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FC_SPLIT_DIV=2 4096 4096 | 300 = 3 10 64 32 1 1 4 1024 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
fp32 pair plain FC_SPLIT_DIV=2 256 100352 | 300 = 1 10 32 4 1 1 32 3136 1 1 1 | 760 = 2x 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 0 5 16 2 1 1 128 784 0 0 0 | 1000 = 2x 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 0 5 16 2 1 1 128 784 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=2 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 126 800 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FC_SPLIT_DIV=2 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 121 832 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
fp32 pair plain FC_SPLIT_DIV=21 4096 25088 | 300 = 1 10 32 64 1 1 4 6272 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 6272 1 1 0 / 120: 0 5 16 32 1 1 16 1568 0 0 0 | 1000 = 2x 960: 1 10 32 32 3 3 8 3136 1 1 0 / 40: 0 5 16 32 1 1 16 1568 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=21 4096 25088 | 300 = 3 10 32 32 1 1 8 3136 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FC_SPLIT_DIV=21 4096 25088 | 300 = 3 10 64 32 1 1 8 3136 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
fp32 pair plain FC_SPLIT_DIV=21 4096 4096 | 300 = 1 10 32 64 1 1 2 2048 1 1 1 | 760 = 2x 640: 1 10 32 32 2 2 4 1024 1 1 0 / 120: 0 5 16 32 1 1 8 512 0 0 0 | 1000 = 2x 960: 1 10 32 32 3 3 5 832 1 1 0 / 40: 0 2 32 32 1 1 16 256 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=21 4096 4096 | 300 = 3 10 32 32 1 1 4 1024 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FC_SPLIT_DIV=21 4096 4096 | 300 = 3 10 64 32 1 1 4 1024 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
fp32 pair plain FC_SPLIT_DIV=21 256 100352 | 300 = 1 10 32 4 1 1 63 1600 1 1 1 | 760 = 2x 640: 1 10 32 2 2 2 64 1568 1 1 0 / 120: 0 5 16 2 1 1 251 400 0 0 0 | 1000 = 2x 960: 1 10 32 2 3 3 42 2400 1 1 0 / 40: 0 5 16 2 1 1 251 400 0 0 0
bf16x3 pair plain FC_SPLIT_DIV=21 256 100352 | 300 = 2x 300: 2 5 32 2 2 2 32 3136 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FC_SPLIT_DIV=21 256 100352 | 300 = 2x 300: 2 5 64 2 2 2 32 3136 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 single pre - 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 640 = 3 10 32 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single pre - 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 640 = 3 10 64 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single pre - 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 640 = 2 5 32 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single pre - 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 640 = 2 5 64 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single osm - 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 640 = 3 10 32 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single osm - 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 640 = 3 10 64 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single osm - 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 640 = 2 5 32 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single osm - 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 640 = 2 5 64 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single pre+osm - 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 640 = 3 10 32 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single pre+osm - 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 640 = 3 10 64 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single pre+osm - 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 640 = 2 5 32 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single pre+osm - 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 640 = 2 5 64 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single pre+ld2 - 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 640 = 3 10 32 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single pre+ld2 - 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 640 = 3 10 64 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single pre+ld2 - 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 640 = 2 5 32 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single pre+ld2 - 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 640 = 2 5 64 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single osm+ld2 - 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 640 = 3 10 32 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single osm+ld2 - 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 640 = 3 10 64 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single osm+ld2 - 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 640 = 2 5 32 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single osm+ld2 - 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 640 = 2 5 64 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single pre+osm+ld2 - 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 640 = 3 10 32 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single pre+osm+ld2 - 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 640 = 3 10 64 16 2 -2 4 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single pre+osm+ld2 - 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 640 = 2 5 32 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single pre+osm+ld2 - 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 640 = 2 5 64 32 4 -4 1 4096 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single plain PLAN=1 4096 25088 | 300 = 2 10 32 32 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 5 5024 0 0 0 | 1000 = 3 8 32 16 4 -4 4 6272 0 0 0
f16 single plain PLAN=1 4096 25088 | 300 = 3 10 64 16 1 1 16 1600 0 0 0 | 760 = 3 8 64 16 3 -3 5 5056 0 0 0 | 1000 = 3 8 64 16 4 -4 4 6272 0 0 0
bf16x3 single plain PLAN=1 4096 4096 | 300 = 2 5 32 32 2 -2 4 1024 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 4 1024 0 0 0
f16 single plain PLAN=1 4096 4096 | 300 = 2 5 64 32 2 -2 4 1024 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 4 1024 0 0 0
bf16x3 single plain PLAN=1 256 100352 | 300 = 2 5 32 2 2 2 64 1568 0 0 0 | 760 = 2 8 32 2 3 3 42 2400 0 0 0 | 1000 = 2 8 32 2 4 4 32 3136 0 0 0
f16 single plain PLAN=1 256 100352 | 300 = 2 5 64 2 2 2 63 1600 0 0 0 | 760 = 2 8 64 2 3 3 42 2432 0 0 0 | 1000 = 2 8 64 2 4 4 32 3136 0 0 0
bf16x3 single plain FCX3_TILE=2 4096 25088 | 300 = 2 2 32 32 5 -5 4 6272 0 0 0 | 760 = 2 2 32 32 12 -12 2 12544 0 0 0 | 1000 = 2 2 32 32 16 -16 1 25088 0 0 0
f16 single plain FCX3_TILE=2 4096 25088 | 300 = 2 2 64 32 5 -5 4 6272 0 0 0 | 760 = 2 2 64 32 12 -12 2 12544 0 0 0 | 1000 = 2 2 64 32 16 -16 1 25088 0 0 0
bf16x3 single plain FCX3_TILE=2 4096 4096 | 300 = 2 2 32 32 5 -5 4 1024 0 0 0 | 760 = 2 2 32 32 12 -12 2 2048 0 0 0 | 1000 = 2 2 32 32 16 -16 1 4096 0 0 0
f16 single plain FCX3_TILE=2 4096 4096 | 300 = 2 2 64 32 5 -5 4 1024 0 0 0 | 760 = 2 2 64 32 12 -12 2 2048 0 0 0 | 1000 = 2 2 64 32 16 -16 1 4096 0 0 0
bf16x3 single plain FCX3_TILE=2 256 100352 | 300 = 2 2 32 2 5 5 52 1952 0 0 0 | 760 = 2 2 32 2 12 12 22 4576 0 0 0 | 1000 = 2 2 32 2 16 16 16 6272 0 0 0
f16 single plain FCX3_TILE=2 256 100352 | 300 = 2 2 64 2 5 5 51 1984 0 0 0 | 760 = 2 2 64 2 12 12 22 4608 0 0 0 | 1000 = 2 2 64 2 16 16 16 6272 0 0 0
bf16x3 single plain FCX3_TILE=5 4096 25088 | 300 = 2 5 32 32 2 -2 2 12544 0 0 0 | 760 = 2 5 32 32 5 -5 4 6272 0 0 0 | 1000 = 2 5 32 32 7 -7 4 6272 0 0 0
f16 single plain FCX3_TILE=5 4096 25088 | 300 = 2 5 64 32 2 -2 2 12544 0 0 0 | 760 = 2 5 64 32 5 -5 4 6272 0 0 0 | 1000 = 2 5 64 32 7 -7 4 6272 0 0 0
bf16x3 single plain FCX3_TILE=5 4096 4096 | 300 = 2 5 32 32 2 -2 2 2048 0 0 0 | 760 = 2 5 32 32 5 -5 4 1024 0 0 0 | 1000 = 2 5 32 32 7 -7 1 4096 0 0 0
f16 single plain FCX3_TILE=5 4096 4096 | 300 = 2 5 64 32 2 -2 2 2048 0 0 0 | 760 = 2 5 64 32 5 -5 4 1024 0 0 0 | 1000 = 2 5 64 32 7 -7 1 4096 0 0 0
bf16x3 single plain FCX3_TILE=5 256 100352 | 300 = 2 5 32 2 2 2 32 3136 0 0 0 | 760 = 2 5 32 2 5 5 25 4032 0 0 0 | 1000 = 2 5 32 2 7 7 9 11168 0 0 0
f16 single plain FCX3_TILE=5 256 100352 | 300 = 2 5 64 2 2 2 32 3136 0 0 0 | 760 = 2 5 64 2 5 5 12 8384 0 0 0 | 1000 = 2 5 64 2 7 7 9 11200 0 0 0
bf16x3 single plain FCX3_TILE=8 4096 25088 | 300 = 3 8 32 16 2 -2 4 6272 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FCX3_TILE=8 4096 25088 | 300 = 3 8 64 16 2 -2 4 6272 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single plain FCX3_TILE=8 4096 4096 | 300 = 3 8 32 16 2 -2 4 1024 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FCX3_TILE=8 4096 4096 | 300 = 3 8 64 16 2 -2 4 1024 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single plain FCX3_TILE=8 256 100352 | 300 = 3 8 32 1 2 2 64 1568 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FCX3_TILE=8 256 100352 | 300 = 3 8 64 1 2 2 63 1600 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 single plain FCX3_TILE=10 4096 25088 | 300 = 2 10 32 32 1 1 4 6272 0 0 0 | 760 = 3 10 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 10 32 16 4 -4 2 12544 0 0 0
f16 single plain FCX3_TILE=10 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 10 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 10 64 16 4 -4 2 12544 0 0 0
bf16x3 single plain FCX3_TILE=10 4096 4096 | 300 = 2 10 32 32 1 1 2 2048 0 0 0 | 760 = 3 10 32 16 3 -3 5 832 0 0 0 | 1000 = 3 10 32 16 4 -4 2 2048 0 0 0
f16 single plain FCX3_TILE=10 4096 4096 | 300 = 2 10 64 32 1 1 2 2048 0 0 0 | 760 = 3 10 64 16 3 -3 5 832 0 0 0 | 1000 = 3 10 64 16 4 -4 2 2048 0 0 0
bf16x3 single plain FCX3_TILE=10 256 100352 | 300 = 2 10 32 2 1 1 49 2048 0 0 0 | 760 = 3 10 32 1 3 3 42 2400 0 0 0 | 1000 = 3 10 32 1 4 4 32 3136 0 0 0
f16 single plain FCX3_TILE=10 256 100352 | 300 = 2 10 64 2 1 1 49 2048 0 0 0 | 760 = 3 10 64 1 3 3 42 2432 0 0 0 | 1000 = 3 10 64 1 4 4 32 3136 0 0 0
bf16x3 single plain FC_NO256=1 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 640: 3 10 32 16 2 -2 4 6272 0 0 0 / 120: 2 5 32 32 1 1 4 6272 0 0 0 | 1000 = 960: 3 10 32 16 3 -3 8 3136 0 0 0 / 40: 2 5 32 32 1 1 4 6272 0 0 0
f16 single plain FC_NO256=1 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 640: 3 10 64 16 2 -2 4 6272 0 0 0 / 120: 2 5 64 32 1 1 4 6272 0 0 0 | 1000 = 960: 3 10 64 16 3 -3 8 3136 0 0 0 / 40: 2 5 64 32 1 1 4 6272 0 0 0
bf16x3 single plain FC_NO256=1 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 640: 2 5 32 32 4 -4 1 4096 0 0 0 / 120: 2 5 32 32 1 1 2 2048 0 0 0 | 1000 = 960: 2 5 32 32 6 -6 2 2048 0 0 0 / 40: 2 2 32 32 1 1 16 256 0 0 0
f16 single plain FC_NO256=1 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 640: 2 5 64 32 4 -4 1 4096 0 0 0 / 120: 2 5 64 32 1 1 2 2048 0 0 0 | 1000 = 960: 2 5 64 32 6 -6 2 2048 0 0 0 / 40: 2 2 64 32 1 1 16 256 0 0 0
bf16x3 single plain FC_NO256=1 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 640: 2 5 32 2 4 4 16 6272 0 0 0 / 120: 2 5 32 2 1 1 49 2048 0 0 0 | 1000 = 960: 3 10 32 1 3 3 42 2400 0 0 0 / 40: 2 5 32 2 1 1 49 2048 0 0 0
f16 single plain FC_NO256=1 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 640: 2 5 64 2 4 4 16 6272 0 0 0 / 120: 2 5 64 2 1 1 49 2048 0 0 0 | 1000 = 960: 3 10 64 1 3 3 42 2432 0 0 0 / 40: 2 5 64 2 1 1 49 2048 0 0 0
bf16x3 single plain FC_RANGE_K=4096 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FC_RANGE_K=4096 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single plain FC_RANGE_K=4096 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FC_RANGE_K=4096 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single plain FC_RANGE_K=4096 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FC_RANGE_K=4096 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 single plain FC_SLOTS=64 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 16 4 -4 1 25088 0 0 0
f16 single plain FC_SLOTS=64 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 16 4 -4 1 25088 0 0 0
bf16x3 single plain FC_SLOTS=64 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 16 4 -4 1 4096 0 0 0
f16 single plain FC_SLOTS=64 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 4 1024 0 0 0 | 1000 = 3 8 64 16 4 -4 1 4096 0 0 0
bf16x3 single plain FC_SLOTS=64 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 3 8 32 1 3 3 21 4800 0 0 0 | 1000 = 3 8 32 1 4 4 16 6272 0 0 0
f16 single plain FC_SLOTS=64 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 3 8 64 1 3 3 21 4800 0 0 0 | 1000 = 3 8 64 1 4 4 16 6272 0 0 0
bf16x3 single plain FC_SLOTS=256 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 5 5024 0 0 0 | 1000 = 3 8 32 16 4 -4 4 6272 0 0 0
f16 single plain FC_SLOTS=256 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 -3 5 5056 0 0 0 | 1000 = 3 8 64 16 4 -4 4 6272 0 0 0
bf16x3 single plain FC_SLOTS=256 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 4 1024 0 0 0
f16 single plain FC_SLOTS=256 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 4 1024 0 0 0
bf16x3 single plain FC_SLOTS=256 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 3 8 32 1 3 3 85 1184 0 0 0 | 1000 = 3 8 32 1 4 4 64 1568 0 0 0
f16 single plain FC_SLOTS=256 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 3 8 64 1 3 3 83 1216 0 0 0 | 1000 = 3 8 64 1 4 4 63 1600 0 0 0
bf16x3 single plain FC_ORDER=0 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 4 2 12544 0 0 0
f16 single plain FC_ORDER=0 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 4 2 12544 0 0 0
bf16x3 single plain FC_ORDER=0 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 3 8 32 16 3 3 5 832 0 0 0 | 1000 = 3 8 32 16 4 4 2 2048 0 0 0
f16 single plain FC_ORDER=0 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 3 8 64 16 3 3 5 832 0 0 0 | 1000 = 3 8 64 16 4 4 2 2048 0 0 0
bf16x3 single plain FC_ORDER=0 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FC_ORDER=0 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 single plain FC_ORDER=1 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FC_ORDER=1 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single plain FC_ORDER=1 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FC_ORDER=1 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single plain FC_ORDER=1 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 3 8 32 1 3 -3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 -4 32 3136 0 0 0
f16 single plain FC_ORDER=1 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 3 8 64 1 3 -3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 -4 32 3136 0 0 0
bf16x3 single plain FCX3_WIDE=0 4096 25088 | 300 = 2 10 32 32 1 1 4 6272 0 0 0 | 760 = 2 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 2 8 32 32 4 -4 1 25088 0 0 0
f16 single plain FCX3_WIDE=0 4096 25088 | 300 = 2 10 64 32 1 1 4 6272 0 0 0 | 760 = 2 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 2 8 64 32 4 -4 1 25088 0 0 0
bf16x3 single plain FCX3_WIDE=0 4096 4096 | 300 = 2 5 32 32 2 -2 2 2048 0 0 0 | 760 = 2 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 2 8 32 32 4 -4 1 4096 0 0 0
f16 single plain FCX3_WIDE=0 4096 4096 | 300 = 2 5 64 32 2 -2 2 2048 0 0 0 | 760 = 2 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 2 8 64 32 4 -4 1 4096 0 0 0
bf16x3 single plain FCX3_WIDE=0 256 100352 | 300 = 2 5 32 2 2 2 32 3136 0 0 0 | 760 = 2 8 32 2 3 3 21 4800 0 0 0 | 1000 = 2 8 32 2 4 4 16 6272 0 0 0
f16 single plain FCX3_WIDE=0 256 100352 | 300 = 2 5 64 2 2 2 32 3136 0 0 0 | 760 = 2 8 64 2 3 3 21 4800 0 0 0 | 1000 = 2 8 64 2 4 4 16 6272 0 0 0
bf16x3 single plain FCX3_WIDE=1 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FCX3_WIDE=1 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single plain FCX3_WIDE=1 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FCX3_WIDE=1 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single plain FCX3_WIDE=1 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FCX3_WIDE=1 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 single plain FUSE_SMALL=0 4096 25088 | 300 = 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 16 4 -4 2 12544 0 0 0
f16 single plain FUSE_SMALL=0 4096 25088 | 300 = 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 single plain FUSE_SMALL=0 4096 4096 | 300 = 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 3 8 32 16 4 -4 2 2048 0 0 0
f16 single plain FUSE_SMALL=0 4096 4096 | 300 = 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 single plain FUSE_SMALL=0 256 100352 | 300 = 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 3 8 32 1 4 4 32 3136 0 0 0
f16 single plain FUSE_SMALL=0 256 100352 | 300 = 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 pair pre - 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 640 = 3 10 32 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair pre - 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 640 = 3 10 64 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair pre - 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 640 = 3 10 32 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair pre - 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 640 = 3 10 64 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair osm - 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 640 = 3 10 32 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair osm - 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 640 = 3 10 64 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair osm - 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 640 = 3 10 32 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair osm - 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 640 = 3 10 64 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair pre+osm - 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 640 = 3 10 32 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair pre+osm - 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 640 = 3 10 64 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair pre+osm - 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 640 = 3 10 32 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair pre+osm - 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 640 = 3 10 64 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair pre+ld2 - 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 640 = 3 10 32 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair pre+ld2 - 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 640 = 3 10 64 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair pre+ld2 - 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 640 = 3 10 32 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair pre+ld2 - 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 640 = 3 10 64 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair osm+ld2 - 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 640 = 3 10 32 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 2 12544 0 0 0
f16 pair osm+ld2 - 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 640 = 3 10 64 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 2 12544 0 0 0
bf16x3 pair osm+ld2 - 4096 4096 | 300 = 3 10 32 32 1 1 2 2048 0 0 0 | 640 = 3 10 32 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 2 2048 0 0 0
f16 pair osm+ld2 - 4096 4096 | 300 = 3 10 64 32 1 1 2 2048 0 0 0 | 640 = 3 10 64 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 2 2048 0 0 0
bf16x3 pair pre+osm+ld2 - 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 640 = 3 10 32 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 2 12544 0 0 0
f16 pair pre+osm+ld2 - 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 640 = 3 10 64 32 2 -2 2 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 2 12544 0 0 0
bf16x3 pair pre+osm+ld2 - 4096 4096 | 300 = 3 10 32 32 1 1 2 2048 0 0 0 | 640 = 3 10 32 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 2 2048 0 0 0
f16 pair pre+osm+ld2 - 4096 4096 | 300 = 3 10 64 32 1 1 2 2048 0 0 0 | 640 = 3 10 64 32 2 -2 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 2 2048 0 0 0
bf16x3 pair plain PLAN=1 4096 25088 | 300 = 3 10 32 32 1 1 8 3136 0 0 0 | 760 = 2x 760: 3 8 32 16 3 -3 5 5024 0 0 0 | 1000 = 2x 1000: 3 8 32 16 4 -4 4 6272 0 0 0
f16 pair plain PLAN=1 4096 25088 | 300 = 3 10 64 32 1 1 8 3136 0 0 0 | 760 = 2x 760: 3 8 64 16 3 -3 5 5056 0 0 0 | 1000 = 2x 1000: 3 8 64 16 4 -4 4 6272 0 0 0
bf16x3 pair plain PLAN=1 4096 4096 | 300 = 3 10 32 32 1 1 8 512 0 0 0 | 760 = 2x 760: 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 2x 1000: 3 8 32 16 4 -4 4 1024 0 0 0
f16 pair plain PLAN=1 4096 4096 | 300 = 3 10 64 32 1 1 8 512 0 0 0 | 760 = 2x 760: 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 2x 1000: 3 8 64 16 4 -4 4 1024 0 0 0
bf16x3 pair plain PLAN=1 256 100352 | 300 = 2x 300: 2 5 32 2 2 2 64 1568 0 0 0 | 760 = 2x 760: 2 8 32 2 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 2 8 32 2 4 4 32 3136 0 0 0
f16 pair plain PLAN=1 256 100352 | 300 = 2x 300: 2 5 64 2 2 2 63 1600 0 0 0 | 760 = 2x 760: 2 8 64 2 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 2 8 64 2 4 4 32 3136 0 0 0
bf16x3 pair plain FCX3_TILE=2 4096 25088 | 300 = 2x 300: 2 2 32 32 5 -5 4 6272 0 0 0 | 760 = 2x 760: 2 2 32 32 12 -12 2 12544 0 0 0 | 1000 = 2x 1000: 2 2 32 32 16 -16 1 25088 0 0 0
f16 pair plain FCX3_TILE=2 4096 25088 | 300 = 2x 300: 2 2 64 32 5 -5 4 6272 0 0 0 | 760 = 2x 760: 2 2 64 32 12 -12 2 12544 0 0 0 | 1000 = 2x 1000: 2 2 64 32 16 -16 1 25088 0 0 0
bf16x3 pair plain FCX3_TILE=2 4096 4096 | 300 = 2x 300: 2 2 32 32 5 -5 4 1024 0 0 0 | 760 = 2x 760: 2 2 32 32 12 -12 2 2048 0 0 0 | 1000 = 2x 1000: 2 2 32 32 16 -16 1 4096 0 0 0
f16 pair plain FCX3_TILE=2 4096 4096 | 300 = 2x 300: 2 2 64 32 5 -5 4 1024 0 0 0 | 760 = 2x 760: 2 2 64 32 12 -12 2 2048 0 0 0 | 1000 = 2x 1000: 2 2 64 32 16 -16 1 4096 0 0 0
bf16x3 pair plain FCX3_TILE=2 256 100352 | 300 = 2x 300: 2 2 32 2 5 5 52 1952 0 0 0 | 760 = 2x 760: 2 2 32 2 12 12 22 4576 0 0 0 | 1000 = 2x 1000: 2 2 32 2 16 16 16 6272 0 0 0
f16 pair plain FCX3_TILE=2 256 100352 | 300 = 2x 300: 2 2 64 2 5 5 51 1984 0 0 0 | 760 = 2x 760: 2 2 64 2 12 12 22 4608 0 0 0 | 1000 = 2x 1000: 2 2 64 2 16 16 16 6272 0 0 0
bf16x3 pair plain FCX3_TILE=5 4096 25088 | 300 = 2x 300: 2 5 32 32 2 -2 2 12544 0 0 0 | 760 = 2x 760: 2 5 32 32 5 -5 4 6272 0 0 0 | 1000 = 2x 1000: 2 5 32 32 7 -7 4 6272 0 0 0
f16 pair plain FCX3_TILE=5 4096 25088 | 300 = 2x 300: 2 5 64 32 2 -2 2 12544 0 0 0 | 760 = 2x 760: 2 5 64 32 5 -5 4 6272 0 0 0 | 1000 = 2x 1000: 2 5 64 32 7 -7 4 6272 0 0 0
bf16x3 pair plain FCX3_TILE=5 4096 4096 | 300 = 2x 300: 2 5 32 32 2 -2 2 2048 0 0 0 | 760 = 2x 760: 2 5 32 32 5 -5 4 1024 0 0 0 | 1000 = 2x 1000: 2 5 32 32 7 -7 1 4096 0 0 0
f16 pair plain FCX3_TILE=5 4096 4096 | 300 = 2x 300: 2 5 64 32 2 -2 2 2048 0 0 0 | 760 = 2x 760: 2 5 64 32 5 -5 4 1024 0 0 0 | 1000 = 2x 1000: 2 5 64 32 7 -7 1 4096 0 0 0
bf16x3 pair plain FCX3_TILE=5 256 100352 | 300 = 2x 300: 2 5 32 2 2 2 32 3136 0 0 0 | 760 = 2x 760: 2 5 32 2 5 5 25 4032 0 0 0 | 1000 = 2x 1000: 2 5 32 2 7 7 9 11168 0 0 0
f16 pair plain FCX3_TILE=5 256 100352 | 300 = 2x 300: 2 5 64 2 2 2 32 3136 0 0 0 | 760 = 2x 760: 2 5 64 2 5 5 12 8384 0 0 0 | 1000 = 2x 1000: 2 5 64 2 7 7 9 11200 0 0 0
bf16x3 pair plain FCX3_TILE=8 4096 25088 | 300 = 2x 300: 3 8 32 16 2 -2 4 6272 0 0 0 | 760 = 2x 760: 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 2x 1000: 3 8 32 16 4 -4 2 12544 0 0 0
f16 pair plain FCX3_TILE=8 4096 25088 | 300 = 2x 300: 3 8 64 16 2 -2 4 6272 0 0 0 | 760 = 2x 760: 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 2x 1000: 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 pair plain FCX3_TILE=8 4096 4096 | 300 = 2x 300: 3 8 32 16 2 -2 4 1024 0 0 0 | 760 = 2x 760: 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 2x 1000: 3 8 32 16 4 -4 2 2048 0 0 0
f16 pair plain FCX3_TILE=8 4096 4096 | 300 = 2x 300: 3 8 64 16 2 -2 4 1024 0 0 0 | 760 = 2x 760: 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 2x 1000: 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 pair plain FCX3_TILE=8 256 100352 | 300 = 2x 300: 3 8 32 1 2 2 64 1568 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FCX3_TILE=8 256 100352 | 300 = 2x 300: 3 8 64 1 2 2 63 1600 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 pair plain FCX3_TILE=10 4096 25088 | 300 = 2x 300: 2 10 32 32 1 1 4 6272 0 0 0 | 760 = 2x 760: 3 10 32 16 3 -3 8 3136 0 0 0 | 1000 = 2x 1000: 3 10 32 16 4 -4 2 12544 0 0 0
f16 pair plain FCX3_TILE=10 4096 25088 | 300 = 2x 300: 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 2x 760: 3 10 64 16 3 -3 8 3136 0 0 0 | 1000 = 2x 1000: 3 10 64 16 4 -4 2 12544 0 0 0
bf16x3 pair plain FCX3_TILE=10 4096 4096 | 300 = 2x 300: 2 10 32 32 1 1 2 2048 0 0 0 | 760 = 2x 760: 3 10 32 16 3 -3 5 832 0 0 0 | 1000 = 2x 1000: 3 10 32 16 4 -4 2 2048 0 0 0
f16 pair plain FCX3_TILE=10 4096 4096 | 300 = 2x 300: 2 10 64 32 1 1 2 2048 0 0 0 | 760 = 2x 760: 3 10 64 16 3 -3 5 832 0 0 0 | 1000 = 2x 1000: 3 10 64 16 4 -4 2 2048 0 0 0
bf16x3 pair plain FCX3_TILE=10 256 100352 | 300 = 2x 300: 2 10 32 2 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 10 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 10 32 1 4 4 32 3136 0 0 0
f16 pair plain FCX3_TILE=10 256 100352 | 300 = 2x 300: 2 10 64 2 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 10 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 10 64 1 4 4 32 3136 0 0 0
bf16x3 pair plain FC_NO256=1 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 760 = 2x 640: 3 10 32 16 2 -2 4 6272 0 0 0 / 120: 2 5 32 32 1 1 4 6272 0 0 0 | 1000 = 2x 960: 3 10 32 16 3 -3 8 3136 0 0 0 / 40: 2 5 32 32 1 1 4 6272 0 0 0
f16 pair plain FC_NO256=1 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 760 = 2x 640: 3 10 64 16 2 -2 4 6272 0 0 0 / 120: 2 5 64 32 1 1 4 6272 0 0 0 | 1000 = 2x 960: 3 10 64 16 3 -3 8 3136 0 0 0 / 40: 2 5 64 32 1 1 4 6272 0 0 0
bf16x3 pair plain FC_NO256=1 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 760 = 2x 640: 2 5 32 32 4 -4 1 4096 0 0 0 / 120: 2 5 32 32 1 1 2 2048 0 0 0 | 1000 = 2x 960: 2 5 32 32 6 -6 2 2048 0 0 0 / 40: 2 2 32 32 1 1 16 256 0 0 0
f16 pair plain FC_NO256=1 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 760 = 2x 640: 2 5 64 32 4 -4 1 4096 0 0 0 / 120: 2 5 64 32 1 1 2 2048 0 0 0 | 1000 = 2x 960: 2 5 64 32 6 -6 2 2048 0 0 0 / 40: 2 2 64 32 1 1 16 256 0 0 0
bf16x3 pair plain FC_NO256=1 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 640: 2 5 32 2 4 4 16 6272 0 0 0 / 120: 2 5 32 2 1 1 49 2048 0 0 0 | 1000 = 2x 960: 3 10 32 1 3 3 42 2400 0 0 0 / 40: 2 5 32 2 1 1 49 2048 0 0 0
f16 pair plain FC_NO256=1 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 640: 2 5 64 2 4 4 16 6272 0 0 0 / 120: 2 5 64 2 1 1 49 2048 0 0 0 | 1000 = 2x 960: 3 10 64 1 3 3 42 2432 0 0 0 / 40: 2 5 64 2 1 1 49 2048 0 0 0
bf16x3 pair plain FC_RANGE_K=4096 4096 25088 | 300 = 3 10 32 32 1 1 4 6272 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FC_RANGE_K=4096 4096 25088 | 300 = 3 10 64 32 1 1 4 6272 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair plain FC_RANGE_K=4096 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FC_RANGE_K=4096 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair plain FC_RANGE_K=4096 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FC_RANGE_K=4096 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 pair plain FC_SLOTS=64 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 760 = 3 8 32 32 3 -3 2 12544 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FC_SLOTS=64 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 760 = 3 8 64 32 3 -3 2 12544 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair plain FC_SLOTS=64 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 760 = 3 8 32 32 3 -3 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FC_SLOTS=64 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 760 = 3 8 64 32 3 -3 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair plain FC_SLOTS=64 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 21 4800 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 16 6272 0 0 0
f16 pair plain FC_SLOTS=64 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 21 4800 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 16 6272 0 0 0
bf16x3 pair plain FC_SLOTS=256 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 760 = 3 8 32 32 3 -3 8 3136 0 0 0 | 1000 = 3 8 32 32 4 -4 2 12544 0 0 0
f16 pair plain FC_SLOTS=256 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 760 = 3 8 64 32 3 -3 5 5056 0 0 0 | 1000 = 3 8 64 32 4 -4 2 12544 0 0 0
bf16x3 pair plain FC_SLOTS=256 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 760 = 3 8 32 32 3 -3 2 2048 0 0 0 | 1000 = 3 8 32 32 4 -4 2 2048 0 0 0
f16 pair plain FC_SLOTS=256 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 760 = 3 8 64 32 3 -3 2 2048 0 0 0 | 1000 = 3 8 64 32 4 -4 2 2048 0 0 0
bf16x3 pair plain FC_SLOTS=256 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 85 1184 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 64 1568 0 0 0
f16 pair plain FC_SLOTS=256 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 83 1216 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 63 1600 0 0 0
bf16x3 pair plain FC_ORDER=0 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FC_ORDER=0 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair plain FC_ORDER=0 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FC_ORDER=0 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair plain FC_ORDER=0 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FC_ORDER=0 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 pair plain FC_ORDER=1 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FC_ORDER=1 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair plain FC_ORDER=1 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FC_ORDER=1 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair plain FC_ORDER=1 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 32 1 3 -3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 -4 32 3136 0 0 0
f16 pair plain FC_ORDER=1 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 64 1 3 -3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 -4 32 3136 0 0 0
bf16x3 pair plain FCX3_WIDE=0 4096 25088 | 300 = 2x 300: 2 10 32 32 1 1 4 6272 0 0 0 | 760 = 2x 760: 2 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 2x 1000: 2 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FCX3_WIDE=0 4096 25088 | 300 = 2x 300: 2 10 64 32 1 1 4 6272 0 0 0 | 760 = 2x 760: 2 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 2x 1000: 2 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair plain FCX3_WIDE=0 4096 4096 | 300 = 2x 300: 2 5 32 32 2 -2 2 2048 0 0 0 | 760 = 2x 760: 2 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 2x 1000: 2 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FCX3_WIDE=0 4096 4096 | 300 = 2x 300: 2 5 64 32 2 -2 2 2048 0 0 0 | 760 = 2x 760: 2 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 2x 1000: 2 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair plain FCX3_WIDE=0 256 100352 | 300 = 2x 300: 2 5 32 2 2 2 32 3136 0 0 0 | 760 = 2x 760: 2 8 32 2 3 3 21 4800 0 0 0 | 1000 = 2x 1000: 2 8 32 2 4 4 16 6272 0 0 0
f16 pair plain FCX3_WIDE=0 256 100352 | 300 = 2x 300: 2 5 64 2 2 2 32 3136 0 0 0 | 760 = 2x 760: 2 8 64 2 3 3 21 4800 0 0 0 | 1000 = 2x 1000: 2 8 64 2 4 4 16 6272 0 0 0
bf16x3 pair plain FCX3_WIDE=1 4096 25088 | 300 = 3 10 32 32 1 1 2 12544 0 0 0 | 760 = 3 8 32 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 32 32 4 -4 1 25088 0 0 0
f16 pair plain FCX3_WIDE=1 4096 25088 | 300 = 3 10 64 32 1 1 2 12544 0 0 0 | 760 = 3 8 64 32 3 -3 4 6272 0 0 0 | 1000 = 3 8 64 32 4 -4 1 25088 0 0 0
bf16x3 pair plain FCX3_WIDE=1 4096 4096 | 300 = 3 10 32 32 1 1 1 4096 0 0 0 | 760 = 3 8 32 32 3 -3 4 1024 0 0 0 | 1000 = 3 8 32 32 4 -4 1 4096 0 0 0
f16 pair plain FCX3_WIDE=1 4096 4096 | 300 = 3 10 64 32 1 1 1 4096 0 0 0 | 760 = 3 8 64 32 3 -3 1 4096 0 0 0 | 1000 = 3 8 64 32 4 -4 1 4096 0 0 0
bf16x3 pair plain FCX3_WIDE=1 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FCX3_WIDE=1 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
bf16x3 pair plain FUSE_SMALL=0 4096 25088 | 300 = 2x 300: 3 10 32 16 1 1 8 3136 0 0 0 | 760 = 2x 760: 3 8 32 16 3 -3 8 3136 0 0 0 | 1000 = 2x 1000: 3 8 32 16 4 -4 2 12544 0 0 0
f16 pair plain FUSE_SMALL=0 4096 25088 | 300 = 2x 300: 3 10 64 16 1 1 8 3136 0 0 0 | 760 = 2x 760: 3 8 64 16 3 -3 8 3136 0 0 0 | 1000 = 2x 1000: 3 8 64 16 4 -4 2 12544 0 0 0
bf16x3 pair plain FUSE_SMALL=0 4096 4096 | 300 = 2x 300: 3 10 32 16 1 1 2 2048 0 0 0 | 760 = 2x 760: 3 8 32 16 3 -3 5 832 0 0 0 | 1000 = 2x 1000: 3 8 32 16 4 -4 2 2048 0 0 0
f16 pair plain FUSE_SMALL=0 4096 4096 | 300 = 2x 300: 3 10 64 16 1 1 2 2048 0 0 0 | 760 = 2x 760: 3 8 64 16 3 -3 5 832 0 0 0 | 1000 = 2x 1000: 3 8 64 16 4 -4 2 2048 0 0 0
bf16x3 pair plain FUSE_SMALL=0 256 100352 | 300 = 2x 300: 3 10 32 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 32 1 3 3 42 2400 0 0 0 | 1000 = 2x 1000: 3 8 32 1 4 4 32 3136 0 0 0
f16 pair plain FUSE_SMALL=0 256 100352 | 300 = 2x 300: 3 10 64 1 1 1 49 2048 0 0 0 | 760 = 2x 760: 3 8 64 1 3 3 42 2432 0 0 0 | 1000 = 2x 1000: 3 8 64 1 4 4 32 3136 0 0 0
"""
