#!/usr/bin/env python
"""CPU: the sequence of library calls mnc_amd.engine.Net makes, as one sha256 per case -- the check that a change to the engine's
host code leaves what the library sees as it was.  The C ABI is the test double of tests/fake_backend.py; every call's entry name
and arguments are recorded, an address inside a buffer the double handed out as (ordinal of the allocation, offset), any other
address as one fixed token.

A case is (graph, math, winograd, fuse, _X3_MIN_FLOPS default or 0): construction, a forward at 96x160, one at 130x203, one
detect_image at 40x56 where the graph ends in the MNC heads, close.  Entries the double does not emulate (the bf16 / f8 packers and
InnerProducts ...) are no-ops here: those cases trace the plan without its arithmetic.  Two more cases ('-split') run the fp32
F(4x4) graph as on a library that selects the unfused split form for every layer.

    python tools/engine_call_trace.py [--only SUBSTRING] [--dump DIR]
Compare two commits by running it at both: every line of the output must be equal."""
import argparse
import bisect
import ctypes
import gc
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fake_backend                                                    # noqa: E402
import test_engine_host_logic as T                                     # noqa: E402  (its fixed inputs)
from mnc_amd import _lib, engine, models, synth                        # noqa: E402

GRAPHS = {"mnc5": models.write_mnc_5stage_test_prototxt, "cfm": models.write_cfm_test_prototxt,
          "resnet50": models.write_mnc_resnet50_test_prototxt}
MODES = [("fp32", 0), ("fp32", 2), ("fp32", 4), ("bf16x3", 4), ("f16", 4), ("mixed", 4), ("bf16", 4), ("f8", 4)]
ADDRESS = 1 << 32                    # no count, size or stride the engine passes reaches this; every heap address is above it


class _Patch(object):
    """The setattr half of pytest's monkeypatch, which fake_backend.install expects."""

    def __init__(self):
        self._saved = []

    def setattr(self, obj, name, value):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def undo(self):
        for obj, name, value in reversed(self._saved):
            setattr(obj, name, value)


class _Sizes(object):
    """What the engine reads off _lib.load() directly: size functions (any deterministic answer serves a trace)."""

    @staticmethod
    def mnc_pack_fc_f8_bytes(n_out, K):
        return (n_out + 255) // 256 * 256 * K


class _SplitSizes(_Sizes):
    """... and a library that moves every F(4x4) layer to the unfused split form (the double has none: the '-split' cases)."""

    @staticmethod
    def mnc_conv3x3_wino4_split_selected(h, H, W, cin, cout):
        return 1

    @staticmethod
    def mnc_conv3x3_wino4_split_ws_bytes(H, W, cin, cout):
        return 36 * ((H + 3) // 4) * ((W + 3) // 4) * (cin + cout) * 4


class Tracer(object):
    def __init__(self, patch, split=False):
        self.fake = fake_backend.install(patch)
        self.fake.mnc_fc_bf16 = lambda *args: None         # (the double's mnc_fc_bf16_ex calls it and has none)
        self.inner = _lib.call
        self.lines, self.bases, self.live, self.count = [], [], {}, 0
        patch.setattr(_lib, "call", self.call)
        patch.setattr(_lib, "load", lambda: _SplitSizes if split else _Sizes)

    def _arg(self, a):
        if a is None or isinstance(a, (str, bytes)):
            return repr(a)
        if isinstance(a, (float, np.floating)):
            return repr(float(a))
        a = int(a)
        if abs(a) < ADDRESS:
            return str(a)
        i = bisect.bisect_right(self.bases, a) - 1
        if i >= 0:
            ordinal, size = self.live[self.bases[i]]
            if a - self.bases[i] <= size:
                return "(%d+%d)" % (ordinal, a - self.bases[i])
        return "ADDR"

    def call(self, name, *args):
        self.lines.append("%s %s" % (name, " ".join(self._arg(a) for a in args)))
        if hasattr(self.fake, name):
            self.inner(name, *args)
        if name in ("mnc_dev_alloc", "mnc_host_alloc"):
            base = ctypes.c_void_p.from_address(int(args[2])).value
            bisect.insort(self.bases, base)
            self.live[base] = (self.count, int(args[1]))
            self.lines[-1] += " -> %d" % self.count
            self.count += 1
        elif name in ("mnc_dev_free", "mnc_host_free") and int(args[1]) in self.live:
            del self.live[int(args[1])]
            self.bases.remove(int(args[1]))
        return 0


def run_case(graph, math, wino, fuse, x3_zero, split=False):
    patch = _Patch()
    tr = Tracer(patch, split)
    if x3_zero:
        patch.setattr(engine, "_X3_MIN_FLOPS", 0.0)
    try:
        path = GRAPHS[graph](width_div=8)
        net = engine.Net(path, synth.synthetic_weights(path, seed=1), 1, device_id=0, fuse=fuse, math=math, winograd=wino)
        for seed, (H, W) in enumerate([(96, 160), (130, 203)]):
            tr.lines.append("# forward %dx%d" % (H, W))
            if graph == "cfm":
                data, rois, masks = T._cfm_inputs(seed, 2, H, W, 37)
                net.forward(data=data, rois=rois, masks=masks)
            else:
                data, im_info = T._inputs(H, W, seed)
                net.forward(data=data, im_info=im_info)
        if graph != "cfm":
            tr.lines.append("# detect_image 40x56")
            net.detect_image(np.random.default_rng(0).integers(0, 256, (40, 56, 3), dtype=np.uint8), use_graph=False)
        tr.lines.append("# close")
        net.close()
    except Exception as e:                                 # a case the engine refuses is part of its behaviour too
        tr.lines.append("# raised %s: %s" % (type(e).__name__, e))
    finally:
        lines, tr.lines = tr.lines, []                     # a Net that a raising case left open is finalised here, off the record
        net = None
        gc.collect()
        patch.undo()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    ap.add_argument("--dump", default=None, help="write each case's trace to DIR/<case>.txt")
    args = ap.parse_args()
    for k in [k for k in os.environ if k.startswith("MNC_")]:
        del os.environ[k]
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    cases = [(g, m, w, f, z, False) for g in GRAPHS for m, w in MODES for f in (True, False) for z in (False, True)]
    cases += [("mnc5", "fp32", 4, f, False, True) for f in (True, False)]          # the unfused F(4x4) form, with and without pool
    for graph, math, wino, fuse, x3_zero, split in cases:
        name = "%s-%s-wino%d-%s-%s%s" % (graph, math, wino, "fuse" if fuse else "nofuse", "x3min0" if x3_zero else "x3min",
                                         "-split" if split else "")
        if args.only not in name:
            continue
        lines = run_case(graph, math, wino, fuse, x3_zero, split)
        if args.dump:
            with open(os.path.join(args.dump, name + ".txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        print("%s %s %d" % (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], name, len(lines)), flush=True)


if __name__ == "__main__":
    main()
