"""GPU: the host-array entry points (one per-device stream and workspace behind a mutex, HostScope::open; mnc_last_error is
thread_local) the way a dataset evaluation or a loader with worker threads calls them.

(1) Under GPU contention: contours, components, fill_holes, RLE and NMS at n = 6000 while the disturbers of tests/contention.py
(mnc_fc 300 x 4096 x 4096 and mnc_add over 3 x 256 MB on contexts of their own; there is no twin: the entry points share ONE stream)
keep the CUs and the memory system busy.  These kernels iterate with atomics and flags across workgroups and launches.  16 calls
alone, then 16 calls each behind a pre-roll of disturber launches that covers three times the slowest solo call; every result equals
its numpy statement or oracle.native byte for byte; at least half of the contended calls must have taken longer than the slowest solo
call, or the test fails.  Durations: the task's own timing span (mnc_mask_components_timing, mnc_mask_contours_timing) where the
task has one, the wall time of the call for mnc_mask_rle and mnc_nms, which have none: that figure includes Python, the host copies
and the final synchronisation, so for those five cases "disturbed" says that the call was delayed, not which kernel -- weaker evidence.

(2) From four host threads at once (ctypes releases the GIL): 12 calls each of contours, components, RLE and NMS, the inputs
alternating between a small and a large set so that the shared workspace is re-grown while other threads wait at its mutex.

Measured on an MI355X, one run (disturbed calls of 16, median contended / median solo duration, wall time of the test):
  entry point      checker              seam                 many                 real
  contours         16  1.65x  0.07 s    16  4.87x  0.03 s    16  4.30x  0.17 s    16  3.41x  0.09 s
  components       16  3.07x  0.05 s    16  4.30x  0.02 s    16  3.56x  0.06 s    16  2.54x  0.04 s
  fill_holes       16  5.65x  0.03 s    16  5.31x  0.02 s    16  4.09x  0.06 s    16  3.11x  0.05 s
  rle              16  1.83x  0.02 s    16  1.85x  0.02 s    16  2.73x  0.22 s    16  2.63x  0.04 s
  nms n = 6000     16  2.18x  0.28 s
  four host threads, 48 calls and 4 refusals: 0.02 s
"""
import os
import sys
import threading

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import contention as CN  # noqa: E402
import golden_inputs as GI  # noqa: E402
import mask_components_inputs as CI  # noqa: E402
import mask_contours_inputs as TI  # noqa: E402
from mnc_amd import _lib, rle  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402
from oracle import native  # noqa: E402

pytestmark = pytest.mark.gpu

SETS = ["checker", "seam", "many", "real"]
NMS_N, NMS_THR = 6000, 0.7
_RLE, _NMS = {}, {}


@pytest.fixture(scope="module")
def disturbers():
    d = CN.Disturbers(("compute", "bandwidth"))        # (no twin: these entry points have one stream)
    yield d
    d.close()


def rle_reference(name):
    """rle_counts_numpy of the set on the smallest image that holds it, computed once."""
    if name not in _RLE:
        pm = TI.get(name)
        H, W = TI.image_size(pm)
        _RLE[name] = (H, W, rle.rle_counts_numpy(pm, H, W))
    return _RLE[name]


def nms_reference(n, seed):
    if (n, seed) not in _NMS:
        dets = GI.nms_case(n, seed)
        _NMS[(n, seed)] = (dets, native.gpu_nms(dets, NMS_THR))
    return _NMS[(n, seed)]


def same_rle(got, want):
    return all(TI.same_array(g, w) for g, w in zip(got, want))


# ---- the entry points on a named input: reference (made once, on the CPU), call, comparison ----
def nms_call(key):
    from nms.gpu_nms import gpu_nms
    return gpu_nms(nms_reference(*key)[0], NMS_THR, 0)


REF = {"contours": lambda name: TI.reference(name, 8), "components": lambda name: CI.reference(name, "components", 8),
       "fill_holes": lambda name: CI.reference(name, "fill_holes", 4), "rle": lambda name: rle_reference(name)[2],
       "nms": lambda key: nms_reference(*key)[1]}
CALL = {"contours": lambda name: CT.contours(TI.get(name), 8), "components": lambda name: TI.get(name).components(8),
        "fill_holes": lambda name: TI.get(name).fill_holes(4),
        "rle": lambda name: rle.rle_counts(TI.get(name), rle_reference(name)[0], rle_reference(name)[1]), "nms": nms_call}
SAME = {"contours": TI.same_contours, "components": CI.same_components, "fill_holes": CI.same_masks, "rle": same_rle,
        "nms": lambda a, b: list(a) == list(b)}
TIMERS = {"contours": "mnc_mask_contours_timing", "components": "mnc_mask_components_timing", "fill_holes": "mnc_mask_components_timing"}


def contended(disturbers, op, arg):
    what, timer = "%s %s" % (op, arg), TIMERS.get(op)
    want = REF[op](arg)                                # (the reference is made before anything is timed)

    def check(k, got):
        if not SAME[op](got, want):
            pytest.fail("%s, call %d: the result differs from its statement" % (what, k))

    def call(k):
        if timer:
            _lib.timing(timer, 1)                      # switching on forgets the kept figure: none of an earlier call is left
        return CALL[op](arg)

    def timed_ms():
        if timer is None:
            return None
        ms = _lib.timing(timer, 1)                     # the figure of the call just made (-1.0 if its span kept none), forgotten again
        assert ms >= 0.0, "%s: the call kept no timing" % what
        return ms
    try:
        CN.contended_call(disturbers, call, timed_ms, what, check)
    finally:
        if timer:
            _lib.timing(timer, 0)


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("op", ["contours", "components", "fill_holes", "rle"])
def test_mask_entry_points_under_contention(disturbers, op, name):
    """Hazard: flags and atomics that one launch leaves for the next (union-find rounds, the jumping rounds of the outlines, the
    scans of the run counts) while other streams delay and interleave with the launches."""
    contended(disturbers, op, name)


def test_nms_under_contention(disturbers):
    """gpu_nms at n = 6000 (the bitmask kernel and the single-wave scan) against oracle.native."""
    contended(disturbers, "nms", (NMS_N, 31))


# ---- four host threads ----
CALLS = 12
REFUSAL = "mnc_mask_contours: connectivity=6 is not 4 or 8"


def refused_call():
    """mnc_mask_contours with connectivity=6 on a valid set of two 10 x 10 masks: refused before anything is launched."""
    bounds = np.array([[0, 0, 9, 9], [0, 0, 9, 9]], np.int32)
    offsets, bits = np.array([0, 80], np.int64), np.full(20, (1 << 10) - 1, np.uint64)
    outs = [np.zeros(2100, np.int64), np.zeros(9, np.int64), np.zeros(8, np.int64), np.zeros((64, 2), np.int32), np.zeros(1, np.uint64),
            np.zeros(1, np.uint64)]
    p = [_lib.ptr(o) for o in outs]
    lib = _lib.load()
    rc = lib.mnc_mask_contours(_lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(bits), bits.nbytes, 2, 6, p[0], p[1], p[2], p[3], 8, 64, p[4],
                               p[5], 0)
    return rc, lib.mnc_last_error().decode()


def test_four_host_threads_share_the_workspace_and_keep_their_own_errors():
    """Four threads, 12 calls each of contours / components / RLE / NMS, small and large inputs alternating: every result equals its
    statement, every valid call leaves an empty mnc_last_error on its own thread, and the thread that interleaves a refused call
    (connectivity=6) reads exactly its own message.  Hazard: the shared per-device stream and workspace (re-grown under the mutex
    while others wait), thread_local error text."""
    plan = {"contours": ("contours", ["seam", "real"]), "components": ("components", ["seam", "real"]),
            "rle": ("rle", ["seam", "real"]), "nms": ("nms", [(64, 34), (NMS_N, 31)])}
    for op, args in plan.values():                     # the references on the CPU; the first large call of a thread may grow the workspace
        for a in args:
            REF[op](a)
    lib = _lib.load()
    problems, done = [], []
    go = threading.Barrier(len(plan))

    def worker(tag, op, args):
        try:
            go.wait(timeout=30)
            for k in range(CALLS):
                if not SAME[op](CALL[op](args[k & 1]), REF[op](args[k & 1])):
                    problems.append("%s call %d (%s): the result differs from its statement" % (tag, k, args[k & 1]))
                err = lib.mnc_last_error().decode()
                if err:
                    problems.append("%s call %d: a valid call left the message %r" % (tag, k, err))
                if tag == "contours" and k % 3 == 1:
                    rc, msg = refused_call()
                    if rc != 1 or msg != REFUSAL:
                        problems.append("%s after call %d: the refused call gave status %d, %r" % (tag, k, rc, msg))
            done.append(tag)
        except BaseException as e:                      # noqa: B902  (reported by the main thread)
            problems.append("%s: %s: %s" % (tag, type(e).__name__, e))

    threads = [threading.Thread(target=worker, args=(tag,) + plan[tag], daemon=True) for tag in plan]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    alive = [t for t in threads if t.is_alive()]
    assert not alive, "%d thread(s) have not returned" % len(alive)
    assert not problems, "\n".join(problems)
    assert sorted(done) == sorted(plan)
    assert lib.mnc_last_error().decode() == ""          # the main thread saw none of it
