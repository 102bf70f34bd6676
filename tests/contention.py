"""A kernel on its own context while other contexts keep the CUs, the caches and the memory system busy (helper module of
tests/test_gpu_contention.py and tests/test_gpu_host_threads.py; tests/test_contention_host.py checks the pure parts on the CPU).

The kernel under test runs R = 16 times on stream 0, each launch into its own NaN-filled outputs, alternating two inputs through the
same scratch, slab and ticket addresses.  Up to three disturber contexts run on streams 1..3, each with buffers allocated once:
  twin       the case under test itself on a third input (what the other images in flight are in production); its last output is
             compared with its own reference at the end;
  compute    mnc_fc at 300 x 4096 x 4096 (matrix pipe, LDS-DMA);
  bandwidth  mnc_add over three 256 MB operands (well past the L2 and the MALL).
Everything is enqueued from one host thread -- the launches are asynchronous --: a pre-roll of disturber launches, then rounds of one
launch per disturber and one of the kernel under test, then one synchronisation of every context.  No kernel waits for another.

The evidence that the contention was real: per-launch profiling (mnc_prof_enable) is on for the context under test only; the R
launches run alone first, then under the schedule; a launch is *disturbed* when it took longer than the slowest solo launch, and
at least half of the contended launches must be.  The pre-roll is sized from measured times (the disturbers' own milliseconds per
launch against the solo time of what they have to cover), never from the outcome."""
import ctypes
import math
import time

import numpy as np

R = 16                    # launches of the kernel under test per case
MIN_SHARE = 0.5           # of the contended launches must be disturbed
COVER = 3.0               # the pre-roll covers this many times the solo time of all R launches ...
MIN_PREROLL, MAX_PREROLL = 4, 4096    # ... within these launch counts per disturber
KERNEL_PREROLL = 32       # the least pre-roll before asynchronous launches: the host needs longer to enqueue a round of four launches
                          # than a small kernel runs, and the disturbers must not run dry meanwhile
KINDS = ("twin", "compute", "bandwidth")


# ---------------------------------------------------------------- the pure parts
def schedule(preroll, rounds=R):
    """The launch order as (stream, launch) pairs: stream 0 is the kernel under test, stream d + 1 the disturber whose pre-roll is
    preroll[d]; `launch` counts per stream from 0.  The pre-roll comes first (the disturbers take turns), then `rounds` rounds of one
    launch per disturber followed by one launch of the kernel under test."""
    preroll = [int(p) for p in preroll]
    if rounds < 1 or any(p < 0 for p in preroll):
        raise ValueError("schedule: rounds %r, preroll %r" % (rounds, preroll))
    seq = []
    for k in range(max(preroll + [0])):
        seq += [(d + 1, k) for d, p in enumerate(preroll) if k < p]
    for r in range(rounds):
        seq += [(d + 1, p + r) for d, p in enumerate(preroll)]
        seq.append((0, r))
    return seq


def input_of(launch):
    """Which of the two inputs launch number `launch` of the kernel under test takes: they alternate."""
    return launch & 1


def preroll_depth(cover_ms, launch_ms, least=MIN_PREROLL):
    """Launches of a disturber that take `cover_ms` when one takes `launch_ms`, within [least, MAX_PREROLL]."""
    if not launch_ms > 0.0:
        return MAX_PREROLL
    return int(min(MAX_PREROLL, max(least, math.ceil(cover_ms / launch_ms))))


def disturbed(solo_ms, contended_ms):
    """-> (share, stretch, flags): flags[i] is True when contended launch i took longer than the slowest solo launch, share their
    fraction, stretch the contended median over the solo median."""
    solo, cont = [float(t) for t in solo_ms], [float(t) for t in contended_ms]
    if not solo or not cont:
        raise ValueError("disturbed: no durations")
    bar = max(solo)
    flags = [t > bar for t in cont]
    med = float(np.median(solo))
    return sum(flags) / float(len(flags)), (float(np.median(cont)) / med if med > 0.0 else float("inf")), flags


def difference(got, want):
    """None when got equals want by value (-0.0 equals +0.0; a NaN where the reference has one too is equal), else the count, the
    NaN count and the first positions (as exact() of tests/test_gpu_exact_arithmetic.py reports them)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s, want %s" % (got.shape, want.shape)
    same = got == want
    if want.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
    if same.all():
        return None
    bad = np.argwhere(~same)
    nan = int(np.isnan(got).sum()) if got.dtype.kind == "f" else 0
    return "%d of %d values differ (NaN: %d); first at %s: got %r, want %r" % (
        len(bad), got.size, nan, bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------- one case on one context
class Running(object):
    """A case set up on one context.  launch(i, slot) enqueues the kernel on input i into output slot `slot` (asynchronous);
    read(slot) -> list of arrays; wants[i] -> the reference's list of arrays for input i; fill(slot) refills the slot with NaN."""

    def __init__(self, launch, read, fill, wants, slots):
        self.launch, self.read, self.fill, self.wants, self.slots = launch, read, fill, wants, slots


def prof_ms(dev, launches):
    """The milliseconds of each of `launches` equal calls recorded since the last mnc_prof_reset (synchronises the stream)."""
    n = ctypes.c_int(0)
    dev.call("mnc_prof_count", ctypes.addressof(n))
    assert n.value > 0 and n.value % launches == 0, "%d profile records for %d launches" % (n.value, launches)
    per, ms, out = n.value // launches, ctypes.c_float(-1.0), []
    for i in range(launches):
        t = 0.0
        for k in range(per):
            dev.call("mnc_prof_get", i * per + k, None, 0, ctypes.addressof(ms), None, None)
            t += ms.value
        out.append(t)
    return out


class Disturbers(object):
    """Up to three extra contexts on device 0, one per kind of load it is asked to hold (dev_count: the first so many of KINDS, or
    the kinds themselves); buffers are allocated once."""

    def __init__(self, dev_count=3):
        from gpu_util import Dev
        kinds = KINDS[:dev_count] if isinstance(dev_count, int) else tuple(dev_count)
        assert len(kinds) <= 3 and len(set(kinds)) == len(kinds) and all(k in KINDS for k in kinds), kinds
        self.kinds = tuple(k for k in KINDS if k in kinds)
        self.devs = [Dev(0) for _ in self.kinds]
        self.by_kind = dict(zip(self.kinds, self.devs))
        rng = np.random.default_rng(77)
        self.static = {}                               # kind -> (launch, ms per launch)
        if "compute" in self.by_kind:
            d, (M, N, K) = self.by_kind["compute"], (300, 4096, 4096)
            a, w = d.put(rng.normal(0, 1, (M, K)).astype(np.float32)), d.put((rng.normal(0, 1, (N, K)) / 64).astype(np.float32))
            b, o = d.put(np.zeros(N, np.float32)), d.empty((M * N,))
            self.static["compute"] = self._timed(d, lambda: d.call("mnc_fc", a, w, b, o, M, N, K, N, 1))
        if "bandwidth" in self.by_kind:
            d, n = self.by_kind["bandwidth"], 64 << 20
            p = [d.alloc(4 * n) for _ in range(3)]
            for q in p:
                d.call("mnc_dev_zero", q, 4 * n)
            self.static["bandwidth"] = self._timed(d, lambda: d.call("mnc_add", p[0], p[1], p[2], n, 0))

    @staticmethod
    def _timed(dev, launch, reps=4):
        launch()
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            launch()
        dev.sync()
        return launch, (time.perf_counter() - t0) * 1e3 / reps

    def loads(self, twin=None, twin_ms=None):
        """-> [(kind, launch(k), ms per launch)] of the streams 1..: the twin's launch reuses its one output slot."""
        out = []
        for kind in self.kinds:
            if kind == "twin":
                if twin is not None:
                    out.append((kind, lambda k: twin.launch(0, 0), twin_ms))
            else:
                fn, ms = self.static[kind]
                out.append((kind, (lambda f: lambda k: f())(fn), ms))
        return out

    def sync(self):
        for d in self.devs:
            d.sync()

    def close(self):
        for d in self.devs:
            d.close()
        self.devs = []


def run_schedule(loads, preroll, under_test, rounds=R):
    """Enqueue schedule(preroll, rounds): stream 0 is under_test(launch), stream d + 1 is loads[d]."""
    for stream, k in schedule(preroll, rounds):
        if stream == 0:
            under_test(k)
        else:
            loads[stream - 1][1](k)


def report(what, solo_ms, cont_ms, preroll, kinds):
    """One line per case: the share, the stretch, which launches were disturbed (X) and which not (.), the solo durations."""
    share, stretch, flags = disturbed(solo_ms, cont_ms)
    print("contention %-58s disturbed %2d/%d  stretch %5.2fx  %s  solo median %.4f max %.4f ms  pre-roll %s" % (
        what, sum(flags), len(flags), stretch, "".join("X" if f else "." for f in flags), float(np.median(solo_ms)), max(solo_ms),
        ", ".join("%s %d" % kp for kp in zip(kinds, preroll))))
    return share, stretch


def contended_kernel(dev, disturbers, build, what, tunes=()):
    """The whole check of one asynchronous case.  build(dev, seeds, slots) -> Running.  Solo: R launches alone, every result equal
    to the reference.  Contended: the same under the schedule; every result equal to the reference AND to the solo result of
    its input; the twin's last output equal to its own reference; at least MIN_SHARE of the launches disturbed.  Returns
    (share, stretch)."""
    import pytest
    twin_dev = disturbers.by_kind.get("twin")
    keys = [k for k, _ in tunes]
    both = [dev] + ([twin_dev] if twin_dev else [])
    marks = [d.mark() for d in both]
    try:
        for d in both:
            for k, v in tunes:
                d.tune(k, v)
        run = build(dev, (0, 1), R)
        twin = build(twin_dev, (2,), 1) if twin_dev else None
        dev.call("mnc_prof_enable", 1)
        run.launch(0, 0)                               # (grows the context's scratch before anything is timed)
        dev.sync()
        run.fill(0)
        dev.call("mnc_prof_reset")
        for k in range(R):
            run.launch(input_of(k), k)
        solo_ms = prof_ms(dev, R)
        solo = [None, None]
        for k in range(R):
            got = run.read(k)
            for g, w in zip(got, run.wants[input_of(k)]):
                diff = difference(g, w)
                if diff:
                    pytest.fail("%s, solo launch %d (input %d): %s" % (what, k, input_of(k), diff))
            if solo[input_of(k)] is None:
                solo[input_of(k)] = got
            run.fill(k)
        loads = disturbers.loads(twin, float(np.median(solo_ms)))
        preroll = [preroll_depth(COVER * R * max(solo_ms), ms, KERNEL_PREROLL) for _, _, ms in loads]
        dev.sync()
        dev.call("mnc_prof_reset")
        run_schedule(loads, preroll, lambda k: run.launch(input_of(k), k))
        cont_ms = prof_ms(dev, R)
        disturbers.sync()
        for k in range(R):
            for g, w, s in zip(run.read(k), run.wants[input_of(k)], solo[input_of(k)]):
                diff = difference(g, w) or difference(g, s)
                if diff:
                    pytest.fail("%s, contended launch %d of %d (input %d): %s" % (what, k, R, input_of(k), diff))
        if twin is not None:
            for g, w in zip(twin.read(0), twin.wants[0]):
                diff = difference(g, w)
                if diff:
                    pytest.fail("%s, the twin's last output: %s" % (what, diff))
        share, stretch = report(what, solo_ms, cont_ms, preroll, [k for k, _, _ in loads])
        assert share >= MIN_SHARE, "%s: only %d of %d contended launches took longer than the slowest solo launch (%.3f ms)" % (
            what, int(round(share * R)), R, max(solo_ms))
        return share, stretch
    finally:
        dev.call("mnc_prof_enable", 0)
        dev.call("mnc_prof_reset")
        disturbers.sync()
        for d, m in zip(both, marks):
            for k in keys:
                d.tune(k, None)
            d.free_since(m)


def contended_call(disturbers, call, timed_ms, what, check, calls=R):
    """The same for a synchronous host-array entry point.  call(k) makes call k (inputs alternate by input_of) and returns its
    result; timed_ms() -> the milliseconds of the call just made (the task's own timing span, or None: the wall time of the call
    is used); check(k, result) fails the test on a difference.  Each contended call is preceded by a pre-roll that covers COVER
    times the slowest solo call."""
    def one(k):
        t0 = time.perf_counter()
        res = call(k)
        wall = (time.perf_counter() - t0) * 1e3
        ms = timed_ms()
        return res, (wall if ms is None else ms)

    call(0), call(1)                                   # (grow the shared workspace before anything is timed)
    solo_ms = []
    for k in range(calls):
        res, ms = one(k)
        check(k, res)
        solo_ms.append(ms)
    loads = disturbers.loads()
    preroll = [preroll_depth(COVER * max(solo_ms), ms) for _, _, ms in loads]
    cont_ms = []
    for k in range(calls):
        run_schedule(loads, preroll, lambda r: None, rounds=1)
        res, ms = one(k)
        disturbers.sync()
        check(k, res)
        cont_ms.append(ms)
    share, stretch = report(what, solo_ms, cont_ms, preroll, [k for k, _, _ in loads])
    assert share >= MIN_SHARE, "%s: only %d of %d contended calls took longer than the slowest solo call (%.3f ms)" % (
        what, int(round(share * calls)), calls, max(solo_ms))
    return share, stretch
