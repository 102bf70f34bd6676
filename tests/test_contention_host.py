"""The pure parts of tests/contention.py on the CPU: the launch schedule and the disturbed-share arithmetic."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import contention as C  # noqa: E402


@pytest.mark.parametrize("preroll,rounds", [([4, 4, 4], C.R), ([48, 7, 19], C.R), ([5], 3), ([], 2), ([0, 3], 1), ([2, 2, 2], 1)])
def test_schedule_keeps_every_stream_in_order_and_the_preroll_first(preroll, rounds):
    seq = C.schedule(preroll, rounds)
    streams = len(preroll) + 1
    # every stream's launches are 0, 1, 2, ... in that order, and complete
    for s in range(streams):
        mine = [k for st, k in seq if st == s]
        assert mine == list(range(rounds if s == 0 else preroll[s - 1] + rounds)), s
    assert all(0 <= st < streams for st, _ in seq)
    # the pre-roll comes first: nothing of the kernel under test, and no disturber launch of a round, before the last pre-roll launch
    first_under_test = seq.index((0, 0))
    head = seq[:sum(preroll)]
    assert sorted(head) == sorted((d + 1, k) for d, p in enumerate(preroll) for k in range(p))
    assert first_under_test == sum(preroll) + len(preroll)
    # then rounds: one launch per disturber, in stream order, followed by one launch of the kernel under test
    tail = seq[sum(preroll):]
    assert len(tail) == rounds * streams
    for r in range(rounds):
        assert tail[r * streams:(r + 1) * streams] == [(d + 1, p + r) for d, p in enumerate(preroll)] + [(0, r)]


def test_schedule_interleaves_the_preroll_of_unequal_depths():
    assert C.schedule([3, 1], 1) == [(1, 0), (2, 0), (1, 1), (1, 2), (1, 3), (2, 1), (0, 0)]
    with pytest.raises(ValueError):
        C.schedule([1], 0)
    with pytest.raises(ValueError):
        C.schedule([-1], 1)


def test_inputs_alternate():
    assert [C.input_of(k) for k in range(C.R)] == [0, 1] * (C.R // 2)
    assert C.R == 16 and C.MIN_SHARE == 0.5
    under_test = [k for st, k in C.schedule([2, 2, 2]) if st == 0]
    assert [C.input_of(k) for k in under_test][:4] == [0, 1, 0, 1]


def test_preroll_depth_covers_the_time_within_its_limits():
    assert C.preroll_depth(10.0, 1.0) == 10 and C.preroll_depth(10.0, 3.0) == 4 and C.preroll_depth(10.1, 1.0) == 11
    assert C.preroll_depth(0.001, 1.0) == C.MIN_PREROLL and C.preroll_depth(1e9, 1.0) == C.MAX_PREROLL
    assert C.preroll_depth(1.0, 0.0) == C.MAX_PREROLL
    assert C.preroll_depth(10.0, 1.0, C.KERNEL_PREROLL) == C.KERNEL_PREROLL and C.preroll_depth(100.0, 1.0, C.KERNEL_PREROLL) == 100
    assert C.MIN_PREROLL <= C.KERNEL_PREROLL < C.MAX_PREROLL


def test_disturbed_share_from_durations():
    solo = [1.0, 1.2, 0.9, 1.1]
    share, stretch, flags = C.disturbed(solo, [1.2, 1.21, 3.0, 0.5])
    assert flags == [False, True, True, False] and share == 0.5             # equal to the slowest solo launch is not disturbed
    assert stretch == pytest.approx(np.median([1.2, 1.21, 3.0, 0.5]) / 1.05)
    assert C.disturbed(solo, [5.0] * 16)[0] == 1.0 and C.disturbed(solo, [1.0] * 16)[0] == 0.0
    assert C.disturbed(solo, [2.0] * 7 + [1.0] * 9)[0] == 7 / 16.0 < C.MIN_SHARE


def test_disturbed_share_edge_cases():
    # all solo durations equal: the bar is that duration; only strictly longer launches count
    share, stretch, flags = C.disturbed([2.0] * 16, [2.0, 2.0001, 1.0, 4.0])
    assert flags == [False, True, False, True] and share == 0.5 and stretch == pytest.approx(2.00005 / 2.0)
    # one launch
    assert C.disturbed([1.0], [1.5]) == (1.0, 1.5, [True])
    assert C.disturbed([1.0], [1.0]) == (0.0, 1.0, [False])
    # zero solo durations (an event pair below the clock's resolution): no division by zero
    assert C.disturbed([0.0, 0.0], [0.0, 0.1])[:2] == (0.5, float("inf"))
    for solo, cont in (([], [1.0]), ([1.0], [])):
        with pytest.raises(ValueError):
            C.disturbed(solo, cont)


def test_difference_reports_count_and_position():
    want = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert C.difference(want.copy(), want) is None
    got = want.copy()
    got[1, 2] = np.nan
    got[2, 3] = -1.0
    msg = C.difference(got, want)
    assert msg.startswith("2 of 12 values differ (NaN: 1); first at [[1, 2], [2, 3]]")
    nan = np.array([np.nan, 1.0], np.float32)
    assert C.difference(nan.copy(), nan) is None                           # a NaN the reference has too is no difference
    assert C.difference(np.zeros(3, np.int32), np.zeros(4, np.int32)) == "shape (3,), want (4,)"
    assert C.difference(np.array([0.0], np.float32), np.array([-0.0], np.float32)) is None
