"""The check every host-array entry of the mask files makes of a set of packed masks (csrc/mask_set.h: HostMaskSet::check), at each
of the host sets that go through it: mnc_mask_overlaps a and b, mnc_mask_nms, mnc_mask_rle, mnc_mask_boundary, dt and gt of
mnc_mask_match and mnc_mask_match_boundary, and the sets of the tight-result entries (csrc/mask_tight.h): mnc_mask_combine a and b,
mnc_mask_merge, mnc_mask_layer, mnc_mask_isometry and mnc_mask_warp.  A set with a coordinate of 2^24, with an offset of 4, or with rows that reach past the
bytes given comes back as MNC_ERR_INVALID with the message that names the entry point, the set and the index, no output array
written -- without a GPU: nothing of this may open a device.  The same for one refused parameter of each matching entry."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mnc_amd import _lib  # noqa: E402

INVALID = 1
FILL = 0x5a                     # every output byte before the call

# what is wrong with instance 1 of a set of two 10 x 10 masks (80 bytes each) -> the message behind "<entry>: "
FLAWS = {
    "coordinate": "%s[1] coordinate 16777216 out of range",
    "offset": "%s[1] offset 4 is negative or not a multiple of 8",
    "rows": "the rows of %s[1] (80 bytes at 80) reach past the 152 bytes given",
}


class Set:
    """Two 10 x 10 masks of ones with classes and scores, good or with one flaw; the arrays live as long as the object."""

    def __init__(self, flaw=None):
        self.bounds = np.array([[0, 0, 9, 9], [0, 0, 9, 9]], np.int32)
        self.offsets = np.array([0, 80], np.int64)
        self.areas = np.array([100, 100], np.int64)
        self.bits = np.full(20, (1 << 10) - 1, np.uint64)
        self.nbytes = self.bits.nbytes
        self.classes = np.array([1, 1], np.int32)
        self.scores = np.array([0.9, 0.8], np.float32)
        if flaw == "coordinate":
            self.bounds[1] = (0, 0, 2 ** 24, 0)
        elif flaw == "offset":
            self.offsets[1] = 4
        elif flaw == "rows":
            self.nbytes = 152
        else:
            assert flaw is None

    def args(self, areas=True):
        p = _lib.ptr
        return (p(self.bounds), p(self.offsets)) + ((p(self.areas),) if areas else ()) + (p(self.bits), self.nbytes, 2)


def out(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def overlaps(a, b):
    outs = [out((2, 2), np.int64), out((2, 2), np.float64)]
    return "mnc_mask_overlaps", a.args() + b.args() + (_lib.ptr(outs[0]), _lib.ptr(outs[1]), 0), outs


def nms(s):
    outs = [out(2, np.int32), out(1, np.int32)]
    return "mnc_mask_nms", s.args()[:5] + (2, _lib.ptr(s.classes), _lib.ptr(s.scores), 0.5, 0, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                           0), outs


def rle(s):
    outs = [out(3, np.int64), out(64, np.uint32), out(1, np.uint64)]
    return "mnc_mask_rle", s.args(areas=False) + (20, 30, _lib.ptr(outs[0]), _lib.ptr(outs[1]), 64, _lib.ptr(outs[2]), 0), outs


def boundary(s):
    outs = [out((2, 4), np.int32), out(2, np.int64), out(2, np.int64), out(20, np.uint64), out(1, np.uint64)]
    return "mnc_mask_boundary", s.args(areas=False) + (20, 30, 2, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]),
                                                       _lib.ptr(outs[3]), outs[3].nbytes, _lib.ptr(outs[4]), 0), outs


KEEP = {"crowd": np.zeros(2, np.uint8), "thrs": np.array([0.5, 0.75]), "rngs": np.array([[0.0, 1e10]])}


def _match(name, dt, gt, T, image):
    A, D, G = 1, 2, 2
    outs = [out(D, np.int32), out((A, 2, D), np.int32), out((A, 2, D), np.uint8), out((A, 2, G), np.int32), out((A, G), np.uint8),
            out((D, G), np.float64)] + ([out((D, G), np.float64)] if image else [])
    p = _lib.ptr
    args = (dt.args() + (p(dt.classes), p(dt.scores)) + gt.args() + (p(gt.classes), p(KEEP["crowd"]), None, None, p(KEEP["thrs"]), T,
                                                                    p(KEEP["rngs"]), A, 100) + image +
            tuple(p(o) for o in outs) + (0,))
    return name, args, outs


def match(dt, gt, T=2):
    return _match("mnc_mask_match", dt, gt, T, ())


def match_boundary(dt, gt, T=2, d=2):
    return _match("mnc_mask_match_boundary", dt, gt, T, (20, 30, d))


def _tight(name, sets, middle):
    """An entry of csrc/mask_tight.h's protocol: its sets, its own arguments, then bounds, offsets, areas, bits with their room, the
    bound, the bytes and the device."""
    outs = [out((2, 4), np.int32), out(2, np.int64), out(2, np.int64), out(20, np.uint64), out(1, np.uint64), out(1, np.uint64)]
    p = _lib.ptr
    return name, sets + tuple(p(m) for m in middle) + tuple(p(o) for o in outs[:4]) + (outs[3].nbytes, p(outs[4]), p(outs[5]), 0), outs


TIGHT = {"group_ptr": np.array([0, 2], np.int64), "members": np.array([0, 1], np.int32), "coef": np.array([1, 0, 0, 0, 1, 0], np.int64),
         "window": np.array([0, 0, 19, 29], np.int32)}


def combine(a, b):
    return _tight("mnc_mask_combine", a.args(areas=False) + b.args(areas=False), (1, None))          # a | b, no window


def merge(s):
    return _tight("mnc_mask_merge", s.args(areas=False), (TIGHT["group_ptr"], TIGHT["members"], 1, 0))


def layer(s):
    return _tight("mnc_mask_layer", s.args(areas=False), (s.scores, None))


def isometry(s):
    return _tight("mnc_mask_isometry", s.args(areas=False), (2, 19, 0))                              # fliplr of a 20-wide image


def warp(s):
    return _tight("mnc_mask_warp", s.args(areas=False), (TIGHT["coef"], 1, TIGHT["window"]))


# the good set beside a flawed one: the calls hold addresses alone, so it must outlive them (a Set() made in the lambda would be
# freed before the call reads it)
GOOD = Set()

# set name in the messages -> the call with that set flawed and every other one good
SETS = {
    "combine a": ("a", lambda bad: combine(bad, GOOD)),
    "combine b": ("b", lambda bad: combine(GOOD, bad)),
    "merge": ("masks", merge),
    "layer": ("masks", layer),
    "isometry": ("masks", isometry),
    "warp": ("masks", warp),
    "overlaps a": ("a", lambda bad: overlaps(bad, GOOD)),
    "overlaps b": ("b", lambda bad: overlaps(GOOD, bad)),
    "nms": ("masks", nms),
    "rle": ("masks", rle),
    "boundary": ("masks", boundary),
    "match dt": ("dt", lambda bad: match(bad, GOOD)),
    "match gt": ("gt", lambda bad: match(GOOD, bad)),
    "match_boundary dt": ("dt", lambda bad: match_boundary(bad, GOOD)),
    "match_boundary gt": ("gt", lambda bad: match_boundary(GOOD, bad)),
}


def refused(call, message):
    name, args, outs = call
    with pytest.raises(_lib.MncError) as e:
        _lib.call(name, *args)
    assert e.value.code == INVALID
    assert str(e.value) == "%s failed (status %d): %s: %s" % (name, INVALID, name, message)
    for o in outs:
        assert (o.view(np.uint8) == FILL).all()


@pytest.mark.parametrize("flaw", list(FLAWS))
@pytest.mark.parametrize("which", list(SETS))
def test_a_flawed_set_is_refused_by_name_before_a_device_is_opened(which, flaw):
    set_name, make = SETS[which]
    bad = Set(flaw)
    refused(make(bad), FLAWS[flaw] % set_name)


def test_a_refused_parameter_of_the_matching_entries_writes_nothing():
    dt, gt = Set(), Set()
    refused(match(dt, gt, T=0), "T=0 not in [1, 16]")
    refused(match_boundary(dt, gt, T=0), "T=0 not in [1, 16]")
    refused(match_boundary(dt, gt, d=0), "d=0 not in [1, 1024]")

