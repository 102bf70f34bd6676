"""GPU: mnc_proposal, mnc_proposal_candidates, mnc_proposal_count, mnc_stage_bridge and mnc_detect_tail on the corpora of
tests/proposal_edge_inputs.py, against the plain statements there.  Every comparison is exact, and every output buffer is
pre-filled with NaN, so a row the library leaves unwritten shows.  Every mnc_proposal case runs with the library's own choice of
top-K and with TOPK_SINGLE_WG=1: each equals the statement (rois, and the candidates with their scores in order) and the two agree
byte for byte.

Values are compared with np.array_equal, which equates -0.0 and +0.0: the sign of a zero COORDINATE is part of no entry's contract
(numpy's maximum(-0.0, 0) and the device's fmaxf may differ there).  The ORDER of zero scores is part of the contract -- the two
zeros tie and the anchor index decides -- and is asserted through the candidates' boxes.  NaN inputs are outside every contract and
appear nowhere.  The corpus properties and the variations each case tells apart are checked without a GPU in
tests/test_proposal_edges_host.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mnc_amd  # noqa: E402
import proposal_edge_inputs as PE  # noqa: E402
from gpu_util import Dev  # noqa: E402
from mnc_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
mnc_amd.install_paths()
F32 = np.float32
RUNS = {"default": 0, "single": 0}                            # mnc_proposal cases run with each top-K setting


@pytest.fixture(scope="module")
def dev():
    d = Dev(0)
    yield d
    d.close()


@pytest.fixture
def tune(dev):
    """tune(name, value): override one of the launchers' choices on the module's context for this test."""
    keys = []

    def set_(name, value):
        keys.append(name)
        dev.tune(name, value)
    yield set_
    for k in keys:
        dev.tune(k, None)


@pytest.fixture(scope="module")
def exp():
    fn, name = PE.exp_reference()
    if fn is None:
        pytest.skip(name)
    print("exp reference: %s" % name)
    return fn


def exact(got, want, what):
    """np.array_equal, with the first differing row and both of its values in the message."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        pytest.fail("%s: shape %r, want %r" % (what, got.shape, want.shape))
    if not np.array_equal(got, want):
        bad = np.argwhere(~(got == want))
        r = int(bad[0][0])
        pytest.fail("%s: %d of %d values differ (NaN: %d); first at row %d: got %r, want %r" % (
            what, len(bad), got.size, int(np.isnan(got).sum()), r, got[r].tolist(), want[r].tolist()))


def proposal(dev, c, single, read_count=True):
    """One mnc_proposal call -> (count, all post_nms_topn rows of d_rois, candidate boxes, candidate scores)."""
    mark = dev.mark()
    try:
        d_prob, d_bbox = dev.put(c["prob"]), dev.put(c["deltas"])
        post = c["post_nms_topn"]
        d_rois = dev.empty((post, 5), fill=np.nan)
        dev.tune("TOPK_SINGLE_WG", "1" if single else None)
        num = ctypes.c_int(-1)
        info = c["im_info"]
        dev.call("mnc_proposal", d_prob, d_bbox, c["A"], c["H"], c["W"], _lib.ptr(c["anchors"]), c["feat_stride"], float(info[0]),
                 float(info[1]), float(info[2]), c["pre_nms_topn"], post, c["nms_thresh"], c["min_size"], d_rois,
                 ctypes.addressof(num) if read_count else None)
        if not read_count:
            dev.call("mnc_proposal_count", ctypes.addressof(num))
        rois = dev.get(d_rois, (post, 5))
        n = ctypes.c_int(-1)
        dev.call("mnc_proposal_candidates", None, None, 0, ctypes.addressof(n))
        cb, cs = np.full((n.value, 4), np.nan, F32), np.full(n.value, np.nan, F32)
        if n.value:
            dev.call("mnc_proposal_candidates", _lib.ptr(cb), _lib.ptr(cs), n.value, ctypes.addressof(n))
        RUNS["single" if single else "default"] += 1
        return num.value, rois, cb, cs
    finally:
        dev.tune("TOPK_SINGLE_WG", None)
        dev.free_since(mark)


def against_statement(c, path, got, want):
    count, rois, cb, cs = got
    what = "%s [%s top-K]" % (c["name"], path)
    assert count == len(want["rois"]), "%s: %d rois, want %d" % (what, count, len(want["rois"]))
    exact(cb, want["boxes"], what + " candidate boxes")
    exact(cs, want["scores"], what + " candidate scores")
    exact(rois[:count], want["rois"], what + " rois")
    exact(rois[count:], np.zeros((len(rois) - count, 5), F32), what + " rows past the count")


def check(dev, c, exp):
    """Both top-K settings against the statement and against each other."""
    want = PE.proposal_statement(c, exp)
    if "expect_valid" in c:
        assert want["valid"] == c["expect_valid"]
    res = {}
    for path, single in (("default", False), ("single", True)):
        res[path] = proposal(dev, c, single)
        against_statement(c, path, res[path], want)
    a, b = res["default"], res["single"]
    assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])), c["name"] + ": the two top-K paths differ"
    return want, res["default"]


# ---- 1. anchor counts, with the tied score sets at three of them ------------------------------------------------------------
@pytest.mark.parametrize("N", [n for n, _ in PE.ANCHOR_COUNTS])
def test_anchor_counts_around_the_topk_constants(dev, exp, N):
    cases = [c for c in PE.count_cases() if c["N"] == N] if N in (2049, 24577, 65537) else [PE.count_case(N)]
    assert len(cases) == {2049: 10, 24577: 12, 65537: 10}.get(N, 1)
    for c in cases:
        want, _ = check(dev, c, exp)
        assert want["valid"] > 0 or N == 1
    print("mnc_proposal cases so far: %r" % RUNS)


def test_pre_nms_topn_above_the_sort_capacity_is_refused(dev):
    for c in PE.refused_cases():
        with pytest.raises(_lib.MncError) as e:
            proposal(dev, c, False)
        assert e.value.code == 1, c["name"]                   # MNC_ERR_INVALID


# ---- 2. / 3. K = min(pre_nms_topn, valid), crossed with the score sets -----------------------------------------------------------
@pytest.mark.parametrize("kind", PE.SCORE_KINDS)
def test_k_edges_with_each_score_set(dev, exp, kind):
    cases = [c for c in PE.k_cases() if c["name"].endswith(kind)]
    assert len(cases) == len(PE.K_TOPNS) + len(PE.K_V_SWEEPS)
    for c in cases:
        want, got = check(dev, c, exp)
        assert got[2].shape[0] == c["expect_K"]
    print("mnc_proposal cases so far: %r" % RUNS)


# ---- 4. the decode's rules ----------------------------------------------------------------------------------------------------
def test_decode_on_its_thresholds_bounds_and_exp_cutoffs(dev, exp):
    for c in PE.decode_cases():
        want, _ = check(dev, c, exp)
        if "thr" in c:
            assert list(want["valid_index"]) == [1, 2, 4, 5, 6]


# ---- 5. the scan's gather paths, rows past the count, nothing left ------------------------------------------------------------
def test_scan_gathers_through_both_paths_and_zeroes_the_rest(dev, exp):
    rows = {}
    for post in PE.SCAN_POSTS:
        want, got = check(dev, PE.scan_case(post), exp)
        assert got[0] == min(post, 5000)
        rows[post] = got[1]
    exact(rows[4097][:4096], rows[4096], "4097 rows (gather through keep) against 4096 rows (gather through the LDS list)")
    exact(rows[6000][:4097], rows[4097], "6000 against 4097 rows")
    assert not rows[6000][5000:].any()
    want, got = check(dev, PE.scan_case(300, 17.0), exp)
    assert got[0] == 0 and got[2].shape == (0, 4) and not got[1].any()


def test_state_left_by_a_larger_map(exp):
    """65537 anchors, then 135, then 2049 on one context: each equals what a fresh context gives, and the statement."""
    cases = [PE.count_case(n) for n in PE.SEQUENCE]
    used = Dev(0)
    try:
        for c in cases:
            got = proposal(used, c, False)
            fresh = Dev(0)
            try:
                alone = proposal(fresh, c, False)
            finally:
                fresh.close()
            against_statement(c, "default, after a larger map", got, PE.proposal_statement(c, exp))
            assert got[0] == alone[0] and all(x.tobytes() == y.tobytes() for x, y in zip(got[1:], alone[1:])), c["name"]
    finally:
        used.close()


def test_asynchronous_count(dev, exp):
    c = PE.count_case(2049)
    sync = proposal(dev, c, False)
    later = proposal(dev, c, False, read_count=False)
    against_statement(c, "default, count read afterwards", later, PE.proposal_statement(c, exp))
    assert sync[0] == later[0] and all(x.tobytes() == y.tobytes() for x, y in zip(sync[1:], later[1:]))


# ---- stage bridge ----------------------------------------------------------------------------------------------------
def bridge(dev, c):
    R, K = c["R"], c["K"]
    mark = dev.mark()
    try:
        d_out = dev.empty((R + 1, 5), fill=np.nan)
        if R:
            dev.call("mnc_stage_bridge", dev.put(c["rois"]), dev.put(c["bbox"]), c["ld_bbox"], dev.put(c["probs"]), c["ld_probs"], R, K,
                     float(c["im_h"]), float(c["im_w"]), d_out)
        else:
            dev.call("mnc_stage_bridge", None, None, c["ld_bbox"], None, c["ld_probs"], 0, K, float(c["im_h"]), float(c["im_w"]), d_out)
        dev.sync()
        out = dev.get(d_out, (R + 1, 5))
        assert np.isnan(out[R]).all(), c["name"] + ": a row past R was written"
        return out[:R]
    finally:
        dev.free_since(mark)


def test_stage_bridge_ties_strides_and_decode_edges(dev, exp):
    for c in PE.bridge_cases():
        exact(bridge(dev, c), PE.bridge_statement_of(c, exp), "mnc_stage_bridge " + c["name"])


# ---- detect tail ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in PE.TAIL_SCALES])
def test_detect_tail_divides_in_float32(dev, name):
    scale = dict(PE.TAIL_SCALES)[name]
    for R1, R2 in PE.TAIL_COUNTS:
        r1, r2 = PE.tail_case(name, R1, R2)
        mark = dev.mark()
        d_out = dev.empty((R1 + R2 + 1, 4), fill=np.nan)
        dev.call("mnc_detect_tail", dev.put(r1) if R1 else None, R1, dev.put(r2) if R2 else None, R2, float(scale), PE.TAIL_H, PE.TAIL_W,
                 d_out)
        dev.sync()
        out = dev.get(d_out, (R1 + R2 + 1, 4))
        dev.free_since(mark)
        assert np.isnan(out[R1 + R2]).all(), "a row past R1 + R2 was written"       # (0, 0): nothing at all is written
        exact(out[:R1 + R2], PE.detect_tail_statement(r1, r2, scale, PE.TAIL_H, PE.TAIL_W),
              "mnc_detect_tail scale %s R1=%d R2=%d" % (name, R1, R2))


# ---- np_exp_f32 on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", (0, 1))
def test_device_exp_over_the_bit_patterns(dev, exp, which):
    """The device body of np_exp.h through mnc_stage_bridge with K = 1: roi (0, 0, 1, 1) makes x2 == y2 == exp(x), roi (0, 0, 0, 0)
    makes them 0.5 * exp(x), on an image as large as float32 goes.  Whole rows against the statement, so any exp bit shows."""
    roi = PE.SWEEP_ROIS[which]
    x = PE.exp_sweep_patterns().view(F32)
    total = 0
    for lo in range(0, len(x), PE.SWEEP_CHUNK):
        v = x[lo:lo + PE.SWEEP_CHUNK]
        rois, d, p = PE.sweep_rows(v, roi)
        c = {"name": "exp sweep", "rois": rois, "bbox": d, "probs": p, "ld_bbox": 4, "ld_probs": 1, "R": len(v), "K": 1,
             "im_h": PE.FLT_MAX, "im_w": PE.FLT_MAX}
        got, want = bridge(dev, c), PE.bridge_statement_of(c, exp)
        if not np.array_equal(got, want):
            bad = np.flatnonzero((got != want).any(axis=1))
            r = int(bad[0])
            pytest.fail("device exp, roi %r: %d of %d rows differ; first at x = %r (bits 0x%08x): got %r, want %r" % (
                roi, len(bad), len(v), float(v[r]), int(v[r:r + 1].view(np.uint32)[0]), got[r].tolist(), want[r].tolist()))
        total += len(v)
    assert total == len(x) > 4_000_000
    print("device exp: %d bit patterns, roi %r, reference %s" % (total, roi, PE.exp_reference()[1]))
