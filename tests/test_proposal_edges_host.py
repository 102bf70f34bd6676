"""The corpora of tests/proposal_edge_inputs.py without a GPU: every case carries the property it is named for, the plain
statements agree with the oracle where the oracle's fixed constants (A = 9, 6000, 300, 0.7, min_size 16) apply, and every variation
of a rule that the statements take as a `mutant` is told apart by at least one case of the matching corpus."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import golden_inputs as GI  # noqa: E402
import mnc_amd  # noqa: E402
import proposal_edge_inputs as PE  # noqa: E402
from oracle import host as ohost  # noqa: E402

mnc_amd.install_paths()
F32 = np.float32


@pytest.fixture(scope="module")
def exp():
    fn, name = PE.exp_reference()
    if fn is None:
        pytest.skip(name)
    return fn


def same(a, b):
    """Two results of proposal_statement: candidates in order and rois."""
    return all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in ("boxes", "scores", "rois"))


def reported(cases, exp, mutant, plain=None):
    """Names of the cases on which the mutated statement differs from the plain one."""
    out = []
    for i, c in enumerate(cases):
        want = plain[i] if plain is not None else PE.proposal_statement(c, exp)
        if not same(PE.proposal_statement(c, exp, (mutant,)), want):
            out.append(c["name"])
    return out


# ---- agreement with the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fh,fw,seed", [(38, 63, 3), (12, 20, 2)])
def test_proposal_statement_equals_oracle_on_golden_cases(fh, fw, seed):
    pc = GI.proposal_case(fh, fw, seed)
    c = {"name": "golden", "prob": pc["cls_prob"], "deltas": pc["bbox_pred"], "A": 9, "H": fh, "W": fw, "N": 9 * fh * fw,
         "anchors": np.ascontiguousarray(ohost.generate_anchors(), F32), "feat_stride": 16, "im_info": pc["im_info"][0],
         "pre_nms_topn": ohost.RPN_PRE_NMS_TOP_N, "post_nms_topn": ohost.RPN_POST_NMS_TOP_N, "nms_thresh": ohost.RPN_NMS_THRESH,
         "min_size": float(ohost.RPN_MIN_SIZE)}
    got = PE.proposal_statement(c, np.exp)                    # the oracle calls np.exp whatever numpy makes of it
    ob, osc = ohost.proposal_candidates(pc["cls_prob"], pc["bbox_pred"], pc["im_info"])
    assert got["boxes"].dtype == F32 and np.array_equal(got["boxes"], ob) and np.array_equal(got["scores"], osc.ravel())
    want = ohost.proposal_forward(pc["cls_prob"], pc["bbox_pred"], pc["im_info"])
    assert got["rois"].dtype == F32 and got["rois"].shape == want.shape and np.array_equal(got["rois"], want)


def test_bridge_and_tail_statements_equal_oracle():
    for seed in (4, 5):
        sc = GI.stage_bridge_case(seed)
        got = PE.stage_bridge_statement(sc["rois"], sc["bbox_pred"], sc["scores"], sc["im_info"][0, 0], sc["im_info"][0, 1], np.exp)
        want = ohost.stage_bridge_forward_test(sc["rois"], sc["bbox_pred"], sc["scores"], sc["im_info"])
        assert got.dtype == F32 and np.array_equal(got, want)
    b = GI.detect_case(6)["blobs"]
    for scale in (1.0, 1.6, 0.8):
        want, _, _ = ohost.im_detect_tail(b["rois"], b["mask_proposal"], b["seg_cls_prob"], b["rois_ext"], b["mask_proposal_ext"],
                                          b["seg_cls_prob_ext"], scale, (600, 1000, 3))
        assert np.array_equal(PE.detect_tail_statement(b["rois"], b["rois_ext"], scale, 600, 1000), want)


# ---- 1. anchor counts ----------------------------------------------------------------------------------------------------------
def test_anchor_counts_bracket_the_constants(exp):
    ns = [n for n, _ in PE.ANCHOR_COUNTS]
    assert ns == [1, 63, 64, 65, 135, 2047, 2048, 2049, 4096, 24575, 24576, 24577, 65535, 65536, 65537]
    for k in (PE.K_RUN, PE.K_REG_KEYS, PE.K_RUN * PE.K_MAX_RUNS):
        assert {k - 1, k, k + 1} <= set(ns)
    assert [n for n in ns if not PE.has_wide_path(n)] == [65537]
    assert all(why for _, why in PE.ANCHOR_COUNTS)
    for n in (1, 135, 2049, 65537):
        c = PE.count_case(n)
        r = PE.proposal_statement(c, exp)
        assert c["N"] == n and r["valid"] == c["expect_valid"] and len(r["scores"]) == min(6000, r["valid"])
        assert float(np.abs(r["boxes"]).max(initial=0)) < 2 ** 19
        assert n < 64 or 0 < len(r["rois"]) < len(r["scores"])          # the NMS removes something
    big = PE.proposal_statement(PE.count_case(24577, "equal", PE.K_SORT_CAP), exp)
    assert len(big["scores"]) == PE.K_SORT_CAP and big["cut"]
    assert all(c["pre_nms_topn"] <= 0 or c["pre_nms_topn"] > PE.K_SORT_CAP for c in PE.refused_cases())
    assert all(min(c["N"], c["pre_nms_topn"] if c["pre_nms_topn"] > 0 else c["N"]) > PE.K_SORT_CAP for c in PE.refused_cases())


# ---- 2. / 3. K and the score sets ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k_runs(exp):
    cases = PE.k_cases()
    return cases, [PE.proposal_statement(c, exp) for c in cases]


def test_k_cases_have_their_valid_count_and_cut(k_runs):
    cases, runs = k_runs
    assert len(cases) == len(PE.SCORE_KINDS) * (len(PE.K_TOPNS) + len(PE.K_V_SWEEPS))
    assert set(PE.K_TOPNS) >= {-1, 0, 1, 2, 63, 64, 65, 1023, 1024, 1025, PE.K_V - 1, PE.K_V, PE.K_V + 1, PE.K_MAP_N, PE.K_MAP_N + 1}
    seen = set()
    for c, r in zip(cases, runs):
        V, K = c["expect_valid"], c["expect_K"]
        assert r["valid"] == V and np.array_equal(r["valid_index"], PE.k_valid(V)) and len(r["scores"]) == K, c["name"]
        assert r["cut"] == (0 < c["pre_nms_topn"] < V)
        assert len(r["rois"]) == min(K, 300)                               # disjoint boxes: the NMS keeps every one
        if K:                                                              # zero deltas: a 16 x 16 box, on the threshold
            assert np.array_equal(r["boxes"][:, 2] - r["boxes"][:, 0] + 1, np.full(K, 16, F32))
        seen.add((c["pre_nms_topn"] - V if c["pre_nms_topn"] > 0 else None, min(V, 2)))
    assert {(-1, 2), (0, 2), (1, 2), (None, 2)} <= seen and {0, 1} <= {v for _, v in seen}


def test_score_sets_are_what_they_are_named(k_runs, exp):
    cases, runs = k_runs
    inside = zero_pairs = 0
    for c, r in zip(cases, runs):
        kind = c["name"].split()[-1]
        s, K = r["scores"], c["expect_K"]
        assert np.all(np.diff(-s.astype(np.float64)[np.isfinite(s)]) >= 0)  # descending by value
        if kind == "equal":
            assert (s == 0.5).all() and np.array_equal(r["boxes"][:, 0], 16 * np.arange(K))    # index ascending
        if kind == "distinct":
            assert len(set(s.tolist())) == K
        if kind == "three" and r["cut"] and K >= 1:
            more = PE.proposal_statement(c, exp, ("cut_plus",))["scores"]
            assert s[K - 1] == 0.5 and more[K] == 0.5, c["name"]           # the cut lies inside the middle class
            inside += 1
        if kind == "special":
            z = np.flatnonzero(s == 0)
            if len(z) > 1:
                sign = np.signbit(s[z])
                assert np.all(np.diff(r["boxes"][z, 0]) > 0)                 # the zeros tie: index order whatever the sign
                zero_pairs += int((sign[:-1] & ~sign[1:]).any())            # a -0.0 in front of a +0.0
    assert inside >= 10 and zero_pairs >= 10
    sp = PE.score_set("special", 4200, None, 0, 1)
    assert (sp < 0).any() and np.isposinf(sp).any() and np.isneginf(sp).any() and not np.isnan(sp).any()
    assert ((sp != 0) & (np.abs(sp) < np.finfo(F32).tiny)).any()
    z = np.flatnonzero(sp == 0)
    assert np.array_equal(np.signbit(sp[z]), np.arange(len(z)) % 2 == 1)      # interleaved by index


@pytest.mark.parametrize("mutant,kinds", [("ties_by_index_descending", ("equal", "three", "special")), ("zeros_by_sign", ("special",)),
                                          ("cut_plus", PE.SCORE_KINDS), ("cut_minus", PE.SCORE_KINDS), ("size_gt", ("distinct",))])
def test_order_and_cut_mutants_are_reported(k_runs, exp, mutant, kinds):
    cases, runs = k_runs
    for kind in kinds:
        pick = [i for i, c in enumerate(cases) if c["name"].endswith(kind)]
        bad = reported([cases[i] for i in pick], exp, mutant, [runs[i] for i in pick])
        assert bad, (mutant, kind)
        if mutant == "zeros_by_sign":
            assert len(bad) >= 10
        if mutant == "cut_plus":                                           # exactly the cases in which something is cut off
            assert set(bad) == {cases[i]["name"] for i in pick if runs[i]["cut"]}
    plain = [c for c in cases if c["name"].endswith("distinct")]
    assert not reported(plain, exp, "zeros_by_sign") and not reported(plain[:6], exp, "ties_by_index_descending")


# ---- 4. the decode's rules ----------------------------------------------------------------------------------------------------
def _decoded(c, exp):
    return PE.decode_statement(c["anchors"], c["deltas"].reshape(c["A"], 4), exp)


def test_threshold_cases_sit_on_the_float32_product(exp):
    assert np.log2(PE.MIN_SIZE_ODD) % 1 != 0
    assert [float(s) for s in PE.DECODE_SCALES] == [1.0, float(np.nextafter(F32(1), F32(2))), float(F32(1.6))]
    rounds_down = 0
    for scale in PE.DECODE_SCALES:
        c = PE.threshold_case(scale)
        thr = c["thr"]
        assert thr.dtype == F32 and thr == F32(PE.MIN_SIZE_ODD) * F32(scale)
        exact = np.float64(F32(PE.MIN_SIZE_ODD)) * np.float64(scale)
        rounds_down += float(thr) < exact
        b = _decoded(c, exp)
        assert np.array_equal(b[:, :2], np.zeros((7, 2), F32))
        for a, (w, h) in enumerate(c["sides"]):
            assert b[a, 2] - b[a, 0] + F32(1) == w and b[a, 3] - b[a, 1] + F32(1) == h and w.dtype == F32
        ts = [w for w, _ in c["sides"][:3]]
        assert ts[0] < thr == ts[1] < ts[2] and np.nextafter(ts[0], F32(99)) == thr and np.nextafter(thr, F32(99)) == ts[2]
        r = PE.proposal_statement(c, exp)
        assert list(r["valid_index"]) == [1, 2, 4, 5, 6]
        assert reported([c], exp, "size_gt") and list(PE.proposal_statement(c, exp, ("size_gt",))["valid_index"]) == [2, 5]
        if float(thr) < exact:                                               # the float64 threshold lies above the on-threshold side
            assert list(PE.proposal_statement(c, exp, ("size_f64",))["valid_index"]) == [2, 5]
    assert rounds_down >= 1


def test_clip_cases_sit_on_the_bounds(exp):
    px, py, boxes = PE.clip_cases()
    for c, axis, bound in ((px, 0, PE.CLIP_W - 1), (py, 1, PE.CLIP_H - 1)):
        b = _decoded(c, exp)
        assert np.array_equal(b[:, 0], c["points"][:, 0]) and np.array_equal(b[:, 2], c["points"][:, 0])     # the box IS the point
        assert np.array_equal(b[:, 1], c["points"][:, 1]) and np.array_equal(b[:, 3], c["points"][:, 1])
        v = c["points"][:, axis]
        assert v[0] == bound and v[1] == np.nextafter(F32(bound), F32(1e9)) and v[2] == np.nextafter(F32(bound), F32(0))
        assert v[3] == bound + 1 and v[4] == 0 and 0 < v[5] < 1e-44 and -1e-44 < v[6] < 0 and np.isinf(v[10]) and np.isinf(v[11])
        r = PE.proposal_statement(c, exp)
        assert r["valid"] == c["A"] and np.isfinite(r["boxes"]).all()
        got = r["boxes"][:, axis]                                            # distinct descending scores: anchor order
        assert list(got[:4]) == [bound, bound, v[2], bound] and list(got[4:8]) == [0, v[5], 0, 0]
        assert list(got[8:]) == [bound, 0, bound, 0]
    assert np.array_equal(_decoded(boxes, exp), boxes["decoded"])
    r = PE.proposal_statement(boxes, exp)
    W, H = PE.CLIP_W, PE.CLIP_H
    assert np.array_equal(r["boxes"], np.array(
        [[W - 16, 0, W - 1, 15], [W - 15, 0, W - 1, 15], [0, H - 16, 15, H - 1], [0, H - 15, 15, H - 1], [0, 0, 14, 15], [0, 0, 15, 14],
         [0, 0, 0, 0], [W - 1, H - 1, W - 1, H - 1], [0, 20, W - 1, 40], [20, 0, 40, H - 1], [0, 0, W - 1, H - 1]], F32))
    for mutant in ("clip_to_size", "clip_skips_y2"):
        assert reported([boxes], exp, mutant) and reported([py], exp, mutant), mutant
    assert reported([px], exp, "clip_to_size")


def test_exp_edge_case_straddles_the_cutoffs(exp):
    with np.errstate(over="ignore"):
        e = exp(np.array(PE.EXP_EDGES, F32))
    assert np.isfinite(e[0]) and e[0] > 3e38 and np.isposinf(e[1]) and np.isposinf(e[2])
    assert e[3] == 0 and e[4] == 0 and 0 < e[5] < np.finfo(F32).tiny
    c = PE.exp_edge_case()
    r = PE.proposal_statement(c, exp)
    assert r["valid"] == 12 and np.isfinite(r["boxes"]).all()
    assert r["boxes"][0, 2] == F32(0.5) * e[0] and r["boxes"][1, 2] == PE.FLT_MAX and r["boxes"][11, 2] == F32(2) * e[5]


# ---- 5. scan ----------------------------------------------------------------------------------------------------
def test_scan_cases_take_both_gather_paths(exp):
    assert PE.SCAN_POSTS == (4096, 4097, 6000)
    rows = {}
    for post in PE.SCAN_POSTS:
        r = PE.proposal_statement(PE.scan_case(post), exp)
        assert r["valid"] == 5000 and len(r["scores"]) == 5000 and len(r["rois"]) == min(post, 5000)
        assert (min(post, len(r["scores"])) > PE.K_SURV_CAP) == (post > 4096)
        rows[post] = r["rois"]
    assert np.array_equal(rows[4096], rows[4097][:4096]) and np.array_equal(rows[4097], rows[6000][:4097])
    none = PE.proposal_statement(PE.scan_case(300, 17.0), exp)
    assert none["valid"] == 0 and none["rois"].shape == (0, 5) and none["boxes"].shape == (0, 4)


# ---- stage bridge ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bridge_runs(exp):
    cases = PE.bridge_cases()
    return cases, [PE.bridge_statement_of(c, exp) for c in cases]


def test_bridge_cases_tie_and_stride(bridge_runs):
    cases, runs = bridge_runs
    assert {(c["R"], c["K"]) for c in cases} >= {(R, K) for R in PE.BRIDGE_RS for K in PE.BRIDGE_KS}
    for c, want in zip(cases, runs):
        R, K = c["R"], c["K"]
        assert want.shape == (R, 5) and want.dtype == F32 and not np.isnan(want).any()
        assert c["ld_bbox"] > 4 * K and c["ld_probs"] > K
        assert np.isnan(c["bbox"][:, 4 * K:]).all() and np.isnan(c["probs"][:, K:]).all()
        assert not np.isnan(c["bbox"][:, :4 * K]).any() and not np.isnan(c["probs"][:, :K]).any()
        if K >= 2 and R >= 3 and not c["name"].startswith("decode"):
            p = c["probs"][:, :K]
            ties = (p == p.max(axis=1, keepdims=True)).sum(axis=1)
            assert ties[0] >= 1 and (ties[2::4] == K).all() and (ties[0::4] <= 2).all() and (ties >= 2).sum() >= R // 2
            assert (p.argmax(axis=1) == 0).any() and (p.argmax(axis=1) > 0).any()


@pytest.mark.parametrize("mutant", ["argmax_last", "argmax_without_background", "clip_to_size", "clip_skips_y2"])
def test_bridge_mutants_are_reported(bridge_runs, exp, mutant):
    cases, runs = bridge_runs
    bad = [c["name"] for c, want in zip(cases, runs) if not np.array_equal(PE.bridge_statement_of(c, exp, (mutant,)), want)]
    assert bad
    if mutant.startswith("argmax"):
        assert {"R=%d K=%d" % (R, K) for R in PE.BRIDGE_RS[2:] for K in PE.BRIDGE_KS[1:]} <= set(bad)
        assert not [n for n in bad if n.endswith("K=1") or n.startswith("R=0")]


# ---- detect tail ----------------------------------------------------------------------------------------------------
def test_tail_table_and_rows():
    assert [float(s) for _, s in PE.TAIL_SCALES] == [1.0, float(F32(1.6)), float(F32(0.8)), float(F32(600.0 / 375.0)), float(F32(1.0 / 3.0))]
    for name, s in PE.TAIL_SCALES:
        assert PE.search_tail_numerators(s) == PE.TAIL_NUMERATORS[name]
        x = np.array(PE.TAIL_NUMERATORS[name], F32)
        assert (name == "1") == (len(x) == 0) and np.all(x / s != x * (F32(1) / s))
        rois = PE.tail_rows(name)
        q = rois[:, 1:] / s
        for k, bound in enumerate((PE.TAIL_W - 1, PE.TAIL_H - 1, PE.TAIL_W - 1, PE.TAIL_H - 1)):
            # no float32 over float32(1/3) gives 499 or 374 exactly: there the neighbouring quotients straddle the bound
            assert (q[:, k] == bound).any() or name == "1/3"
            assert ((q[:, k] > bound) & (q[:, k] < bound + 1e-3)).any() and ((q[:, k] < bound) & (q[:, k] > bound - 1e-3)).any()
            assert (q[:, k] > bound + 1).any() and (q[:, k] < 0).any() and (q[:, k] == 0).any()
        plain = PE.detect_tail_statement(rois, rois[:0], s, PE.TAIL_H, PE.TAIL_W)
        assert plain.shape == (len(rois), 4) and plain.min() == 0 and plain[:, 0].max() == PE.TAIL_W - 1 and plain[:, 1].max() == PE.TAIL_H - 1
        mutated = PE.detect_tail_statement(rois, rois[:0], s, PE.TAIL_H, PE.TAIL_W, ("reciprocal",))
        assert (name == "1") == np.array_equal(plain, mutated)
        assert not np.array_equal(plain, PE.detect_tail_statement(rois, rois[:0], s, PE.TAIL_H, PE.TAIL_W, ("clip_to_size",)))
    assert set(PE.TAIL_COUNTS) == {(0, 7), (7, 0), (1, 1), (300, 300), (0, 0)}
    a, b = PE.tail_case("1.6f", 300, 300)
    assert a.shape == b.shape == (300, 5) and not np.array_equal(a, b)


# ---- the exp sweep ----------------------------------------------------------------------------------------------------
def test_exp_sweep_patterns_and_the_rounded_mutant(exp):
    bits = PE.exp_sweep_patterns()
    x = bits.view(F32)
    assert bits.dtype == np.uint32 and 4_000_000 < len(bits) < 6_000_000 and np.all(np.diff(bits.astype(np.int64)) > 0)
    assert not np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert (bits % 1024 == 0).sum() >= (1 << 22) - (1 << 14)                 # the thinned space less its NaN patterns
    for centre in (PE.XMAX, PE.XMIN, F32(1), F32(0.0), F32(-0.0)):
        b = int(np.array(centre, F32).view(np.uint32))
        near = np.arange(b, b + 4097, dtype=np.uint32)
        assert np.isin(near, bits).all()
    for h in (-150.5, -0.5, 0.5, 127.5, 128.5):                               # quadrant = rint(x * log2(e)) flips at the half-integers
        b = int(np.array(h / PE.LOG2E, F32).view(np.uint32))
        near = np.arange(b - 64, b + 65, dtype=np.uint32)
        assert np.isin(near, bits).all()
        q = np.rint(near.view(F32).astype(np.float64) * PE.LOG2E)
        assert len(set(q.tolist())) == 2
    den = (x >= F32(-103.98)) & (x <= F32(-87.3))
    assert den.sum() > 500_000 and ((exp(x[den]) > 0) & (exp(x[den]) < np.finfo(F32).tiny)).sum() > 490_000
    # the two rois of the sweep make x2 the exp itself, resp. half of it; the rounded exp is told apart on the patterns around 1
    v = x[(x > 0.99) & (x < 1.01)]
    assert len(v) > 8000
    for roi, factor in zip(PE.SWEEP_ROIS, (F32(1), F32(0.5))):
        rois, d, p = PE.sweep_rows(v, roi)
        got = PE.stage_bridge_statement(rois, d, p, PE.FLT_MAX, PE.FLT_MAX, exp)
        assert np.array_equal(got[:, 3], factor * exp(v)) and np.array_equal(got[:, 4], got[:, 3]) and not got[:, :3].any()
        wrong = PE.stage_bridge_statement(rois, d, p, PE.FLT_MAX, PE.FLT_MAX, exp, ("exp_rounded",))
        assert 0.2 < float((wrong[:, 3] != got[:, 3]).mean()) < 0.6
    assert reported([PE.count_case(135)], exp, "exp_rounded") == []           # zero and -1 deltas: no exp bit reaches a result
