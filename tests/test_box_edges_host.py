"""The on-threshold corpora of tests/box_edge_inputs.py without a GPU: the corpus has the properties it claims (in Python
integers and Fractions), every plain statement agrees with the oracle -- and with the reference's own .cu code where oracle/_ref
is built -- and every variation of a rule that the issue names is told apart by at least one case of its section."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import box_edge_inputs as BE  # noqa: E402
import mnc_amd  # noqa: E402
from oracle import host as ohost  # noqa: E402
from oracle import native  # noqa: E402

mnc_amd.install_paths()
F32 = np.float32


# ---- 1. NMS ---------------------------------------------------------------------------------------------------------------
def test_nms_pairs_have_the_iou_of_their_class():
    for t in (0.3, 0.7):
        for cls in ("below", "on", "above"):
            assert len(BE.NMS_PAIRS[(t, cls)]) >= 4
    assert len(BE.NMS_PAIRS[(0.5, "on")]) >= 4 and (0.5, "below") not in BE.NMS_PAIRS and (0.5, "above") not in BE.NMS_PAIRS
    for (t, cls), pairs in BE.NMS_PAIRS.items():
        want = BE.nms_class_float(t, cls)
        assert (want < F32(t), want == F32(t), want > F32(t)) == (cls == "below", cls == "on", cls == "above")
        assert len(set(pairs)) == len(pairs)
        for a, b in pairs:
            inter, union, Sa, Sb = BE.pair_integers(a, b)
            assert 0 < inter < min(Sa, Sb)                                  # a partial overlap, neither box inside the other
            assert max(max(a), max(b), Sa, Sb, Sa + Sb) < 2 ** 24 and min(min(a), min(b)) >= 0
            got = BE.fraction_to_f32(Fraction(inter, union))
            assert got == want and got.tobytes() == want.tobytes(), (t, cls, a, b)
            i32, u32 = BE.iou32(np.array(a), np.array([b]))                 # the float32 statement sees the same integers
            assert int(i32[0]) == inter and int(u32[0]) == union and i32[0] / u32[0] == want


def test_fraction_rounding_is_numpy_s():
    rng = np.random.default_rng(1)
    for _ in range(500):
        p, q = (int(v) for v in rng.integers(1, 2 ** 24, 2))
        assert BE.fraction_to_f32(Fraction(p, q)) == F32(p) / F32(q)
    assert BE.fraction_to_f32(Fraction(2 ** 24 + 1, 2 ** 24)) == F32(1)     # a tie goes to the even neighbour
    assert BE.fraction_to_f32(Fraction(2 ** 24 + 3, 2 ** 24)) == F32(1 + 2.0 ** -22)


def test_search_finds_a_pair_of_each_class():
    """The committed table is what the search gives; one pair per class is searched again here (well under a second each)."""
    for t in (0.3, 0.7):
        for cls in ("below", "on", "above"):
            (a, b), = BE.search_nms_pairs(BE.nms_class_float(t, cls), 1, seed=3 * int(10 * t) + len(cls))
            assert (a, b) == BE.NMS_PAIRS[(t, cls)][0]
    assert BE.search_near_half(1) == BE.NEAR_HALF["below"] and BE.search_near_half(-1) == BE.NEAR_HALF["above"]


def test_placements_cover_every_position_and_size():
    pl = BE.nms_placements()
    assert {(i, j) for _, _, _, i, j, _ in pl} == set(BE.NMS_POSITIONS)
    assert {n for _, _, _, _, _, n in pl} == set(BE.NMS_SIZES)
    for t in (0.3, 0.7):
        for cls in ("below", "on", "above"):
            assert {(i, j) for tt, c, _, i, j, _ in pl if (tt, c) == (t, cls)} == set(BE.NMS_POSITIONS)
    dets = BE.place_pair(BE.NMS_PAIRS[(0.3, "on")][0], 63, 127, 129)
    assert np.all(np.diff(dets[:, 4]) < 0)
    inter = [BE.pair_integers(dets[p, :4].astype(int), dets[q, :4].astype(int))[0] for p in range(129) for q in range(p)]
    assert sum(1 for v in inter if v) == 1                                   # the pair alone overlaps


@pytest.fixture(scope="module")
def nms_runs():
    """(placement, dets, statement bits, statement keep) of every placement, computed once."""
    out = []
    for (t, cls, k, i, j, n) in BE.nms_placements():
        dets = BE.place_pair(BE.NMS_PAIRS[(t, cls)][k], i, j, n)
        bits, keep = BE.nms_statement(dets, t)
        out.append(((t, cls, k, i, j, n), dets, bits, keep))
    return out


def test_nms_statement_expected_and_oracle(nms_runs):
    for (t, cls, k, i, j, n), dets, bits, keep in nms_runs:
        want = [p for p in range(n) if p != j] if cls == "above" else list(range(n))
        assert keep == want, (t, cls, i, j, n)
        assert np.triu(bits, 1).sum() == (1 if cls == "above" else 0) and bits[i, j] == (cls == "above")
        assert np.array_equal(native.nms_sorted(dets, t), keep)
        assert np.array_equal(native.nms_mask(dets, t), BE.mask_words(bits))
        if native.ref_available():
            assert np.array_equal(native.ref_nms_sorted(dets, t), keep)


@pytest.mark.parametrize("mutant,caught_by", [("ge", "on"), ("mul", None)])
def test_nms_mutants_are_reported(nms_runs, mutant, caught_by):
    bad = [(t, cls) for (t, cls, k, i, j, n), dets, bits, keep in nms_runs if BE.nms_statement(dets, t, mutant)[1] != keep]
    if caught_by:
        assert {c for _, c in bad} == {caught_by} and {t for t, _ in bad} == {0.3, 0.5, 0.7}
    # the degenerate boxes are cases of this section too: a negative union tells the product form from the quotient
    odd = [name for name, dets, thr, _ in BE.degenerate_cases()
           if BE.nms_statement(dets, thr, mutant)[1] != BE.nms_statement(dets, thr)[1]]
    assert bad or odd
    if mutant == "mul":
        assert "small against inverted" in odd


def test_degenerate_boxes_statement_and_oracle():
    for name, dets, thr, want in BE.degenerate_cases():
        bits, keep = BE.nms_statement(dets, thr)
        assert np.isfinite(dets).all()
        if want is not None:
            assert keep == want, name
        assert np.array_equal(native.nms_sorted(dets, thr), keep), name
        assert np.array_equal(native.nms_mask(dets, thr), BE.mask_words(bits)), name
        if native.ref_available():
            assert np.array_equal(native.ref_nms_sorted(dets, thr), keep), name
    z = np.array(BE.degenerate_cases()[7][1][0, :4])
    inter, union = BE.iou32(z, z[None])
    with np.errstate(invalid="ignore"):
        assert np.isnan(inter / union)[0]


# ---- 2. bbox_overlaps and membership ------------------------------------------------------------------------------------------
def test_half_pairs_and_their_neighbours():
    for a, b in BE.HALF_PAIRS:
        inter, union, _, _ = BE.pair_integers(a, b)
        assert union == 2 * inter
        assert BE.overlaps_statement([a], [b])[0, 0] == 0.5
    lo = Fraction(*BE.pair_integers(*BE.NEAR_HALF["below"])[:2])
    hi = Fraction(*BE.pair_integers(*BE.NEAR_HALF["above"])[:2])
    assert lo == Fraction(2792790, 5585581) and hi == Fraction(2790744, 5581487)
    assert lo.denominator == 2 * lo.numerator + 1 and hi.denominator == 2 * hi.numerator - 1
    for pair in BE.NEAR_HALF.values():
        assert max(pair[0][2] - pair[0][0], pair[0][3] - pair[0][1], pair[1][2] - pair[1][0], pair[1][3] - pair[1][1]) + 1 < 2048
    flo = BE.overlaps_statement([BE.NEAR_HALF["below"][0]], [BE.NEAR_HALF["below"][1]])[0, 0]
    fhi = BE.overlaps_statement([BE.NEAR_HALF["above"][0]], [BE.NEAR_HALF["above"][1]])[0, 0]
    assert flo < 0.5 < fhi and flo == lo.numerator / lo.denominator and fhi == hi.numerator / hi.denominator
    for (a, b), inter in BE.TOUCHING_PAIRS:
        assert BE.pair_integers(a, b)[0] == inter
        got = BE.overlaps_statement([a], [b])[0, 0]
        assert (got > 0) == (inter > 0) and got == inter / BE.pair_integers(a, b)[1]


def _all_pairs():
    pairs = list(BE.HALF_PAIRS) + list(BE.NEAR_HALF.values()) + [p for p, _ in BE.TOUCHING_PAIRS]
    return np.array([p[0] for p in pairs], np.float64), np.array([p[1] for p in pairs], np.float64)


def test_overlaps_statement_equals_oracle():
    a, b = _all_pairs()
    assert np.array_equal(BE.overlaps_statement(a, b), native.bbox_overlaps(a, b))
    assert np.array_equal(BE.overlaps_statement(b, a), native.bbox_overlaps(b, a))
    for n, m in BE.VOTING_SETS:
        v = BE.voting_set(n, m)
        bx = v["boxes"].astype(np.float64)
        assert np.array_equal(BE.overlaps_statement(bx, bx[:2]), native.bbox_overlaps(bx, bx[:2]))


@pytest.fixture(scope="module")
def voting_runs():
    out = []
    for n, m in BE.VOTING_SETS:
        v = BE.voting_set(n, m)
        want = ohost.gpu_mask_voting(v["masks"], v["boxes"], v["scores"], v["num_classes"], v["max_per_image"], v["W"], v["H"])
        out.append((v, want))
    return out


def test_voting_sets_sit_on_the_threshold(voting_runs):
    assert {m for _, m in BE.VOTING_SETS} == {1, 63, 64, 129}
    for v, want in voting_runs:
        idx, bx = v["idx"], v["boxes"].astype(np.float64)
        assert idx["M"] in (1, 63, 64, 129) and v["n"] <= 130 and v["W"] <= 101 and v["H"] <= 77
        ov = BE.overlaps_statement(bx, bx[idx["K"]][None])[:, 0]
        assert ov[idx["M"]] == 0.5 and 0.4999 < ov[idx["L"]] < 0.5
        members = {idx["K"], idx["M"]}
        if "J" in idx:
            assert 0.5 < ov[idx["J"]] < 0.5001
            members.add(idx["J"])
        assert set(BE.members_statement(bx, bx[idx["K"]])) == members
        assert set(BE.members_statement(bx, bx[idx["M"]])) >= {idx["K"], idx["M"], idx["L"]}
        # K is kept in class 1 and suppresses M, L and J at 0.3; the fillers overlap nothing
        keep = native.gpu_nms(np.hstack((v["boxes"], v["scores"][:, 1:2])), 0.3)
        assert keep[0] == idx["K"] and not set(keep) & (set(idx.values()) - {idx["K"]})
        assert len(keep) == v["n"] - (len(idx) - 1)
        lm, lb = want
        assert np.array_equal(lb[0][0, :4], [10, 10, 49, 39])               # with M a member the voted box reaches x = 49


def test_membership_has_teeth(voting_runs):
    """Without M in K's set the voted box and mask of K change: the oracle with M's overlap zeroed differs."""
    for v, want in voting_runs:
        m = v["idx"]["M"]
        k_box = v["boxes"][v["idx"]["K"]].astype(np.float64)

        def without_m(boxes, query):
            ov = native.bbox_overlaps(boxes, query)
            if np.array_equal(query[0], k_box):
                ov[m] = 0.0
            return ov
        lm, lb = ohost.gpu_mask_voting(v["masks"], v["boxes"], v["scores"], v["num_classes"], v["max_per_image"], v["W"], v["H"],
                                       overlaps_fn=without_m)
        assert np.array_equal(lb[0][0, :4], [10, 10, 19, 39]) and not np.array_equal(lm[0][0], want[0][0][0])
        assert np.array_equal(lb[1], want[1][1]) and np.array_equal(lm[1], want[0][1])


@pytest.mark.parametrize("mutant", ["gt", "f32thr"])
def test_membership_mutants_are_reported(voting_runs, mutant):
    for v, _ in voting_runs:
        bx = v["boxes"].astype(np.float64)
        k = bx[v["idx"]["K"]]
        assert set(BE.members_statement(bx, k)) - set(BE.members_statement(bx, k, mutant)) == {v["idx"]["M"]}
    a, b = _all_pairs()
    for p in range(len(BE.HALF_PAIRS)):
        assert len(BE.members_statement(a[p:p + 1], b[p])) == 1 and len(BE.members_statement(a[p:p + 1], b[p], mutant)) == 0


# ---- 3. binarisation ------------------------------------------------------------------------------------------------------------
def test_levels_are_neighbouring_floats():
    (_, lo), (_, on), (_, hi) = BE.BIN_LEVELS
    assert lo < on < hi and np.nextafter(lo, F32(1)) == on and np.nextafter(on, F32(1)) == hi
    assert on == F32(0.4) and float(on) > 0.4 > float(lo)                   # float32(0.4) lies above the double 0.4
    assert BE.MV_W % 2 == 1 and BE.MV_H % 2 == 1 and BE.MV_W <= 101 and BE.MV_H <= 77


def test_mv_statement_expected_and_oracle():
    centre = [BE.MV_W // 2, BE.MV_H // 2, BE.MV_W // 2, BE.MV_H // 2]
    full = [BE.MV_X, BE.MV_Y, BE.MV_X + 20, BE.MV_Y + 20]
    for name, c in BE.mv_cases():
        box = BE.mv_box_statement(c)
        if name.endswith("below") or name.endswith(" on"):
            assert list(box) == centre, name
        elif name.endswith("above"):
            assert list(box) == full, name
        else:
            py, px = (int(s) for s in name.split()[1:])
            assert list(box) == [BE.MV_X + px, BE.MV_Y + py, BE.MV_X + px, BE.MV_Y + py], name
        om, ob = native.mv(*BE.mv_args(c))
        assert np.array_equal(ob[0], box), name
        if native.ref_available():
            rm, rb = native.ref_mv(*BE.mv_args(c))
            assert np.array_equal(rb, ob) and np.array_equal(rm, om), name


@pytest.mark.parametrize("mutant", ["ge", "f64"])
def test_binarise_mutants_are_reported(mutant):
    bad = [name for name, c in BE.mv_cases() if not np.array_equal(BE.mv_box_statement(c, mutant), BE.mv_box_statement(c))]
    assert "const on" in bad and "halves on" in bad and "pixel 10 10" in bad
    assert not [name for name in bad if name.endswith("below") or name.endswith("above")]


def test_image_vote_statement_and_mutant():
    got = {name: BE.image_vote_statement(BE.image_vote_case(v)) for name, v in BE.BIN_LEVELS}
    centre = [BE.MV_W // 2, BE.MV_H // 2, BE.MV_W // 2, BE.MV_H // 2]
    full = [BE.MV_X, BE.MV_Y, BE.MV_X + 20, BE.MV_Y + 20]
    assert list(got["below"][0]) == centre and not got["below"][1].any()
    for name in ("on", "above"):
        assert list(got[name][0]) == full and (got[name][1] == 1).all()
    mut = BE.image_vote_statement(BE.image_vote_case(F32(BE.BIN)), "gt")
    assert list(mut[0]) == centre


def test_instance_mask_statement_host_rule_and_mutant():
    from transform.mask_transform import instance_masks_numpy
    boxes, masks, H, W = BE.instance_mask_case()
    want = BE.instance_mask_statement(masks)
    assert not want[0].any() and want[1].all() and want[2].all() and want[3].sum() == 440 and not want[3, 6, 13]
    pm = instance_masks_numpy(boxes, masks, H, W, binarize_thresh=BE.BIN)
    for i in range(len(boxes)):
        assert np.array_equal(pm.dense(i), want[i])
    mut = BE.instance_mask_statement(masks, "gt")
    assert not mut[1].any() and np.array_equal(mut[2], want[2])


def test_score_statement_and_mutant():
    told = False
    for thr, scores, kept in BE.SCORE_CASES:
        assert tuple(BE.score_statement(scores, thr)) == kept
        told |= tuple(BE.score_statement(scores, thr, "f32")) != kept
    assert told
    assert tuple(BE.score_statement(BE.SCORE_CASES[0][1], 0.3, "f32")) == BE.SCORE_CASES[0][2]   # at 0.3 both forms agree


# ---- 4. ROIPooling ------------------------------------------------------------------------------------------------------------
def test_roi_corpus_lands_on_halves():
    rois = BE.roi_cases()
    scaled = rois[:, 1:] * F32(BE.ROI_SCALE)
    vals = set(float(v) for v in scaled.ravel())
    assert {0.5, 1.5, 2.5, 3.5, -0.5, float(F32(0.49999997))} <= vals
    assert float(F32(0.49999997)) < 0.5 and F32(0.49999997) + F32(0.5) == F32(1)
    x = np.array([0.5, 1.5, 2.5, 3.5, -0.5, 0.49999997, 8.5, -1.5, 7.0], F32)
    assert list(BE.round_half_away(x)) == [1, 2, 3, 4, -1, 0, 9, -2, 7]
    assert list(np.rint(x[:4]).astype(int)) == [0, 2, 2, 4]
    assert list(np.floor(x[4:6] + F32(0.5)).astype(int)) == [0, 1]
    feat = BE.roi_feature()
    assert feat.shape == (1, BE.ROI_C, BE.ROI_H, BE.ROI_W) and len(np.unique(feat)) == feat.size
    sides = set()
    for r in rois:
        x1, y1, x2, y2 = BE.round_half_away(r[1:] * F32(BE.ROI_SCALE))
        sides |= {int(x2 - x1 + 1), int(y2 - y1 + 1)}
    assert {7, 14, 15, 21, 22} <= sides


def test_roi_corpus_has_bins_where_float32_and_exact_edges_differ():
    """7 * float32(57 / 7) is 57.000004: ceilf gives 58 where the exact rational gives 57 (and so Caffe's layer pools one more row;
    conv5_3 of a 600 x 1000 image is 38 x 63, so the product meets a side of 57).  The corpus holds such bins with the differing edge
    inside the map, and at every other side the float32 edges equal the exact ones."""
    differ = []
    for roi in BE.roi_cases():
        x1, y1, x2, y2 = (int(v) for v in BE.round_half_away(roi[1:] * F32(BE.ROI_SCALE)))
        for P in BE.ROI_P:
            for side, lo, size in ((max(y2 - y1 + 1, 1), y1, BE.ROI_H), (max(x2 - x1 + 1, 1), x1, BE.ROI_W)):
                b = F32(side) / F32(P)
                for p in range(P):
                    assert int(np.floor(F32(p) * b)) == math.floor(Fraction(p * side, P))
                    got, exact = int(np.ceil(F32(p + 1) * b)), math.ceil(Fraction((p + 1) * side, P))
                    if got != exact:
                        assert side in BE.ROI_LONG_SIDES and P == 7 and got == exact + 1
                        differ.append((side, 0 <= exact + lo < got + lo <= size))
    assert {s for s, _ in differ} == set(BE.ROI_LONG_SIDES) and all(inside for _, inside in differ)


@pytest.fixture(scope="module")
def roi_runs():
    feat, rois = BE.roi_feature(), BE.roi_cases()
    return feat, rois, {P: BE.roi_pool_statement(feat, rois, P, P) for P in BE.ROI_P}


def test_roi_statement_equals_oracle(roi_runs):
    feat, rois, want = roi_runs
    for P in BE.ROI_P:
        assert np.array_equal(native.roi_pool(feat, rois, P, P, BE.ROI_SCALE), want[P])
        assert want[P].any()


@pytest.mark.parametrize("mutant", ["rint", "floor", "exact"])
def test_roi_mutants_are_reported(roi_runs, mutant):
    feat, rois, want = roi_runs
    for P in BE.ROI_P:
        got = BE.roi_pool_statement(feat, rois, P, P, mutant=mutant)
        bad = np.where((got != want[P]).reshape(len(rois), -1).any(1))[0]
        assert len(bad) or (mutant == "exact" and P == 2), (mutant, P)
