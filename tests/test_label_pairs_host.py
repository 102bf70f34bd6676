"""The numpy statements of mnc_amd.pairs and mnc_amd.panoptic (label_pairs_numpy, confusion, semantic_scores, pq_image_numpy,
PanopticEval with device=False) against facts that do not come from them: scikit-learn's contingency_matrix and confusion_matrix, a
double loop over (a == i) & (b == j), np.bincount, a hand-computed 3-class example, panoptic scenes whose counts are known by
construction and a brute force over boolean masks.  Every comparison of integers is exact.  No GPU is needed or touched."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import label_pairs_inputs as PI  # noqa: E402
import mask_labels_inputs as LI  # noqa: E402
from mnc_amd import pairs as PR  # noqa: E402
from mnc_amd import panoptic as PQ  # noqa: E402

HOST_CASES = sorted(k for k in PI.CASES if k not in ("one_pair", "most_cells"))


# ---- the pair table ----

@pytest.mark.parametrize("name", HOST_CASES)
def test_statement_against_sklearn_contingency_matrix(name):
    from sklearn.metrics.cluster import contingency_matrix
    a, b = PI.get(name)
    t = PI.reference(name)
    m = contingency_matrix(a.ravel(), b.ravel(), sparse=True).tocsr()
    m.sort_indices()
    assert t.a_ids.dtype == t.b_ids.dtype == t.ia.dtype == t.ib.dtype == np.int32 and t.count.dtype == np.int64
    assert np.array_equal(t.a_ids, np.unique(a)) and np.array_equal(t.b_ids, np.unique(b))
    assert np.array_equal(t.row_ptr, m.indptr) and t.row_ptr.dtype == np.int64
    assert np.array_equal(t.ib, m.indices) and np.array_equal(t.count, m.data)
    assert np.array_equal(t.ia, np.repeat(np.arange(t.a_ids.size), np.diff(m.indptr)))
    assert (t.count > 0).all() and int(t.count.sum()) == a.size


@pytest.mark.parametrize("name", HOST_CASES)
def test_areas_are_bincounts_and_the_key_rule(name):
    a, b = PI.get(name)
    t = PI.reference(name)
    assert np.array_equal(t.a_areas, np.bincount(a.ravel())[t.a_ids]) and t.a_areas.dtype == np.int64
    assert np.array_equal(t.b_areas, np.bincount(b.ravel())[t.b_ids]) and t.b_areas.dtype == np.int64
    key, count = np.unique((a.astype(np.int64) << 24) | b, return_counts=True)
    assert np.array_equal((t.a_ids[t.ia].astype(np.int64) << 24) | t.b_ids[t.ib], key) and np.array_equal(t.count, count)
    order = np.lexsort((t.ib, t.ia))
    assert np.array_equal(order, np.arange(len(t)))


@pytest.mark.parametrize("name", PI.SMALL)
def test_statement_against_the_double_loop(name):
    a, b = PI.get(name)
    t = PI.reference(name)
    dense = t.dense()
    assert dense.dtype == np.int64 and dense.shape == (t.a_ids.size, t.b_ids.size)
    for r, i in enumerate(t.a_ids):
        for c, j in enumerate(t.b_ids):
            n = int(((a == i) & (b == j)).sum())
            assert dense[r, c] == n and t.get(int(i), int(j)) == n
    assert t.get(int(t.a_ids[-1]) + 1, int(t.b_ids[0])) == 0 and t.get(int(t.a_ids[0]), int(t.b_ids[-1]) + 1) == 0


def test_without_drops_rows_and_columns():
    a, b = PI.get("size_65x130")
    t = PI.reference("size_65x130")
    drop_a, drop_b = [int(t.a_ids[1]), 999999], [int(t.b_ids[0]), int(t.b_ids[-1])]
    w = t.without(a_values=drop_a, b_values=drop_b)
    keep = ~np.isin(a, drop_a) & ~np.isin(b, drop_b)
    key, count = np.unique((a[keep].astype(np.int64) << 24) | b[keep], return_counts=True)
    assert np.array_equal(w.a_ids, np.setdiff1d(t.a_ids, drop_a)) and np.array_equal(w.b_ids, np.setdiff1d(t.b_ids, drop_b))
    assert np.array_equal((w.a_ids[w.ia].astype(np.int64) << 24) | w.b_ids[w.ib], key) and np.array_equal(w.count, count)
    assert PI.same_pairs(t.without(), t)
    for f in PR.LabelPairs.FIELDS:
        assert getattr(w, f).dtype == getattr(t, f).dtype


def test_other_dtypes_and_what_the_statement_refuses():
    a, b = PI.get("size_2x65")
    for dtype in (np.uint8, np.int64, np.uint16):
        assert PI.same_pairs(PR.label_pairs_numpy(a.astype(dtype), b.astype(np.int64)), PI.reference("size_2x65"))
    with pytest.raises(ValueError, match=r"not in \[0, 16777216\)"):
        PR.label_pairs_numpy(np.where(a == a.max(), 2 ** 24, a), b)
    with pytest.raises(ValueError, match=r"not in \[0, 16777216\)"):
        PR.label_pairs_numpy(a, np.where(b == b.max(), -1, b))
    with pytest.raises(ValueError, match="shape"):
        PR.label_pairs_numpy(a, b[:, :-1])
    with pytest.raises(ValueError):
        PR.label_pairs_numpy(a.astype(np.float32), b)
    with pytest.raises(ValueError, match="2048 x 2049.*4196352"):
        PR.label_pairs_numpy(*PI.get("most_cells_plus_one"))
    ids = np.arange(65540, dtype=np.int32).reshape(4, 16385)
    with pytest.raises(ValueError, match="65540 and 1 distinct values"):
        PR.label_pairs_numpy(ids, np.zeros_like(ids))
    t = PI.reference("most_cells")
    assert t.a_ids.size * t.b_ids.size == PR.MAX_CELLS == 2 ** 22 and PR.LDS_CELLS == 16384 and PR.MAX_IDS == 65536


# ---- the semantic scores ----

def test_confusion_against_sklearn():
    from sklearn.metrics import confusion_matrix
    gt, pred = PI.class_pair()
    conf = PR.confusion(gt, pred, 21, device=False)
    keep = gt != 255
    assert conf.dtype == np.int64 and conf.shape == (21, 21)
    assert np.array_equal(conf, confusion_matrix(gt[keep], pred[keep], labels=np.arange(21)))
    assert np.array_equal(conf, np.bincount(21 * gt[keep].astype(np.int64) + pred[keep], minlength=441).reshape(21, 21))
    every = PR.confusion(np.where(gt == 255, 0, gt), pred, 21, ignore=None, device=False)
    assert int(every.sum()) == gt.size
    with pytest.raises(ValueError, match="gt value 255"):
        PR.confusion(gt, pred, 21, ignore=None, device=False)
    with pytest.raises(ValueError, match="pred value 20 "):
        PR.confusion(np.where(gt == 20, 0, gt), pred, 20, device=False)
    with pytest.raises(ValueError, match="gt value 254"):
        PR.confusion(np.where(gt == 255, 254, gt), pred, 21, device=False)


def test_semantic_scores_by_hand_perfect_and_permuted():
    conf = np.array([[3, 1, 0], [0, 2, 2], [1, 0, 1]], np.int64)     # rows 4, 4, 2; columns 4, 3, 3; 10 pixels
    s = PR.semantic_scores(conf)
    assert s["pixel_acc"] == 6 / 10
    assert s["mean_acc"] == (3 / 4 + 2 / 4 + 1 / 2) / 3
    assert s["miou"] == (3 / 5 + 2 / 5 + 1 / 4) / 3
    assert s["fwiou"] == (4 * (3 / 5) + 4 * (2 / 5) + 2 * (1 / 4)) / 10
    wide = np.zeros((5, 5), np.int64)                                # two classes that do not occur in gt: left out of the means
    wide[:3, :3] = conf
    wide[0, 4] = 2                                                   # (predicted, never true: the union of class 0 grows, no row 4)
    w = PR.semantic_scores(wide)
    assert w["mean_acc"] == (3 / 6 + 2 / 4 + 1 / 2) / 3 and w["pixel_acc"] == 6 / 12
    gt, pred = PI.class_pair()
    perfect = PR.semantic_scores(PR.confusion(gt, np.where(gt == 255, 0, gt), 21, device=False))
    assert perfect == {"pixel_acc": 1.0, "mean_acc": 1.0, "miou": 1.0, "fwiou": 1.0}
    perm = np.random.default_rng(7).permutation(21)
    table = np.concatenate([perm, np.full(256 - 21, 255)]).astype(np.int32)
    c0, c1 = PR.confusion(gt, pred, 21, device=False), PR.confusion(table[gt], table[pred], 21, device=False)
    assert np.array_equal(c1[np.ix_(perm, perm)], c0)
    assert PR.semantic_scores(c1)["pixel_acc"] == PR.semantic_scores(c0)["pixel_acc"]


# ---- panoptic quality ----

H = 6


def counts(r):
    return {c: (s["tp"], s["fp"], s["fn"], s["matches"]) for c, s in r.items()}


def test_identical_maps_score_one():
    gt, gs, _, _ = PI.random_scene(3)
    gs = [PI.seg(s["id"], s["category_id"]) for s in gs]
    ev = PQ.PanopticEval(PI.CATEGORIES, device=False)
    r = ev.add("im", gt, gs, gt, gs)
    for c, s in r.items():
        n = len([g for g in gs if g["category_id"] == c])
        assert (s["tp"], s["fp"], s["fn"]) == (n, 0, 0) and all(i == u for i, u in s["matches"])
    out = ev.summarize()
    present = sorted({g["category_id"] for g in gs})
    assert out["All"] == {"pq": 1.0, "sq": 1.0, "rq": 1.0, "n": len(present)}
    for c in present:
        assert (out["per_class"][c]["pq"], out["per_class"][c]["sq"], out["per_class"][c]["rq"]) == (1.0, 1.0, 1.0)


def test_iou_of_exactly_one_half_is_no_match_and_three_fifths_is():
    # the rest of the ground truth is a stuff segment, 1: nothing of the prediction lies on void
    gs = [PI.seg(1, 3), PI.seg(5, 1)]
    gt, pred = PI.columns(H, 8, [(1, 0, 7), (5, 0, 2)]), PI.columns(H, 8, [(9, 1, 3)])
    r = PQ.pq_image_numpy(gt, gs, pred, [PI.seg(9, 1)], PI.CATEGORIES)
    assert counts(r)[1] == (0, 1, 1, []) and counts(r)[2] == (0, 0, 0, []) and counts(r)[3] == (0, 0, 1, [])
    # on void instead, the prediction's fourth column leaves the union: 2 / 3, a match
    r = PQ.pq_image_numpy(PI.columns(H, 8, [(5, 0, 2)]), [PI.seg(5, 1)], pred, [PI.seg(9, 1)], PI.CATEGORIES)
    assert counts(r)[1] == (1, 0, 0, [(2 * H, 3 * H)])
    gt, pred = PI.columns(H, 8, [(1, 0, 7), (5, 0, 3)]), PI.columns(H, 8, [(9, 1, 4)])
    r = PQ.pq_image_numpy(gt, gs, pred, [PI.seg(9, 1)], PI.CATEGORIES)
    assert counts(r)[1] == (1, 0, 0, [(3 * H, 5 * H)]) and counts(r)[3] == (0, 0, 1, [])
    gt = PI.columns(H, 8, [(5, 0, 3), (1, 4, 4)])
    ev = PQ.PanopticEval(PI.CATEGORIES, device=False)
    ev.add(0, gt, [PI.seg(5, 1)], pred, [PI.seg(9, 1)])
    assert ev.summarize()["All"] == {"pq": 3 / 5, "sq": 3 / 5, "rq": 1.0, "n": 1}


def test_void_and_crowd_absorb_and_another_class_does_not():
    # gt 5 (category 1) on columns 0 .. 3; pred 9 on columns 6 .. 8, two thirds of it (7, 8) on void, one third on gt 6
    gt = PI.columns(H, 10, [(5, 0, 3), (6, 4, 6)])
    pred = PI.columns(H, 10, [(8, 0, 3), (9, 6, 8)])
    gs, ps = [PI.seg(5, 1), PI.seg(6, 2)], [PI.seg(8, 1), PI.seg(9, 1)]
    r = counts(PQ.pq_image_numpy(gt, gs, pred, ps, PI.CATEGORIES))
    assert r[1] == (1, 0, 0, [(4 * H, 4 * H)]) and r[2] == (0, 0, 1, [])          # pred 9: neither a match nor a false positive
    gt2 = PI.columns(H, 10, [(5, 0, 3), (6, 4, 6), (7, 7, 8)])                    # the void under pred 9 labelled: category 2, no crowd
    r = counts(PQ.pq_image_numpy(gt2, gs + [PI.seg(7, 2)], pred, ps, PI.CATEGORIES))
    assert r[1] == (1, 1, 0, [(4 * H, 4 * H)]) and r[2] == (0, 0, 2, [])          # a false positive
    r = counts(PQ.pq_image_numpy(gt2, gs + [PI.seg(7, 1, crowd=1)], pred, ps, PI.CATEGORIES))
    assert r[1] == (1, 0, 0, [(4 * H, 4 * H)]) and r[2] == (0, 0, 1, [])          # a crowd of its category absorbs it, is no fn
    r = counts(PQ.pq_image_numpy(gt2, gs + [PI.seg(7, 2, crowd=1)], pred, ps, PI.CATEGORIES))
    assert r[1] == (1, 1, 0, [(4 * H, 4 * H)]) and r[2] == (0, 0, 1, [])          # a crowd of another category does not
    # a crowd is never matched, however well it is covered; the last crowd of a category is the one that absorbs
    r = counts(PQ.pq_image_numpy(gt, [PI.seg(5, 1, crowd=1), PI.seg(6, 2)], pred, ps, PI.CATEGORIES))
    assert r[1] == (0, 0, 0, []) and r[2] == (0, 0, 1, [])
    gt3 = PI.columns(H, 10, [(5, 0, 3), (6, 4, 5), (7, 6, 8)])
    pred3 = PI.columns(H, 10, [(8, 0, 3), (9, 6, 7), (10, 8, 8)])
    both, ps3 = [PI.seg(7, 1, crowd=1), PI.seg(5, 1, crowd=1), PI.seg(6, 2)], ps + [PI.seg(10, 1)]
    r = counts(PQ.pq_image_numpy(gt3, both, pred3, ps3, PI.CATEGORIES))
    assert r[1] == (0, 2, 0, [])                                                  # 5 is kept: it absorbs pred 8; 7 no longer 9 and 10
    r = counts(PQ.pq_image_numpy(gt3, both[::-1], pred3, ps3, PI.CATEGORIES))
    assert r[1] == (0, 1, 0, [])                                                  # 7 is kept: it absorbs 9 and 10; 5 no longer pred 8


def test_the_three_sanity_errors():
    gt, pred = PI.columns(H, 8, [(5, 0, 3)]), PI.columns(H, 8, [(9, 1, 4), (4, 6, 7)])
    gs = [PI.seg(5, 1)]
    with pytest.raises(KeyError, match="4 is in the predicted map"):
        PQ.pq_image_numpy(gt, gs, pred, [PI.seg(9, 1)], PI.CATEGORIES)
    with pytest.raises(KeyError, match=r"\[77\]"):
        PQ.pq_image_numpy(gt, gs, pred, [PI.seg(9, 1), PI.seg(4, 1), PI.seg(77, 1)], PI.CATEGORIES)
    with pytest.raises(KeyError, match="unknown category 12"):
        PQ.pq_image_numpy(gt, gs, pred, [PI.seg(9, 1), PI.seg(4, 12)], PI.CATEGORIES)
    ev = PQ.PanopticEval(PI.CATEGORIES, device=False)
    ev.add("a", gt, gs, pred, [PI.seg(9, 1), PI.seg(4, 1)])
    with pytest.raises(ValueError, match="added before"):
        ev.add("a", gt, gs, pred, [PI.seg(9, 1), PI.seg(4, 1)])


def brute_force(gt, gs, pred, ps):
    """The published loop on boolean masks map == id per segment; no pair table."""
    out = {c: [0, 0, 0, []] for c in PI.CATEGORIES}
    void = gt == PQ.VOID
    g_hit, p_hit = set(), set()
    for g in sorted(gs, key=lambda s: s["id"]):
        for p in sorted(ps, key=lambda s: s["id"]):
            G, P = gt == g["id"], pred == p["id"]
            inter = int((G & P).sum())
            if inter == 0 or g["iscrowd"] or g["category_id"] != p["category_id"]:
                continue
            union = int(P.sum()) + int(G.sum()) - inter - int((P & void).sum())
            if inter / union > 0.5:
                out[g["category_id"]][0] += 1
                out[g["category_id"]][3].append((inter, union))
                g_hit.add(g["id"])
                p_hit.add(p["id"])
    crowd = {}
    for g in gs:
        if g["iscrowd"]:
            crowd[g["category_id"]] = g["id"]
        elif g["id"] not in g_hit:
            out[g["category_id"]][2] += 1
    for p in ps:
        if p["id"] in p_hit:
            continue
        P = pred == p["id"]
        covered = int((P & void).sum())
        if p["category_id"] in crowd:
            covered += int((P & (gt == crowd[p["category_id"]])).sum())
        if covered / int(P.sum()) > 0.5:
            continue
        out[p["category_id"]][1] += 1
    return {c: tuple(v) for c, v in out.items()}


@pytest.mark.parametrize("seed", range(12))
def test_random_scenes_against_the_brute_force_and_relabelling(seed):
    gt, gs, pred, ps = PI.random_scene(seed)
    r = counts(PQ.pq_image_numpy(gt, gs, pred, ps, PI.CATEGORIES))
    assert r == brute_force(gt, gs, pred, ps)
    # relabelling the ids of either map by a permutation that keeps their order changes nothing; one that does not keep it may
    # reorder the matches of a category, never the sets
    rng = np.random.default_rng(seed)
    for which in (0, 1):
        src = gt if which == 0 else pred
        ids = np.unique(src)
        ids = ids[ids != 0]                                                  # (0 is void in either map)
        table = np.zeros(int(src.max()) + 1, np.int32)
        table[ids] = rng.permutation(np.arange(1, 400))[:ids.size]
        re = lambda segs: [dict(s, id=int(table[s["id"]])) for s in segs]    # noqa: E731
        args = (table[gt], re(gs), pred, ps) if which == 0 else (gt, gs, table[pred], re(ps))
        r2 = counts(PQ.pq_image_numpy(*(args + (PI.CATEGORIES,))))
        assert {c: (v[0], v[1], v[2], sorted(v[3])) for c, v in r2.items()} == {c: (v[0], v[1], v[2], sorted(v[3])) for c, v in r.items()}


def test_eval_sums_images_in_sorted_order_and_skips_empty_categories():
    ev, rev = PQ.PanopticEval(PI.CATEGORIES, device=False), PQ.PanopticEval(list(PI.CATEGORIES.values()), device=False)
    scenes = {k: PI.random_scene(k) for k in range(6)}
    for k in range(6):
        ev.add(k, *scenes[k])
    for k in reversed(range(6)):
        rev.add(k, *scenes[k])
    out = ev.summarize()
    assert out == rev.summarize()
    for c, s in out["per_class"].items():
        tp, fp, fn, iou = 0, 0, 0, 0.0
        for k in range(6):
            b = brute_force(*scenes[k])[c]
            tp, fp, fn = tp + b[0], fp + b[1], fn + b[2]
            for i, u in b[3]:
                iou += i / u
        assert (s["tp"], s["fp"], s["fn"]) == (tp, fp, fn)
        if tp + fp + fn:
            assert s["pq"] == iou / (tp + 0.5 * fp + 0.5 * fn) and s["rq"] == tp / (tp + 0.5 * fp + 0.5 * fn)
            assert s["sq"] == (iou / tp if tp else 0.0)
    only = PQ.PanopticEval(dict(list(PI.CATEGORIES.items()) + [(9, {"id": 9, "isthing": 0})]), device=False)
    only.add(0, *scenes[0])
    assert only.summarize()["per_class"][9] == {"pq": 0.0, "sq": 0.0, "rq": 0.0, "tp": 0, "fp": 0, "fn": 0}
    assert only.summarize()["All"]["n"] <= 3 and only.summarize()["Things"]["n"] + only.summarize()["Stuff"]["n"] == only.summarize()["All"]["n"]
    assert len(ev.lines()) == 5


# ---- the tools ----

def test_eval_panoptic_reads_what_save_panoptic_writes(tmp_path):
    import demo
    import eval_panoptic
    pm, Hh, Ww = LI.sets()["equal"]
    pm = pm.take(np.arange(len(pm)))
    pm.classes[:] = np.arange(len(pm)) % 20 + 1
    entry = demo._save_panoptic(str(tmp_path), "im", (Hh, Ww, 3), pm, cpu=True)
    cats = [{"id": k + 1, "name": "c%d" % k, "isthing": 1} for k in range(20)]
    path = str(tmp_path / "panoptic.json")
    with open(path, "w") as f:
        json.dump({"annotations": [entry], "categories": cats}, f)
    ev = eval_panoptic.evaluate(path, str(tmp_path), path, str(tmp_path), cpu=True)
    out = ev.summarize()
    assert out["All"]["pq"] == out["All"]["sq"] == out["All"]["rq"] == 1.0 and out["All"]["n"] == len({s["category_id"] for s in entry["segments_info"]})
    out_file = str(tmp_path / "pq.json")
    assert eval_panoptic.main(["--gt-json", path, "--gt-dir", str(tmp_path), "--dt-json", path, "--dt-dir", str(tmp_path), "--cpu",
                               "--out", out_file]) == 0
    assert json.load(open(out_file))["All"]["pq"] == 1.0


def test_sbd_to_panoptic_writes_ground_truth_the_evaluator_reads(tmp_path):
    import scipy.io as sio
    import eval_panoptic
    import sbd_to_panoptic
    inst, cls = LI.class_maps()
    for sub, key, arr in (("inst", "GTinst", inst), ("cls", "GTcls", cls)):
        os.makedirs(str(tmp_path / "devkit" / sub))
        sio.savemat(str(tmp_path / "devkit" / sub / "im0.mat"), {key: {"Segmentation": arr.astype(np.uint8)}})
    with open(str(tmp_path / "set.txt"), "w") as f:
        f.write("im0\n")
    out = str(tmp_path / "pan")
    assert sbd_to_panoptic.main(["--devkit", str(tmp_path / "devkit"), "--image-set", str(tmp_path / "set.txt"), "--out", out, "--cpu"]) == 0
    maps, cats = eval_panoptic.read_panoptic(os.path.join(out, "panoptic.json"), out)
    seg, info = maps["im0"]
    assert np.array_equal(seg, inst) and len(cats) == 20 and all(c["isthing"] == 1 for c in cats)
    assert [s["id"] for s in info] == [int(i) for i in np.unique(inst)[1:]]
    assert [s["category_id"] for s in info] == [int(cls[inst == s["id"]][0]) for s in info]
    assert [s["area"] for s in info] == [int((inst == s["id"]).sum()) for s in info]
    ev = eval_panoptic.evaluate(os.path.join(out, "panoptic.json"), out, os.path.join(out, "panoptic.json"), out, cpu=True)
    assert ev.summarize()["All"]["pq"] == 1.0
