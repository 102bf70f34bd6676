"""Panoptic quality of COCO panoptic results on the pair table of mnc_amd/pairs.py (csrc/label_pairs.hip): what scores the PNGs and
the panoptic.json that tools/demo.py --save-panoptic writes.

    pq_image(gt_map, gt_segments, pred_map, pred_segments, categories, device=True)  -> {category: {"tp", "fp", "fn", "matches"}}
    pq_image_numpy(...)                                                              the same with label_pairs_numpy
    PanopticEval(categories, device=True).add(...) / .summarize() / .lines()         PQ, SQ, RQ over a set of images

The rule is that of the published panopticapi's pq_compute_single_core, with VOID = 0, restated:

    maps       gt_map and pred_map are the segment ids of one image (labels.rgb_to_id of the PNGs), integer [H, W] of one shape;
               gt_segments and pred_segments are their segments_info lists ({"id", "category_id", "iscrowd"}; pred has no crowd).
    sanity     a pred id in the map (other than VOID) that is not in pred_segments, a pred id in pred_segments that is not in
               the map, and a pred category_id that is not in categories each raise KeyError.
    matching   over the pairs (g, p) of the table of (gt_map, pred_map), in the table's order: both ids are segments, g is not
               crowd, the categories are equal, and
                   2 * inter > area(p) + area(g) - inter - pairs.get(VOID, p)        (IoU strictly above 1/2, in integers)
               with union the right-hand side.  Such a pair is a true positive of the category; above 1/2 a match is unique.
    leftovers  a gt segment that is not matched and not crowd is a false negative.  A pred segment that is not matched is a false
               positive, unless 2 * (pairs.get(VOID, p) + pairs.get(c, p)) > area(p), with c the crowd segment of its category --
               the LAST such segment of gt_segments, as the published code keeps it.
    numbers    per category PQ = sum IoU / (tp + fp / 2 + fn / 2), SQ = sum IoU / tp (0 without a tp), RQ = tp / (tp + fp / 2 +
               fn / 2); categories without any tp, fp or fn are left out of the means over all, things and stuff.

One difference: areas are the counted row and column sums of the table, not the JSON's "area" fields.  A file whose areas are right
scores the same.

The IoU sum is taken on the host as float64 inter / union in pair order and image order (images by sorted id), whichever side
counted the pairs: the device and the numpy forms agree bit for bit."""
import numpy as np

from . import pairs as PR

VOID = 0


def _categories(categories):
    """{id: {"isthing": 0 / 1, ...}} from that dict, or from COCO's list of {"id", "isthing"} entries."""
    if isinstance(categories, dict):
        return {int(k): v for k, v in categories.items()}
    return {int(c["id"]): c for c in categories}


def _pq_from_pairs(t, gt_segments, pred_segments, categories):
    cats = _categories(categories)
    gt = {}
    for s in gt_segments:
        gt[int(s["id"])] = s
    pred = {}
    for s in pred_segments:
        pred[int(s["id"])] = s
    gt_area = dict(zip((int(v) for v in t.a_ids), (int(v) for v in t.a_areas)))
    pred_area = dict(zip((int(v) for v in t.b_ids), (int(v) for v in t.b_areas)))
    unseen = set(pred)
    for p in pred_area:
        if p not in pred:
            if p == VOID:
                continue
            raise KeyError("pq_image: segment %d is in the predicted map and not in its segments_info" % p)
        unseen.discard(p)
        if int(pred[p]["category_id"]) not in cats:
            raise KeyError("pq_image: segment %d has the unknown category %d" % (p, int(pred[p]["category_id"])))
    if unseen:
        raise KeyError("pq_image: segments %s are in the predicted segments_info and not in the map" % sorted(unseen))
    inter = {}
    for k in range(len(t)):
        inter[(int(t.a_ids[t.ia[k]]), int(t.b_ids[t.ib[k]]))] = int(t.count[k])
    out = {c: {"tp": 0, "fp": 0, "fn": 0, "matches": []} for c in cats}

    def stat(c):
        return out.setdefault(c, {"tp": 0, "fp": 0, "fn": 0, "matches": []})

    gt_matched, pred_matched = set(), set()
    for (g, p), n in inter.items():
        if g not in gt or p not in pred or int(gt[g].get("iscrowd", 0)) == 1:
            continue
        c = int(gt[g]["category_id"])
        if c != int(pred[p]["category_id"]):
            continue
        union = pred_area[p] + gt_area[g] - n - inter.get((VOID, p), 0)
        if 2 * n > union:
            stat(c)["tp"] += 1
            stat(c)["matches"].append((n, union))
            gt_matched.add(g)
            pred_matched.add(p)
    crowd = {}
    for g, s in gt.items():
        if g in gt_matched:
            continue
        if int(s.get("iscrowd", 0)) == 1:
            crowd[int(s["category_id"])] = g
            continue
        stat(int(s["category_id"]))["fn"] += 1
    for p, s in pred.items():
        if p in pred_matched:
            continue
        c = int(s["category_id"])
        covered = inter.get((VOID, p), 0)
        if c in crowd:
            covered += inter.get((crowd[c], p), 0)
        if 2 * covered > pred_area[p]:
            continue
        stat(c)["fp"] += 1
    return out


def pq_image_numpy(gt_map, gt_segments, pred_map, pred_segments, categories):
    """The rule of the module's docstring as the plain loop over the pair table of label_pairs_numpy -- the statement.
    -> {category id: {"tp", "fp", "fn", "matches": [(inter, union), ...] in pair order}} with every category of `categories`."""
    return _pq_from_pairs(PR.label_pairs_numpy(gt_map, pred_map), gt_segments, pred_segments, categories)


def pq_image(gt_map, gt_segments, pred_map, pred_segments, categories, device=True, device_id=None):
    """pq_image_numpy with the pairs counted on the GPU (pairs.label_pairs); device=False is pq_image_numpy and never touches it."""
    if not device:
        return pq_image_numpy(gt_map, gt_segments, pred_map, pred_segments, categories)
    return _pq_from_pairs(PR.label_pairs(gt_map, pred_map, device_id), gt_segments, pred_segments, categories)


class PanopticEval(object):
    """Panoptic quality over the images added, in the shape of coco_eval.CocoSegmEval.  categories: {id: {"isthing": 0 / 1}} or
    COCO's list.  device=True counts the pairs on the GPU, device=False with label_pairs_numpy, never touching it; the numbers are
    the same bits either way."""

    def __init__(self, categories, device=True):
        self.categories, self.device = _categories(categories), bool(device)
        self._images = {}
        self.stats = None

    def add(self, image_id, gt_map, gt_segments, pred_map, pred_segments):
        """Score one image and keep its counts -> what pq_image returns."""
        if image_id in self._images:
            raise ValueError("PanopticEval.add: image %r was added before" % (image_id,))
        r = pq_image(gt_map, gt_segments, pred_map, pred_segments, self.categories, self.device)
        self._images[image_id] = r
        self.stats = None
        return r

    def summarize(self):
        """-> {"All" / "Things" / "Stuff": {"pq", "sq", "rq", "n"}, "per_class": {id: {"pq", "sq", "rq", "tp", "fp", "fn"}}}.
        Images in the order of their sorted ids; a group without a category that has a tp, fp or fn gives 0.0 with n = 0."""
        try:
            ids = sorted(self._images)
        except TypeError:
            ids = list(self._images)
        per = {}
        for c in self.categories:
            tp = fp = fn = 0
            iou = 0.0
            for i in ids:
                s = self._images[i].get(c)
                if s is None:
                    continue
                tp, fp, fn = tp + s["tp"], fp + s["fp"], fn + s["fn"]
                for n, u in s["matches"]:
                    iou += np.float64(n) / np.float64(u)
            if tp + fp + fn == 0:
                per[c] = {"pq": 0.0, "sq": 0.0, "rq": 0.0, "tp": 0, "fp": 0, "fn": 0}
                continue
            den = tp + 0.5 * fp + 0.5 * fn
            per[c] = {"pq": float(iou / den), "sq": float(iou / tp) if tp else 0.0, "rq": float(tp / den), "tp": tp, "fp": fp, "fn": fn}
        out = {"per_class": per}
        for name, want in (("All", None), ("Things", 1), ("Stuff", 0)):
            cs = [c for c in self.categories if per[c]["tp"] + per[c]["fp"] + per[c]["fn"] > 0
                  and (want is None or int(self.categories[c].get("isthing", 1)) == want)]
            out[name] = {k: (float(sum(per[c][k] for c in cs) / len(cs)) if cs else 0.0) for k in ("pq", "sq", "rq")}
            out[name]["n"] = len(cs)
        self.stats = out
        return out

    def lines(self):
        """The table the published evaluator prints."""
        s = self.stats or self.summarize()
        rows = ["%-10s| %5s  %5s  %5s %5s" % ("", "PQ", "SQ", "RQ", "N"), "-" * 38]
        for name in ("All", "Things", "Stuff"):
            rows.append("%-10s| %5.1f  %5.1f  %5.1f %5d" % (name, 100 * s[name]["pq"], 100 * s[name]["sq"], 100 * s[name]["rq"], s[name]["n"]))
        return rows
