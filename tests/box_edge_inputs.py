"""Inputs that sit ON the decision rules of the box side of the result tail, and the plain statement of every rule.

Seeded random floats never land on a threshold, so `>` against `>=`, round-half-away against round-half-even, or a threshold
compared in float32 against float64 all pass a random test.  The corpora here are built so that each rule decides:

  1. NMS (nms_kernel.cu:24-32, 66-71): pairs of integer boxes whose float32 IoU is the float below, on and above 0.3f / 0.7f
     (0.5f: on only), placed at chosen sorted positions of box sets of 2..129 boxes.
  2. bbox_overlaps / voting membership (bbox.pyx:15-55, mask_transform.py:259-262): integer pairs at IoU exactly 1/2 and at the
     rationals next to it, one-pixel overlaps, and voting sets whose member M sits at IoU exactly 1/2 with the kept box.
  3. Binarisation (mv_kernel.cu:13, :121, :136; mask_transform.py:122, :125; vis_seg.py:115 / voc_eval.py:247): masks constant at the
     float below, on and above 0.4f.
  4. ROIPooling: roi edges that scale to k + 0.5, -0.5 and 0.49999997, sides whose float32 bin edge is / is not the exact one.

The statements are numpy written from the reference lines they cite, not calls into the oracle; every one takes the variations
(`mutants`) that tests/test_box_edges_host.py shows the corpus to tell apart.  tests/test_gpu_box_edges.py runs the library
entries on the same inputs.  Every comparison is exact."""
from fractions import Fraction

import numpy as np

F32 = np.float32


def f32_below(x):
    return np.nextafter(F32(x), F32(-np.inf))


def f32_above(x):
    return np.nextafter(F32(x), F32(np.inf))


# =====================================================================================================================
# 1. NMS at 0.3 / 0.5 / 0.7 in float32
# =====================================================================================================================
def search_nms_pairs(target, count, seed=0, lo=600, hi=1400, side_max=2040, grow=48):
    """Pairs of integer boxes whose IoU, computed as devIoU does (float32(inter) / float32(union), every other operation exact
    because all integers stay below 2^24), is exactly the float32 `target`.

    Directed: pick the overlap ow x oh, I = ow * oh; the integers U with float32(I) / float32(U) == target lie in a window
    of width about I * ulp(target) / target^2 around I / target, so there are O(1) of them (often none); the first box is
    (ow + a) x (oh + c) with the overlap in its bottom-right corner, and U + I - Sa must factor into a second box
    (ow + b) x (oh + d) that has the overlap in its top-left corner.  -> [((x1, y1, x2, y2), (x1, y1, x2, y2)), ...]
    This is how NMS_PAIRS below was made; the tests read the table and do not search."""
    target = F32(target)
    rng = np.random.default_rng(seed)
    found, seen = [], set()
    a = np.arange(1, grow + 1, dtype=np.int64)
    while len(found) < count:
        ow, oh = (int(v) for v in rng.integers(lo, hi + 1, 2))
        I = ow * oh
        centre = int(round(I / float(target)))
        U = np.arange(centre - 4, centre + 5, dtype=np.int64)
        U = U[(F32(I) / U.astype(np.float32)) == target]
        for u in U:
            total = int(u) + I                                           # Sa + Sb
            if total >= 1 << 24:
                continue
            Sa = (ow + a)[:, None] * (oh + a)[None, :]                    # [a][c]
            Sb = total - Sa
            wb = np.arange(ow + 1, side_max + 1, dtype=np.int64)
            hb = Sb[:, :, None] // wb[None, None, :]
            ok = (hb * wb[None, None, :] == Sb[:, :, None]) & (hb > oh) & (hb <= side_max)
            hit = np.argwhere(ok)
            if not len(hit):
                continue
            ia, ic, ib = (int(v) for v in hit[rng.integers(len(hit))])
            wa, ha, w2, h2 = ow + int(a[ia]), oh + int(a[ic]), int(wb[ib]), int(hb[ia, ic, ib])
            if wa > side_max or ha > side_max or (ow, oh) in seen:
                continue
            seen.add((ow, oh))
            found.append(((0, 0, wa - 1, ha - 1), (wa - ow, ha - oh, wa - ow + w2 - 1, ha - oh + h2 - 1)))
            break
    return found[:count]


NMS_THRESHOLDS = (0.3, 0.5, 0.7)


def nms_class_float(t, cls):
    """The float32 IoU of class `cls` ("below" / "on" / "above") at threshold t."""
    t32 = F32(t)
    return {"below": np.nextafter(t32, F32(0)), "on": t32, "above": np.nextafter(t32, F32(1))}[cls]


# search_nms_pairs(nms_class_float(t, cls), 8, seed=3 * int(10 * t) + len(cls)), each class well under a second.  0.5 has the
# on-threshold class alone: 0.5f needs U == 2 * I, and its neighbours need an overlap of more than 2^24 pixels.
NMS_PAIRS = {
    (0.3, "below"): (
        ((0, 0, 901, 1330), (24, 43, 1872, 2043)),
        ((0, 0, 1218, 1078), (15, 39, 2036, 2071)),
        ((0, 0, 819, 1316), (24, 46, 1810, 1894)),
        ((0, 0, 841, 1282), (45, 31, 2065, 1635)),
        ((0, 0, 1035, 1046), (48, 31, 1794, 1899)),
        ((0, 0, 898, 1297), (30, 1, 1961, 1924)),
        ((0, 0, 1132, 931), (25, 9, 1691, 2033)),
        ((0, 0, 836, 1232), (22, 35, 1739, 1896)),
    ),
    (0.3, "on"): (
        ((0, 0, 745, 704), (39, 3, 1945, 854)),
        ((0, 0, 1028, 1091), (30, 20, 2033, 1774)),
        ((0, 0, 1194, 630), (25, 9, 1939, 1261)),
        ((0, 0, 763, 926), (46, 6, 1292, 1735)),
        ((0, 0, 1063, 703), (26, 48, 1311, 1759)),
        ((0, 0, 1264, 805), (34, 8, 1864, 1775)),
        ((0, 0, 724, 789), (17, 27, 1893, 968)),
        ((0, 0, 909, 1364), (28, 22, 1938, 2057)),
    ),
    (0.3, "above"): (
        ((0, 0, 1126, 933), (4, 45, 2035, 1655)),
        ((0, 0, 1074, 700), (36, 43, 1451, 1602)),
        ((0, 0, 1294, 966), (42, 48, 2044, 1913)),
        ((0, 0, 1378, 698), (37, 5, 1670, 1884)),
        ((0, 0, 1046, 772), (7, 42, 1283, 1987)),
        ((0, 0, 1293, 982), (35, 22, 1993, 2048)),
        ((0, 0, 710, 1297), (5, 43, 1777, 1687)),
        ((0, 0, 1295, 700), (20, 28, 2004, 1444)),
    ),
    (0.7, "below"): (
        ((0, 0, 1233, 1266), (24, 16, 1680, 1290)),
        ((0, 0, 1070, 1398), (32, 45, 1421, 1424)),
        ((0, 0, 1357, 1038), (38, 34, 1586, 1202)),
        ((0, 0, 912, 981), (43, 1, 1071, 1143)),
        ((0, 0, 1230, 816), (32, 25, 1615, 845)),
        ((0, 0, 1368, 818), (8, 39, 1719, 889)),
        ((0, 0, 1403, 1249), (9, 16, 1509, 1631)),
        ((0, 0, 1124, 1344), (48, 33, 1332, 1525)),
    ),
    (0.7, "on"): (
        ((0, 0, 649, 1172), (22, 18, 674, 1547)),
        ((0, 0, 1119, 815), (7, 5, 1213, 1063)),
        ((0, 0, 1089, 716), (5, 26, 1295, 830)),
        ((0, 0, 1162, 1156), (40, 30, 1427, 1274)),
        ((0, 0, 720, 1217), (35, 45, 769, 1508)),
        ((0, 0, 672, 797), (22, 48, 737, 953)),
        ((0, 0, 832, 1135), (14, 12, 1145, 1150)),
        ((0, 0, 1326, 696), (46, 9, 1394, 909)),
    ),
    (0.7, "above"): (
        ((0, 0, 1316, 1005), (27, 13, 1821, 1007)),
        ((0, 0, 1020, 1232), (16, 5, 1271, 1388)),
        ((0, 0, 1015, 1203), (7, 44, 1315, 1280)),
        ((0, 0, 1092, 1052), (45, 16, 1412, 1103)),
        ((0, 0, 1035, 1312), (1, 44, 1166, 1612)),
        ((0, 0, 1314, 1406), (47, 30, 1773, 1413)),
        ((0, 0, 1278, 918), (7, 22, 1418, 1151)),
        ((0, 0, 1166, 1085), (39, 31, 1483, 1153)),
    ),
    (0.5, "on"): (
        ((0, 0, 1198, 1295), (6, 20, 1655, 1845)),
        ((0, 0, 755, 971), (28, 6, 1050, 1349)),
        ((0, 0, 1211, 934), (2, 41, 1376, 1576)),
        ((0, 0, 789, 1009), (18, 45, 798, 1884)),
        ((0, 0, 1363, 949), (31, 8, 1456, 1740)),
        ((0, 0, 1126, 701), (38, 30, 1523, 974)),
        ((0, 0, 669, 639), (30, 28, 909, 875)),
        ((0, 0, 832, 896), (30, 4, 1577, 910)),
    ),
}


def pair_integers(a, b):
    """(inter, union, Sa, Sb) of two integer boxes in Python integers, +1 widths, each side of the intersection clamped at 0."""
    iw = max(min(a[2], b[2]) - max(a[0], b[0]) + 1, 0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]) + 1, 0)
    Sa, Sb = (a[2] - a[0] + 1) * (a[3] - a[1] + 1), (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
    return iw * ih, Sa + Sb - iw * ih, Sa, Sb


def fraction_to_f32(q):
    """A positive Fraction rounded to the nearest float32, ties to even, in integers alone."""
    e = 0
    while q >= 1 << 24:
        q, e = q / 2, e + 1
    while q < 1 << 23:
        q, e = q * 2, e - 1
    m, rest = divmod(q.numerator, q.denominator)
    twice = Fraction(2 * rest, q.denominator)
    if twice > 1 or (twice == 1 and m & 1):
        m += 1
    return F32(np.ldexp(np.float64(m), e))


# Sorted positions (i, j) of a pair: both ends of a 64-box tile, the diagonal tile's `j > i` rule, a tile apart and two apart.
NMS_POSITIONS = ((0, 1), (0, 63), (62, 63), (63, 64), (0, 64), (63, 127), (64, 128), (127, 128))
NMS_SIZES = (2, 64, 65, 128, 129)
FILLER_GRID = 4096


def place_pair(pair, i, j, n):
    """[n, 5] float32 in descending score order with the pair at positions i < j.  The pair keeps its place near the origin
    (translated by an integer: its IoU stays bit-identical); position p of the rest is a 10 x 10 box at x = 4096 * (p + 2),
    disjoint from everything, all coordinates below 2^24.  Scores are distinct and descend with the position."""
    assert 0 <= i < j < n
    out = np.zeros((n, 5), np.float32)
    p = np.arange(n)
    out[:, 0] = FILLER_GRID * (p + 2)
    out[:, 1] = 7
    out[:, 2] = out[:, 0] + 9
    out[:, 3] = 16
    out[:, 4] = 1.0 - p / 256.0
    shift = np.array([3 + i, 5 + j, 3 + i, 5 + j], np.float32)
    out[i, :4] = np.array(pair[0], np.float32) + shift
    out[j, :4] = np.array(pair[1], np.float32) + shift
    assert out[:, :4].max() < 2 ** 24
    return out


def nms_placements():
    """(t, cls, pair number, i, j, n) of every placement the tests run: each position at the smallest size that holds it and at
    the next size up, the pairs of a class taken in turn."""
    out = []
    for t in NMS_THRESHOLDS:
        for cls in ("below", "on", "above"):
            if (t, cls) not in NMS_PAIRS:
                continue
            k = 0
            for (i, j) in NMS_POSITIONS:
                sizes = [n for n in NMS_SIZES if n > j][:2]
                for n in sizes:
                    out.append((t, cls, k % len(NMS_PAIRS[(t, cls)]), i, j, n))
                    k += 1
    return out


def iou32(a, b):
    """devIoU, nms_kernel.cu:24-32, in numpy float32 operation by operation; a [4], b [m, 4]."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    one, zero = F32(1), F32(0)
    left, right = np.maximum(a[0], b[:, 0]), np.minimum(a[2], b[:, 2])
    top, bottom = np.maximum(a[1], b[:, 1]), np.minimum(a[3], b[:, 3])
    width, height = np.maximum(right - left + one, zero), np.maximum(bottom - top + one, zero)
    inter = width * height
    Sa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    Sb = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    return inter, Sa + Sb - inter


def nms_statement(boxes, thr, mutant=None, max_keep=None):
    """nms_kernel.cu:66-71 and :124-140 on boxes already in score order: bit j of row i is set iff IoU(i, j) > thr (and j > i),
    strict, in float32 after a correctly rounded division; the scan keeps a row whose bit is clear and ORs its row in.
    -> (bits bool [n, n], keep list).  mutants: "ge" (>=), "mul" (inter > thr * union, no division)."""
    boxes = np.asarray(boxes, F32)[:, :4]
    n, thr = len(boxes), F32(thr)
    bits = np.zeros((n, n), bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            inter, union = iou32(boxes[i], boxes)
            hit = {None: lambda: inter / union > thr, "ge": lambda: inter / union >= thr, "mul": lambda: inter > thr * union}[mutant]()
            bits[i] = hit
            bits[i, i // 64 * 64:i + 1] = False          # :66-69: inside the diagonal tile only j > i (other tiles are whole)
    gone, keep = np.zeros(n, bool), []
    for i in range(n):
        if not gone[i] and (max_keep is None or len(keep) < max_keep):
            keep.append(i)
            gone |= bits[i]
    return bits, keep


def mask_words(bits):
    """bool [n, n] -> the uint64 words [n, ceil(n / 64)] of mnc_nms_mask / orc_nms_mask."""
    n = len(bits)
    cb = (n + 63) // 64
    pad = np.zeros((n, cb * 64), np.uint8)
    pad[:, :n] = bits
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint64).reshape(n, cb)


def degenerate_cases():
    """(name, boxes [n, 5] in score order, thr, keep the reference's rule gives).  Finite coordinates only."""
    def dets(*rows):
        return np.array([list(r) + [1.0 - 0.1 * k] for k, r in enumerate(rows)], np.float32)
    box = (10, 20, 49, 79)
    return [
        ("identical at 1.0", dets(box, box), 1.0, [0, 1]),                    # 1.0 > 1.0 is false
        ("identical at 0.7", dets(box, box), 0.7, [0]),
        ("one shared column at 0.0", dets(box, (49, 30, 90, 60)), 0.0, [0]),  # inter 31 > 0
        ("one shared row at 0.0", dets(box, (20, 79, 30, 99)), 0.0, [0]),
        ("one shared pixel at 0.0", dets(box, (49, 79, 60, 90)), 0.0, [0]),
        ("one pixel apart at 0.0", dets(box, (50, 20, 90, 79)), 0.0, [0, 1]),  # 0 > 0 is false
        ("disjoint at 0.0", dets(box, (200, 200, 240, 260)), 0.0, [0, 1]),
        ("zero width twice", dets((30, 20, 29, 79), (30, 20, 29, 79)), 0.3, [0, 1]),   # 0 / 0 is NaN, NaN > thr is false
        # negative area: inter 0, union 2400 - 80 * 60 + ... whatever float32 gives; the statement decides
        ("inverted against ordinary", dets(box, (40, 20, 20, 79)), 0.3, None),
        ("ordinary against inverted", dets((40, 20, 20, 79), box, (41, 20, 19, 79)), 0.3, None),
        # union 9 - 1140 < 0: 0 / union is -0, not > 0.3, both kept -- whereas 0 > 0.3 * union holds
        ("small against inverted", dets((10, 20, 12, 22), (40, 20, 20, 79)), 0.3, [0, 1]),
    ]


# =====================================================================================================================
# 2. bbox_overlaps and the voting membership at 1/2 in float64
# =====================================================================================================================
def search_near_half(sign, lo=2030, hi=2047):
    """The pair of integer boxes with sides below 2048 whose IoU I / (2 * I + sign) is closest to 1/2: below it for sign = +1,
    above it for sign = -1.  Sa + Sb = 3 * I + sign; every pair with a side under `lo` has a smaller Sa + Sb than the one found,
    so the window is exhaustive.  This is how NEAR_HALF below was made."""
    import itertools
    best = None
    r = range(lo, hi + 1)
    for wa, ha, wb, hb in itertools.product(r, r, r, r):
        T = wa * ha + wb * hb
        if (T - sign) % 3:
            continue
        I = (T - sign) // 3
        if best is not None and I <= best[0]:
            continue
        ow = np.arange(1, min(wa, wb) + 1, dtype=np.int64)
        oh = I // ow
        ok = (oh * ow == I) & (oh <= min(ha, hb))
        if ok.any():
            k = int(ow[ok][-1])
            best = (I, ((0, 0, wa - 1, ha - 1), (wa - k, ha - I // k, wa - k + wb - 1, ha - I // k + hb - 1)))
    assert best is not None and 3 * best[0] + sign > (lo - 1) * hi + hi * hi
    return best[1]


NEAR_HALF = {"below": ((0, 0, 2045, 2046), (0, 682, 2046, 2728)),        # 2792790 / 5585581
             "above": ((0, 0, 2044, 2046), (123, 595, 2168, 2640))}      # 2790744 / 5581487
HALF_PAIRS = NMS_PAIRS[(0.5, "on")] + (((10, 10, 39, 39), (20, 10, 49, 39)), ((0, 0, 2, 1), (1, 0, 3, 1)),
                                       ((5, 5, 5, 6), (5, 6, 5, 6)))
# (pair, inter): one shared pixel row, one column, one pixel; one pixel apart in x, in y, diagonally
TOUCHING_PAIRS = ((((10, 20, 49, 79), (20, 79, 30, 99)), 11), (((10, 20, 49, 79), (49, 30, 90, 60)), 31),
                  (((10, 20, 49, 79), (49, 79, 60, 90)), 1), (((10, 20, 49, 79), (50, 20, 90, 79)), 0),
                  (((10, 20, 49, 79), (10, 80, 49, 99)), 0), (((10, 20, 49, 79), (50, 80, 60, 90)), 0))


def overlaps_statement(boxes, query):
    """bbox.pyx:15-55 in numpy float64: +1 widths, an entry stays 0 unless iw > 0 and ih > 0."""
    b, q = np.asarray(boxes, np.float64), np.asarray(query, np.float64)
    out = np.zeros((len(b), len(q)))
    for k in range(len(q)):
        qarea = (q[k, 2] - q[k, 0] + 1) * (q[k, 3] - q[k, 1] + 1)
        iw = np.minimum(b[:, 2], q[k, 2]) - np.maximum(b[:, 0], q[k, 0]) + 1
        ih = np.minimum(b[:, 3], q[k, 3]) - np.maximum(b[:, 1], q[k, 1]) + 1
        ua = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1) + qarea - iw * ih
        ok = (iw > 0) & (ih > 0)
        out[ok, k] = (iw * ih)[ok] / ua[ok]
    return out


def members_statement(boxes, kept, mutant=None):
    """mask_transform.py:259-262: the indices with IoU >= 0.5, non-strict, in float64.  mutants: "gt" (>), "f32thr" (the
    threshold taken as float32(0.5000001) widened)."""
    ov = overlaps_statement(boxes, np.asarray(kept, np.float64)[None])[:, 0]
    if mutant == "gt":
        return np.where(ov > 0.5)[0]
    if mutant == "f32thr":
        return np.where(ov >= np.float64(F32(0.5000001)))[0]
    return np.where(ov >= 0.5)[0]


VOTE_W, VOTE_H, VOTE_S = 101, 77, 21
VOTE_K = (10, 10, 39, 39)                                    # 30 x 30
VOTE_M = (20, 10, 49, 39)                                    # 600 / 1200 with K
_E = 2.0 ** -16
VOTE_L = (20 + _E, 10, 49 + _E, 39)                          # (600 - 30 e) / (1200 + 30 e)
VOTE_J = (20 - _E, 10, 49 - _E, 39)                          # (600 + 30 e) / (1200 - 30 e)
VOTING_SETS = ((3, 1), (66, 63), (66, 64), (130, 129), (130, 64))     # (n, index of M)


def voting_set(n, m_index):
    """One crafted voting problem, two foreground classes.  Index 0 is K, the top score of class 1; M (IoU exactly 1/2 with K)
    sits at m_index; L (just below 1/2) and, from n = 66 on, J (just above) take the first free indices; the rest are 21 x 21
    boxes beyond the canvas, disjoint from everything.  K's mask is 0.9 on its left third and 0.1 elsewhere, M's and L's are
    1.0, J's is 0: with M a member the voted box of K reaches x = 49, without it x = 19.  In class 2 M has the top score and K
    is the member at 1/2."""
    S = VOTE_S
    boxes = np.zeros((n, 4), np.float32)
    masks = np.zeros((n, 1, S, S), np.float32)
    scores = np.zeros((n, 3), np.float32)
    free = [i for i in range(1, n) if i != m_index]
    idx = {"K": 0, "M": m_index, "L": free[0]}
    if n >= 66:
        idx["J"] = free[1]
    special = set(idx.values())
    k = 0
    for i in range(n):
        if i in special:
            continue
        boxes[i] = (1000 + 50 * k, 1000, 1020 + 50 * k, 1020)
        masks[i] = 0.25 + (k % 8) / 16.0
        scores[i] = (0.5, 0.04 - k / 4096.0, 0.01 + k / 4096.0)
        k += 1
    for name, box, mask, s1, s2 in (("K", VOTE_K, None, 0.9, 0.85), ("M", VOTE_M, 1.0, 0.85, 0.9), ("L", VOTE_L, 1.0, 0.8, 0.3),
                                    ("J", VOTE_J, 0.0, 0.05, 0.2)):
        if name not in idx:
            continue
        i = idx[name]
        boxes[i] = box
        if mask is None:
            masks[i, 0] = 0.1
            masks[i, 0, :, :7] = 0.9
        else:
            masks[i] = mask
        scores[i] = (0.1, s1, s2)
    assert np.array_equal(boxes[idx["L"]].astype(np.float64), np.array(VOTE_L))      # the shifted edges are float32 values
    return {"boxes": boxes, "masks": masks, "scores": scores, "idx": idx, "n": n, "H": VOTE_H, "W": VOTE_W, "num_classes": 3,
            "max_per_image": 100}


# =====================================================================================================================
# 3. Binarisation at 0.4f
# =====================================================================================================================
BIN = 0.4                                                     # cfg.BINARIZE_THRESH; mv_kernel.cu:13 holds it as a float
BIN_LEVELS = (("below", f32_below(BIN)), ("on", F32(BIN)), ("above", f32_above(BIN)))
MV_W, MV_H = 101, 77                                          # odd: the centre fallback is (50, 38)
MV_X, MV_Y = 31, 17


def mv_case(mask, weights=(1.0,), x=MV_X, y=MV_Y, W=MV_W, H=MV_H):
    """mnc_mv arguments for one result whose len(weights) candidates share the box (x, y, x + 20, y + 20) and the 21 x 21 mask:
    rw = rh = 1, fx = fy = 0, so the render is the mask itself."""
    k = len(weights)
    mask = np.broadcast_to(np.asarray(mask, F32), (VOTE_S, VOTE_S))
    return {"boxes": np.tile(np.array([[x, y, x + 20, y + 20]], F32), (k, 1)), "masks": np.tile(mask[None, None], (k, 1, 1, 1)),
            "inds": np.arange(k, dtype=np.int32), "start": np.array([k], np.int32), "weights": np.array(weights, F32),
            "H": H, "W": W}


def mv_args(c):
    return c["boxes"], c["masks"], c["inds"], c["start"], c["weights"], c["H"], c["W"]


def mv_cases():
    """(name, case): the three constants with one candidate and with two of weight 1/2 (the same aggregate, exactly), and a mask
    at 0.4f except one pixel at the float above it, that pixel at each corner and in the middle."""
    out = []
    for name, v in BIN_LEVELS:
        out.append(("const %s" % name, mv_case(v)))
        out.append(("halves %s" % name, mv_case(v, (0.5, 0.5))))
    for py, px in ((0, 0), (0, 20), (20, 0), (20, 20), (10, 10)):
        m = np.full((VOTE_S, VOTE_S), F32(BIN), F32)
        m[py, px] = f32_above(BIN)
        out.append(("pixel %d %d" % (py, px), mv_case(m)))
    return out


def mv_box_statement(c, mutant=None):
    """The voted box of an mv_case: aggregate = ((0 + m * w0) + m * w1) ... in float32 (mv_kernel.cu:104-110), a pixel counts
    when aggregate > 0.4f, strict, against the float constant (:13, :121, :136); none: (W / 2, H / 2) twice (:149, :173).
    mutants: "ge" (>=), "f64" (the aggregate widened and compared with the double 0.4)."""
    agg = np.zeros((VOTE_S, VOTE_S), F32)
    for i, w in zip(c["inds"], c["weights"]):
        agg = agg + c["masks"][i, 0] * w
    on = {None: lambda: agg > F32(BIN), "ge": lambda: agg >= F32(BIN), "f64": lambda: agg.astype(np.float64) > BIN}[mutant]()
    if not on.any():
        return np.array([c["W"] // 2, c["H"] // 2, c["W"] // 2, c["H"] // 2], np.int32)
    ys, xs = np.where(on)
    x, y = int(c["boxes"][0, 0]), int(c["boxes"][0, 1])
    return np.array([x + xs.min(), y + ys.min(), x + xs.max(), y + ys.max()], np.int32)


def image_vote_case(level):
    """mnc_mask_voting_image arguments: one box (MV_X, MV_Y, +20, +20), one class, a constant mask.  The cv2 resize of a 21 x 21
    mask to a 21 x 21 box is the identity."""
    return {"boxes": np.array([[MV_X, MV_Y, MV_X + 20, MV_Y + 20]], F32), "masks": np.full((1, 1, VOTE_S, VOTE_S), level, F32),
            "scores": np.array([[0.1, 0.9]], F32), "H": MV_H, "W": MV_W}


def image_vote_statement(c, mutant=None):
    """cpu_mask_voting with one instance: mask_transform.py:122 binarises the float32 mask with `>= cfg.BINARIZE_THRESH`, a
    float32 comparison under the numpy the reference ran on; the canvas is 1.0 * binary in float64 and :125 takes `canvas >= 0.4`;
    none: the centre (:126-130).  -> (box int32 [4], mask float32 [S, S]): the canvas crop resized to S x S, a constant here.
    mutant: "gt"."""
    m = c["masks"][0, 0]
    binary = (m > F32(BIN)) if mutant == "gt" else (m >= F32(BIN))
    canvas = np.zeros((c["H"], c["W"]))
    canvas[MV_Y:MV_Y + 21, MV_X:MV_X + 21] += binary.astype(float) * np.float64(1.0)
    r, cc = np.where(canvas >= BIN)
    if len(r) == 0:
        box = np.array([c["W"] // 2, c["H"] // 2, c["W"] // 2, c["H"] // 2], np.int32)
    else:
        box = np.array([cc.min(), r.min(), cc.max(), r.max()], np.int32)
    crop = canvas[box[1]:box[3] + 1, box[0]:box[2] + 1].astype(F32)
    assert (crop == crop[0, 0]).all()                        # a constant resizes to itself
    return box, np.full((VOTE_S, VOTE_S), crop[0, 0], F32)


def instance_mask_case():
    """mnc_instance_masks inputs: three 21 x 21 integer boxes (the resize is the identity) with masks constant at the three
    levels, and a fourth whose mask is 0.4f except one pixel below it."""
    boxes = np.array([[5, 4, 25, 24], [30, 4, 50, 24], [55, 4, 75, 24], [5, 40, 25, 60]], np.float64)
    masks = np.stack([np.full((VOTE_S, VOTE_S), v, F32) for _, v in BIN_LEVELS] + [np.full((VOTE_S, VOTE_S), F32(BIN), F32)])
    masks[3, 6, 13] = f32_below(BIN)
    return boxes, masks, MV_H, MV_W


def instance_mask_statement(masks, mutant=None):
    """vis_seg.py:115 / voc_eval.py:247: `mask >= cfg.BINARIZE_THRESH` on a float32 array, i.e. against float32(0.4).
    mutant: "gt"."""
    return (masks > F32(BIN)) if mutant == "gt" else (masks >= F32(BIN))


# (score_thresh, scores float32, kept): the record's float32 score is widened and compared with the double (demo.py's
# `det[:, -1] >= thresh` on float64 boxes).  float32(0.3) lies above 0.3 and is kept; float32(0.7) lies below 0.7 and is dropped,
# which a float32 comparison would keep.
SCORE_CASES = ((0.3, (f32_below(0.3), F32(0.3), f32_above(0.3), F32(0.9)), (False, True, True, True)),
               (0.7, (f32_below(0.7), F32(0.7), f32_above(0.7), F32(0.9)), (False, False, True, True)))


def score_statement(scores, thresh, mutant=None):
    s = np.asarray(scores, F32)
    return (s >= F32(thresh)) if mutant == "f32" else (s.astype(np.float64) >= float(thresh))


# =====================================================================================================================
# 4. ROIPooling: rounding and bin edges
# =====================================================================================================================
ROI_SCALE = 0.0625
ROI_C, ROI_H, ROI_W = 8, 12, 12
ROI_P = (2, 7)
_B8 = float(np.nextafter(F32(8), F32(0)))                     # * 0.0625 = 0.49999997
# roi edge -> edge * scale: 8 -> 0.5, 24 -> 1.5, 40 -> 2.5, 56 -> 3.5, -8 -> -0.5
ROI_HALF_EDGES = (8.0, 24.0, 40.0, 56.0, -8.0, _B8)
ROI_SIDES = (7, 14, 15, 21, 22, 1, 2, 3, 5, 9, 11, 12)
# sides at which 7 * float32(side / 7) lands above the integer side, so that ceilf gives side + 1 (Caffe's own result)
ROI_LONG_SIDES = (57, 114, 121)


def roi_cases():
    """rois [R, 5]: every half edge as x1 and as y1 against far edges that are themselves halves (8.5 -> 9, 9.5 -> 10, 10.5 -> 11)
    or integers; then integer rois of every height and width of ROI_SIDES, at the origin and hanging over the top left."""
    rows = []
    for k, e in enumerate(ROI_HALF_EDGES):
        far = (136.0, 152.0, 168.0, 112.0, 176.0, 96.0)[k]
        rows.append((0, e, 16.0, far, 144.0))
        rows.append((0, 16.0, e, 160.0, far))
        rows.append((0, e, e, far, far))
    for e in ROI_HALF_EDGES:                                   # the half edge as the far edge
        rows.append((0, -32.0, 0.0, e, 120.0))
        rows.append((0, 0.0, -32.0, 120.0, e))
    for k, s in enumerate(ROI_SIDES):
        t = ROI_SIDES[(k + 5) % len(ROI_SIDES)]
        rows.append((0, 0.0, 0.0, 16.0 * (t - 1), 16.0 * (s - 1)))
        rows.append((0, -80.0, -160.0, -80.0 + 16.0 * (s - 1), -160.0 + 16.0 * (t - 1)))
    for s in ROI_LONG_SIDES:                                   # the far edge at 7, the last bin's end at 8 (exact) or 9 (float32)
        rows.append((0, 16.0, 16.0 * (8 - s), 112.0, 112.0))
        rows.append((0, 16.0 * (8 - s), 16.0, 112.0, 112.0))
    return np.array(rows, np.float32)


def roi_feature():
    """[1, C, H, W] of distinct integers, ascending along another diagonal in every channel: any bin error changes a maximum."""
    C, H, W = ROI_C, ROI_H, ROI_W
    y, x = np.mgrid[0:H, 0:W]
    feat = np.zeros((1, C, H, W), np.float32)
    for c in range(C):
        sy, sx = (1 if c & 1 else -1), (1 if c & 2 else -1)
        order = (sy * y * W + sx * x) if c & 4 else (sx * x * H + sy * y)
        feat[0, c] = order - order.min() + 1000 * c
    return feat


def round_half_away(x):
    """roundf on float32 values, written out: truncate, then step away from zero when the (exact) rest reaches one half."""
    x = np.asarray(x, F32)
    t = np.trunc(x)
    return (t + np.where(np.abs(x - t) >= F32(0.5), np.sign(x), F32(0))).astype(np.int64)


def roi_pool_statement(feat, rois, PH, PW, scale=ROI_SCALE, mutant=None):
    """Caffe's ROIPooling forward (Fast R-CNN roi_pooling_layer.cu) in numpy float32: corners round(roi * scale) half away from
    zero, sides max(x2 - x1 + 1, 1), bin = side / P in float32, edges floor(p * bin) and ceil((p + 1) * bin) moved by the corner
    and clipped to the map, the maximum of the bin, 0 for an empty one.  mutants: "rint" (half to even), "floor"
    (floor(x + 0.5) in float32), "exact" (bin edges from the exact rational p * side / P)."""
    feat, rois = np.asarray(feat, F32), np.asarray(rois, F32)
    N, C, H, W = feat.shape
    rnd = {None: round_half_away, "exact": round_half_away, "rint": lambda v: np.rint(v).astype(np.int64),
           "floor": lambda v: np.floor(v + F32(0.5)).astype(np.int64)}[mutant]
    out = np.zeros((len(rois), C, PH, PW), F32)
    if mutant == "exact":
        rnd = round_half_away
    for r, roi in enumerate(rois):
        x1, y1, x2, y2 = (int(v) for v in rnd(roi[1:5] * F32(scale)))
        rw, rh = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
        bh, bw = F32(rh) / F32(PH), F32(rw) / F32(PW)
        if mutant == "exact":
            bh, bw = Fraction(rh, PH), Fraction(rw, PW)
        for ph in range(PH):
            hs = min(max(int(np.floor(ph * bh if mutant == "exact" else F32(ph) * bh)) + y1, 0), H)
            he = min(max(int(np.ceil((ph + 1) * bh if mutant == "exact" else F32(ph + 1) * bh)) + y1, 0), H)
            for pw in range(PW):
                ws = min(max(int(np.floor(pw * bw if mutant == "exact" else F32(pw) * bw)) + x1, 0), W)
                we = min(max(int(np.ceil((pw + 1) * bw if mutant == "exact" else F32(pw + 1) * bw)) + x1, 0), W)
                if he > hs and we > ws:
                    out[r, :, ph, pw] = feat[int(roi[0]), :, hs:he, ws:we].max(axis=(1, 2))
    return out
