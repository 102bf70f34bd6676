"""One corpus and the relations BETWEEN the packed-mask entries (include/mnc_hip.h n5 .. n18), shared by
tests/test_mask_cross_host.py (the numpy statements) and tests/test_gpu_mask_cross.py (the GPU entries).  Every family's own test
compares its kernel with its own statement on its own inputs; here the families examine each other on the same pixels:

    A  re-framing       the same pixels framed l columns and t rows further left and up (loosen), the padding bits set (dirty): every
                        result in image coordinates is unchanged.
    B  isometries       the eight lattice isometries of the image commute with every entry, through the map.
    C  between families split / merge, six ways to count, loops rasterised back, the band and the erosion, the erosion and the
                        distance, the duality of erosion and dilation, hulls, overlaps and the algebra, layers, RLE there and back,
                        the resize by two.
    D  producers as consumers   the raw tight-result set of a combine, with empty instances in the middle, through every entry once,
                        against that entry's numpy statement on the same arrays.

A relation is a plain function rel_*(ops, ...) -> [failure strings]; ops is a namespace with one callable per entry (NUMPY_OPS: the
*_numpy statements, GPU_OPS: the GPU entries), so the same code runs on both and the second call of a relation reads the arrays the
first one returned.  Every comparison is exact: np.array_equal or an equality of Python integers or Fractions.  No instance is
exempted; one without rows or without a pixel takes part as the empty case.  The corpus is seeded and built with
PackedMasks.from_dense; nothing is read from disk."""
import collections
import math
import os
import sys
import types
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_boundary_inputs as BI  # noqa: E402  (blob)
import mask_overlap_inputs as MI  # noqa: E402,F401  (sets up the reference-shaped import paths)
from mnc_amd import algebra as AL  # noqa: E402
from mnc_amd import boundary as BD  # noqa: E402
from mnc_amd import components as CC  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402
from mnc_amd import distance as DT  # noqa: E402
from mnc_amd import masks as MK  # noqa: E402
from mnc_amd import polygons as PG  # noqa: E402
from mnc_amd import rle as RL  # noqa: E402
from mnc_amd import shape as SH  # noqa: E402
from mnc_amd import warp as WP  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

H, W = 200, 400                                  # the image
OX, OY = 150, 90                                 # base stands at image coordinates minus this: it has negative coordinates
MARGIN = 12                                      # what the translated corpus keeps from every image edge
LEFTS, TOPS = (1, 31, 63, 64, 65), (0, 2)        # the frames of A: (l, t, 70 - l, 1)
CODES = tuple(range(8))
MORPH_OPS = DT.OPS
EMPTY = (0, 0, -1, -1)

ENTRIES = ("tighten", "combine", "merge", "layer", "isometry", "resize", "components", "select", "fill_holes", "split", "contours",
           "simplify", "from_polygons", "distance", "inscribed", "morph", "moments", "hull", "oriented", "boundary", "overlaps", "nms",
           "rle_counts", "from_rle")


# ---- the namespaces ----

def make_ops(name, **entries):
    """A namespace with one callable per entry of ENTRIES; .calls counts the calls per entry, .memo keeps what a relation computes
    once per namespace (the results on the unframed corpus)."""
    assert sorted(entries) == sorted(ENTRIES), sorted(set(entries) ^ set(ENTRIES))
    ops = types.SimpleNamespace(name=name, calls=collections.Counter(), memo={}, entries=dict(entries))

    def counted(key, fn):
        def call(*args, **kwargs):
            ops.calls[key] += 1
            return fn(*args, **kwargs)
        return call
    for key, fn in entries.items():
        setattr(ops, key, counted(key, fn))
    return ops


def mutated(ops, name, **swap):
    """ops with some entries swapped: a namespace of its own, with its own memo."""
    return make_ops(name, **dict(ops.entries, **swap))


def _window_of_image(H2, W2):
    return (0, 0, int(W2) - 1, int(H2) - 1)


NUMPY_OPS = make_ops(
    "numpy",
    tighten=lambda pm: AL.combine_numpy(pm, None, "copy"),
    combine=AL.combine_numpy,
    merge=lambda pm, groups, intersect=False: AL.merge_numpy(pm, *AL.groups_csr(groups), intersect=intersect),
    layer=AL.layer_numpy,
    isometry=WP.isometry_numpy,
    resize=lambda pm, h, w, h2, w2: WP.warp_numpy(pm, *WP.resize_map(h, w, h2, w2), window=_window_of_image(h2, w2)),
    components=CC.components_numpy, select=CC.select_numpy, fill_holes=CC.fill_holes_numpy, split=CC.split_numpy,
    contours=CT.contours_numpy, simplify=CT.simplify_numpy, from_polygons=PG.masks_from_polygons_numpy,
    distance=DT.distance_numpy, inscribed=DT.inscribed_numpy,
    morph=lambda pm, op, r2, H=None, W=None: DT.morph_numpy(pm, op, r2, H, W),
    moments=SH.moments_numpy, hull=SH.hull_numpy, oriented=SH.oriented_numpy,
    boundary=BD.boundary_numpy, overlaps=MK.mask_overlaps_numpy, nms=MK.mask_nms_numpy,
    rle_counts=RL.rle_counts_numpy, from_rle=RL.masks_from_counts_numpy)

GPU_OPS = make_ops(
    "gpu",
    tighten=lambda pm: pm.tighten(),
    combine=lambda a, b, op, window=None: a.combine(b, op, window),
    merge=lambda pm, groups, intersect=False: pm.merge(groups, intersect),
    layer=lambda pm, order=None: pm.layered(order),
    isometry=lambda pm, code, tx=0, ty=0: pm.isometry(code, tx, ty),
    resize=lambda pm, h, w, h2, w2: pm.resize(h, w, h2, w2),
    components=lambda pm, c=8: pm.components(c),
    select=lambda pm, c=8, min_area=1, keep=0: pm.select(c, min_area, keep),
    fill_holes=lambda pm, c=4: pm.fill_holes(c),
    split=lambda pm, c=8: pm.split(c),
    contours=lambda pm, c=8: pm.contours(c),
    simplify=CT.simplify, from_polygons=PG.masks_from_polygons,
    distance=lambda pm: pm.distance(), inscribed=lambda pm: pm.inscribed(),
    morph=lambda pm, op, r2, H=None, W=None: DT.morph(pm, op, r2=r2, H=H, W=W),
    moments=lambda pm: pm.moments(), hull=lambda pm: pm.hull(), oriented=lambda pm: pm.oriented_boxes(),
    boundary=lambda pm, h, w, d: pm.boundary(h, w, d),
    overlaps=MK.mask_overlaps, nms=MK.mask_nms,
    rle_counts=lambda pm, h, w: pm.rle_counts(h, w), from_rle=RL.masks_from_counts)


def memo(ops, key, make):
    if key not in ops.memo:
        ops.memo[key] = make()
    return ops.memo[key]


# ---- the corpus ----

def smooth_blob(rng, h, w, k=4):
    """bool [h, w]: a random field smoothed by a (2k + 1)^2 box and cut at its median -- organic regions with bays, holes and islets
    -- with a set pixel on each of its four sides, so that the frame is tight."""
    f = np.pad(rng.random((h + 2 * k, w + 2 * k)), ((1, 0), (1, 0)))
    c = np.cumsum(np.cumsum(f, axis=0), axis=1)
    n = 2 * k + 1
    s = c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
    m = s > np.median(s)
    m[0, w // 3] = m[-1, w // 2] = m[h // 3, 0] = m[h // 2, -1] = True
    return m


def _ring_island_hole():
    """41 x 90: a ring three pixels thick, inside it an island, inside the island a hole that lies across column 63|64 and holds one
    pixel."""
    m = np.zeros((41, 90), bool)
    m[:, :] = True
    m[3:-3, 3:-3] = False
    m[8:33, 50:81] = True
    m[15:26, 58:70] = False
    m[20, 64] = True
    return m


def _word_edges():
    """70 x 140: an outline that runs along columns 63|64 and 127|128 and along rows 63|64 of its frame, and two pixels that touch
    at the corner (128, 64) alone -- the last bit of a word and the last row of a block of 64 rows."""
    m = np.zeros((70, 140), bool)
    m[0:64, 0:64] = True                          # its right side: column 63|64, rows 0 .. 19; its lower side: row 63|64
    m[20:64, 64:128] = True                       # its right side: column 127|128; its upper side starts at bit 0 of word 1
    m[64:70, 128:140] = True                      # touches pixel (127, 63) at a corner
    m[30:40, 60:68] = False                       # a hole across column 63|64
    return m


def _checker():
    """8 x 80: a checkerboard of 5 x 26 across column 63|64, with an empty margin inside the frame."""
    m = np.zeros((8, 80), bool)
    yy, xx = np.mgrid[2:7, 50:76]
    m[2:7, 50:76] = (yy + xx) % 2 == 0
    return m


def _staircase():
    """70 x 70: the diagonal (one pixel a row: 70 components under 4, one under 8), and a thick bar it runs into."""
    m = np.eye(70, dtype=bool)
    m[40:52, 5:30] = True
    return m


def _annulus():
    yy, xx = np.mgrid[0:50, 0:150]
    r = ((yy - 24.5) / 25.0) ** 2 + ((xx - 74.5) / 75.0) ** 2
    return (r <= 1.0) & (r >= 0.4)


def _three_parts(rng):
    """25 x 90: three regions of different areas in one frame."""
    m = np.zeros((25, 90), bool)
    m[0:25, 0:30] = BI.blob(rng, 25, 30, 1)
    m[4:20, 36:60] = True
    m[10:25, 66:90] = BI.blob(rng, 15, 24, 0)
    return m


def _runs(lengths):
    """bool [sum(lengths)]: runs of set and unset pixels in turn, a set one first."""
    return np.repeat(np.arange(len(lengths)) % 2 == 0, lengths)


# set runs of 13, 9, 7, 6, 5, 3, 2, 1, 1 pixels: no two of the runs that select(min_area=5, keep=2) ranks are equal (SELECT below)
_LINE_65 = _runs([13, 2, 9, 1, 7, 3, 6, 2, 5, 4, 3, 1, 2, 2, 1, 3, 1])
_LINE_129 = np.concatenate((_LINE_65[::-1], _runs([0, 2, 21, 1, 17, 3, 11, 4, 5])))


def select_ties(table, keep=2, min_area=5):
    """The instances of a component table in which the `keep`-th and the next largest areas >= min_area are equal: there select's
    choice depends on the components' numbers, which an isometry changes."""
    out = []
    for i in range(len(table.comp_ptr) - 1):
        a = sorted((int(v) for v in table.area[int(table.comp_ptr[i]):int(table.comp_ptr[i + 1])] if v >= min_area), reverse=True)
        if len(a) > keep and a[keep - 1] == a[keep]:
            out.append(i)
    return out


def _base_items():
    """[(x, y, dense)] in image coordinates; dense None: the instance without rows."""
    rng = np.random.default_rng(1900)
    loose = np.zeros((64, 100), bool)
    loose[5:50, 7:90] = BI.blob(rng, 45, 83, 2)
    return [
        (12, 12, smooth_blob(rng, 70, 197)),
        (259, 12, smooth_blob(rng, 64, 129)),
        (100, 100, smooth_blob(rng, 65, 128)),
        (14, 118, smooth_blob(rng, 63, 127)),
        (300, 90, BI.blob(rng, 33, 65)),
        (230, 140, BI.blob(rng, 40, 64)),
        (60, 60, smooth_blob(rng, 20, 63, 2)),
        (310, 150, np.ones((17, 70), bool)),                                   # a full rectangle
        (200, 100, np.ones((1, 1), bool)),                                     # a single pixel
        (12, 100, _LINE_65.reshape(65, 1)),                                    # one column
        (140, 187, _LINE_129.reshape(1, 129)),                                 # one row
        (220, 12, np.stack((_LINE_65, np.roll(_LINE_65[::-1], 1) | _runs([1, 63, 1])))),
        (100, 50, np.zeros((5, 70), bool)),                                    # rows and no set pixel
        (0, 0, None),                                                          # no rows, between instances with rows
        (150, 20, _checker()),
        (300, 30, _staircase()),
        (20, 70, _ring_island_hole()),
        (240, 60, _word_edges()),
        (120, 30, loose),                                                      # empty rows and columns inside the frame
        (30, 140, smooth_blob(rng, 40, 130) & (rng.random((40, 130)) > 0.04)),  # pinholes
        (180, 110, BI.blob(rng, 65, 65)),
        (215, 125, _annulus()),
        (50, 150, BI.blob(rng, 30, 191)),
        (100, 15, _three_parts(rng)),
    ]


def _other_items():
    rng = np.random.default_rng(1901)
    return [
        (150, 12, np.ones((109, 181), bool)),                                  # covers several instances of base whole
        (40, 40, smooth_blob(rng, 60, 150)),
        (250, 20, smooth_blob(rng, 64, 64)),
        (200, 90, BI.blob(rng, 70, 130)),
        (100, 140, smooth_blob(rng, 33, 193)),
        (290, 85, rng.random((20, 65)) < 0.5),
        (0, 0, None),
        (20, 80, smooth_blob(rng, 100, 100)),
    ]


def _packed(items):
    n = len(items)
    bounds = [EMPTY if m is None else (x - OX, y - OY, x - OX + m.shape[1] - 1, y - OY + m.shape[0] - 1) for x, y, m in items]
    scores = ((np.arange(n) * 7 % n + 1) / (n + 1.0)).astype(np.float32)
    return PackedMasks.from_dense(np.array(bounds, np.int32), [m for _, _, m in items], np.arange(n) % 3 + 1, scores)


_CORPUS = {}


def base():
    """The 24 instances in their own frame: negative coordinates."""
    if "base" not in _CORPUS:
        _CORPUS["base"] = _packed(_base_items())
    return _CORPUS["base"]


def other():
    """8 instances that overlap base, in base's frame."""
    if "other" not in _CORPUS:
        _CORPUS["other"] = _packed(_other_items())
    return _CORPUS["other"]


def in_image(pm):
    return pm.translate(OX, OY)


def has_rows(pm, i):
    h, w = pm.size(i)
    return h > 0 and w > 0


def loosen(pm, l, t, r, b):
    """The same pixels, the bounds of every instance with rows grown by l, t, r, b empty columns and rows."""
    n = len(pm)
    bounds, dense = np.array(pm.bounds, np.int32).reshape(n, 4), [None] * n
    for i in range(n):
        if has_rows(pm, i):
            bounds[i] += np.array([-l, -t, r, b], np.int32)
            dense[i] = np.pad(pm.dense(i), ((t, b), (l, r)))
    return PackedMasks.from_dense(bounds, dense, pm.classes, pm.scores)


def dirty(pm):
    """The same set with every padding bit (the columns >= w of the last word of a row) set."""
    bits = pm.bits.copy()
    for i in range(len(pm)):
        h, w = pm.size(i)
        if h and w and w % 64:
            lo, words = int(pm.offsets[i]) // 8, (w + 63) // 64
            bits[lo:lo + h * words].reshape(h, words)[:, -1] |= np.uint64(2 ** 64 - 2 ** (w % 64))
    return PackedMasks(pm.bounds, pm.offsets, pm.areas, pm.classes, pm.scores, bits)


# ---- comparing ----

def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def fields(pm):
    """What two equal sets in the canonical layout share (classes and scores are the caller's)."""
    return [("bounds", pm.bounds), ("offsets", pm.offsets), ("areas", pm.areas), ("bits", pm.bits)]


def diff_masks(tag, got, want):
    """-> failure strings: the instances of two sets in the canonical layout that differ."""
    if len(got) != len(want):
        return ["%s: %d instances, not %d" % (tag, len(got), len(want))]
    out = []
    for i in range(len(got)):
        if tuple(got.bounds[i]) != tuple(want.bounds[i]) or got.areas[i] != want.areas[i] or \
                (has_rows(got, i) and not np.array_equal(got.dense(i), want.dense(i))):
            out.append("%s: instance %d is %s area %d, not %s area %d" % (tag, i, tuple(got.bounds[i]), got.areas[i],
                                                                           tuple(want.bounds[i]), want.areas[i]))
    if not out and not all(_same(a, b) for (_, a), (_, b) in zip(fields(got), fields(want))):
        out.append("%s: the same pixels in another layout (offsets or padding bits)" % tag)
    return out


def diff_arrays(tag, got, want):
    out = []
    if len(got) != len(want):
        return ["%s: %d arrays, not %d" % (tag, len(got), len(want))]
    for (name, a), (_, b) in zip(got, want):
        if not _same(a, b):
            a, b = np.asarray(a), np.asarray(b)
            where = ""
            if a.shape == b.shape and a.size:
                at = np.argwhere(a != b)[0]
                where = " first at %s: %s, not %s" % (tuple(int(v) for v in at), a[tuple(at)], b[tuple(at)])
            out.append("%s: %s differs (shapes %s, %s)%s" % (tag, name, a.shape, b.shape, where))
    return out


def same_result(tag, got, want):
    """Two results of one entry, whatever their type -> failure strings."""
    if isinstance(got, PackedMasks):
        return diff_arrays(tag, fields(got) + [("classes", got.classes), ("scores", got.scores)],
                           fields(want) + [("classes", want.classes), ("scores", want.scores)])
    if isinstance(got, CT.Contours):
        return diff_arrays(tag, [(f, getattr(got, f)) for f in got.FIELDS], [(f, getattr(want, f)) for f in want.FIELDS])
    if isinstance(got, tuple):
        if len(got) != len(want):
            return ["%s: %d parts, not %d" % (tag, len(got), len(want))]
        return [f for k, (g, w) in enumerate(zip(got, want)) for f in same_result("%s[%d]" % (tag, k), g, w)]
    if got is None or want is None:
        return [] if got is want else ["%s: one is None" % tag]
    return diff_arrays(tag, [("array", got)], [("array", want)])


def first_pixel(pm, i):
    """(x, y) of the first set pixel of instance i in row-major order, in image coordinates; None without one."""
    if not has_rows(pm, i):
        return None
    ys, xs = np.nonzero(pm.dense(i))
    return (int(pm.bounds[i][0]) + int(xs[0]), int(pm.bounds[i][1]) + int(ys[0])) if len(ys) else None


# ---- A: re-framing ----

Framed = collections.namedtuple("Framed", "pm img other l t r b")


def framed(l=0, t=0, r=0, b=0, dirt=False):
    key = ("framed", l, t, r, b, dirt)
    if key not in _CORPUS:
        pm = base() if (l, t, r, b) == (0, 0, 0, 0) else loosen(base(), l, t, r, b)
        pm = dirty(pm) if dirt else pm
        _CORPUS[key] = Framed(pm, in_image(pm), other(), l, t, r, b)
    return _CORPUS[key]


def _a_tighten(ops, c):
    return fields(ops.tighten(c.pm)), []


def _a_components(ops, c):
    out = []
    for k in (4, 8):
        t = ops.components(c.pm, k)
        out += [("%s/%d" % (f, k), getattr(t, f)) for f in t._fields]
    return out, []


def _a_split(ops, c):
    out = []
    for k in (4, 8):
        s, source = ops.split(c.pm, k)
        out += [("%s/%d" % (f, k), a) for f, a in fields(s)] + [("source/%d" % k, source)]
    return out, []


def _a_fill_holes(ops, c):
    return [("%s/%d" % (f, k), a) for k in (4, 8) for f, a in fields(ops.tighten(ops.fill_holes(c.pm, k)))], []


def _a_select(ops, c):
    return [("%s/%d" % (f, k), a) for k in (4, 8) for f, a in fields(ops.tighten(ops.select(c.pm, k, 5, 2)))], []


def _a_contours(ops, c):
    out = []
    for k in (4, 8):
        ct = ops.contours(c.pm, k)
        out += [("%s/%d" % (f, k), getattr(ct, f)) for f in ct.FIELDS]
        s = ops.simplify(ct, 1.0)
        out += [("simplified %s/%d" % (f, k), getattr(s, f)) for f in s.FIELDS]
    return out, []


def _a_inscribed(ops, c):
    """(xy, r2), and with it the tie-break, which no re-framing can see: under every framing the position is the first pixel in
    row-major order that reaches the largest value of that framing's distance map."""
    xy, r2 = ops.inscribed(c.pm)
    d, fails = ops.distance(c.pm), []
    for i in range(len(c.pm)):
        want = ((-1, -1), 0)
        if has_rows(c.pm, i):
            m = d.map(i)
            at = int(np.argmax(m))
            if m.reshape(-1)[at] > 0:
                want = ((int(c.pm.bounds[i][0]) + at % m.shape[1], int(c.pm.bounds[i][1]) + at // m.shape[1]), int(m.reshape(-1)[at]))
        if (tuple(int(v) for v in xy[i]), int(r2[i])) != want:
            fails.append("inscribed: instance %d gives %s r2 %d, the first maximum of the distance map is %s r2 %d"
                         % (i, tuple(xy[i]), r2[i], want[0], want[1]))
    return [("xy", xy), ("r2", r2)], fails


def _a_distance(ops, c):
    """The maps cropped to the unloosened frame; what is cropped away must be 0."""
    d, out, fails = ops.distance(c.pm), [], []
    for i in range(len(c.pm)):
        if not has_rows(c.pm, i):
            continue
        m = d.map(i)
        inner = m[c.t:m.shape[0] - c.b, c.l:m.shape[1] - c.r]
        if int(m.sum(dtype=np.int64)) != int(inner.sum(dtype=np.int64)):
            fails.append("distance: instance %d is not 0 in the empty rows and columns of its frame" % i)
        out.append(("map %d" % i, inner))
    return out, fails


def _a_moments(ops, c):
    """The sums moved to the unloosened corner in closed form, in Python integers: x = x' - l, y = y' - t."""
    mo = ops.moments(c.pm)
    rows = np.array([has_rows(c.pm, i) for i in range(len(c.pm))])
    origin = np.where(rows[:, None], mo.origin.astype(np.int64) + np.array([c.l, c.t]), mo.origin)
    moved = []
    for m00, m10, m01, m20, m11, m02 in mo.m.tolist():
        l, t = c.l, c.t
        moved.append((m00, m10 - l * m00, m01 - t * m00, m20 - 2 * l * m10 + l * l * m00, m11 - l * m01 - t * m10 + l * t * m00,
                      m02 - 2 * t * m01 + t * t * m00))
    return [("origin", origin), ("m", np.array(moved, object).reshape(len(c.pm), 6))], []


def _a_morph(ops, c):
    return [("%s %s r2=%d" % (f, op, r2), a) for op in MORPH_OPS for r2 in (2, 25)
            for f, a in fields(ops.tighten(ops.morph(c.pm, op, r2)))], []


def _a_hull(ops, c):
    h = ops.hull(c.pm)
    return [(f, getattr(h, f)) for f in h._fields], []


def _a_oriented(ops, c):
    o = ops.oriented(c.pm)
    return [("box", o.box), ("diameter", o.diameter)], []


def _a_boundary(ops, c):
    return [("%s d=%d" % (f, d), a) for d in (1, 3) for f, a in fields(ops.tighten(ops.boundary(c.img, H, W, d)))], []


def _a_rle(ops, c):
    run_ptr, runs = ops.rle_counts(c.img, H, W)
    return [("run_ptr", run_ptr), ("runs", runs)], []


def _a_overlaps(ops, c):
    inter, iou = ops.overlaps(c.pm, c.other)
    return [("inter", inter), ("iou", iou)], []


REFRAME = collections.OrderedDict([
    ("tighten", _a_tighten), ("components", _a_components), ("split", _a_split), ("fill_holes", _a_fill_holes), ("select", _a_select),
    ("contours", _a_contours), ("inscribed", _a_inscribed), ("distance", _a_distance), ("moments", _a_moments), ("morph", _a_morph),
    ("hull", _a_hull), ("oriented", _a_oriented), ("boundary", _a_boundary), ("rle", _a_rle), ("overlaps", _a_overlaps)])


def rel_reframe(ops, l, t, dirt, parts=None):
    """A for one frame (l, t, 70 - l, 1): every part of REFRAME (or `parts`) on the loosened set against the same call on base."""
    c0, c = framed(), framed(l, t, 70 - l, 1, dirt)
    fails = []
    for name in parts or REFRAME:
        want, f0 = memo(ops, ("A", name), lambda: REFRAME[name](ops, c0))
        got, f1 = REFRAME[name](ops, c)
        tag = "A %s l=%d t=%d%s" % (name, l, t, " dirty" if dirt else "")
        fails += ["%s base: %s" % (tag, f) for f in f0] + ["%s: %s" % (tag, f) for f in f1] + diff_arrays(tag, got, want)
    return fails


def frames_of(l):
    return [(l, t, dirt) for t in TOPS for dirt in (False, True)]


# ---- B: isometries ----

def image_isometry(code):
    """-> (tx, ty, H', W'): the translation with which `code` maps the H x W image onto the H' x W' image."""
    w2, h2 = (H, W) if code & 1 else (W, H)
    return (w2 - 1 if code & 2 else 0), (h2 - 1 if code & 4 else 0), h2, w2


def map_array(a, code):
    """An array [y, x] of per-pixel values under the isometry: isometry_numpy's moves."""
    a = a.T if code & 1 else a
    a = a[:, ::-1] if code & 2 else a
    return a[::-1] if code & 4 else a


def map_lattice(xy, code, tx, ty):
    """Lattice points [k, 2] under the isometry: pixel x is the square [x, x + 1], so a negated axis lands one further."""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    u, v = (xy[:, 1], xy[:, 0]) if code & 1 else (xy[:, 0], xy[:, 1])
    u = -u + tx + 1 if code & 2 else u + tx
    v = -v + ty + 1 if code & 4 else v + ty
    return np.stack((u, v), axis=1)


def map_box(box, code, tx, ty):
    return tuple(int(v) for v in WP.isometry_frame(box, code, tx, ty))


def _per_instance(ptr, i):
    return range(int(ptr[i]), int(ptr[i + 1]))


def _rect_area(o, i):
    _, _, _, ex, ey, tmin, tmax, smax = (int(v) for v in o.box[i])
    return Fraction((tmax - tmin) * smax, ex * ex + ey * ey) if ex or ey else Fraction(0)


def _spread(m):
    """(m00, mu20 + mu02) as exact rationals."""
    m00, m10, m01, m20, _, m02 = (int(v) for v in m)
    return (m00, Fraction(m00 * (m20 + m02) - m10 * m10 - m01 * m01, m00) if m00 else Fraction(0))


def _rows_key(pm, i):
    return (tuple(int(v) for v in pm.bounds[i]), pm.dense(i).tobytes() if has_rows(pm, i) else b"")


def rel_isometry(ops, code):
    """B for one code: f = isometry(base in the image) against the entries' results on base in the image, through the map."""
    tx, ty, h2, w2 = image_isometry(code)
    img, oth = framed().img, in_image(other())
    iso = lambda pm: ops.isometry(pm, code, tx, ty)  # noqa: E731
    f = iso(img)
    n, tag, fails = len(img), "B code=%d" % code, []
    for op in MORPH_OPS:
        for r2 in (2, 25):
            want = memo(ops, ("B morph", op, r2), lambda: ops.morph(img, op, r2))
            fails += diff_masks("%s %s r2=%d" % (tag, op, r2), ops.tighten(ops.morph(f, op, r2)), ops.tighten(iso(want)))
    for d in (1, 3):
        want = memo(ops, ("B boundary", d), lambda: ops.boundary(img, H, W, d))
        fails += diff_masks("%s boundary d=%d" % (tag, d), ops.tighten(ops.boundary(f, h2, w2, d)), ops.tighten(iso(want)))
    for k in (4, 8):
        want = memo(ops, ("B fill_holes", k), lambda: ops.fill_holes(img, k))
        fails += diff_masks("%s fill_holes %d" % (tag, k), ops.tighten(ops.fill_holes(f, k)), ops.tighten(iso(want)))
        want = memo(ops, ("B select", k), lambda: ops.select(img, k, 5, 2))
        fails += diff_masks("%s select %d" % (tag, k), ops.tighten(ops.select(f, k, 5, 2)), ops.tighten(iso(want)))
    # the distance maps, pixel by pixel through the map; f is tight, so what of base's map falls outside f's bounds must be 0
    d0, d1 = memo(ops, "B distance", lambda: ops.distance(img)), ops.distance(f)
    for i in range(n):
        if not has_rows(img, i):
            if has_rows(f, i):
                fails.append("%s distance: instance %d got rows" % (tag, i))
            continue
        moved = map_array(d0.map(i), code)
        x1, y1, _, _ = map_box(img.bounds[i], code, tx, ty)
        if not has_rows(f, i):
            ok = not moved.any()
        else:
            fx1, fy1, fx2, fy2 = (int(v) for v in f.bounds[i])
            inner = moved[fy1 - y1:fy2 - y1 + 1, fx1 - x1:fx2 - x1 + 1]
            ok = _same(inner, d1.map(i)) and int(inner.sum(dtype=np.int64)) == int(moved.sum(dtype=np.int64))
        if not ok:
            fails.append("%s distance: the map of instance %d does not follow the isometry" % (tag, i))
    r0, r1 = memo(ops, "B inscribed", lambda: ops.inscribed(img))[1], ops.inscribed(f)[1]
    if not _same(r0, r1):
        fails.append("%s inscribed: r2 %s, not %s" % (tag, r1.tolist(), r0.tolist()))
    for k in (4, 8):
        t0, t1 = memo(ops, ("B components", k), lambda: ops.components(img, k)), ops.components(f, k)
        for i in range(n):
            a = sorted((int(t0.area[c]), map_box(t0.bbox[c], code, tx, ty)) for c in _per_instance(t0.comp_ptr, i))
            b = sorted((int(t1.area[c]), tuple(int(v) for v in t1.bbox[c])) for c in _per_instance(t1.comp_ptr, i))
            if a != b:
                fails.append("%s components %d: instance %d has %d components, %d before; or other areas and boxes"
                             % (tag, k, i, len(b), len(a)))
        (s0, src0), (s1, src1) = memo(ops, ("B split", k), lambda: ops.split(img, k)), ops.split(f, k)
        s0 = iso(s0)
        a = sorted((int(src0[c]),) + _rows_key(s0, c) for c in range(len(s0)))
        b = sorted((int(src1[c]),) + _rows_key(s1, c) for c in range(len(s1)))
        if a != b:
            fails.append("%s split %d: %d instances, %d before; or other bounds and rows" % (tag, k, len(b), len(a)))
        c0, c1 = memo(ops, ("B contours", k), lambda: ops.contours(img, k)), ops.contours(f, k)
        for i in range(n):
            a = sorted(int(c0.area[j]) for j in _per_instance(c0.loop_ptr, i))
            b = sorted(int(c1.area[j]) for j in _per_instance(c1.loop_ptr, i))
            if a != b:
                fails.append("%s contours %d: instance %d has %d loops, %d before; or other areas" % (tag, k, i, len(b), len(a)))
    h0, h1 = memo(ops, "B hull", lambda: ops.hull(img)), ops.hull(f)
    for i in range(n):
        a = sorted(map(tuple, map_lattice(h0.vertices(i), code, tx, ty).tolist()))
        b = sorted(map(tuple, np.asarray(h1.vertices(i), np.int64).reshape(-1, 2).tolist()))
        if a != b or int(h0.area2[i]) != int(h1.area2[i]):
            fails.append("%s hull: instance %d has other vertices or area2 %d, not %d" % (tag, i, h1.area2[i], h0.area2[i]))
    o0, o1 = memo(ops, "B oriented", lambda: ops.oriented(img)), ops.oriented(f)
    for i in range(n):
        if _rect_area(o0, i) != _rect_area(o1, i) or int(o0.diameter[i][0]) != int(o1.diameter[i][0]):
            fails.append("%s oriented: instance %d has rectangle area %s d2 %d, before %s d2 %d"
                         % (tag, i, _rect_area(o1, i), o1.diameter[i][0], _rect_area(o0, i), o0.diameter[i][0]))
    m0, m1 = memo(ops, "B moments", lambda: ops.moments(img)), ops.moments(f)
    for i in range(n):
        if _spread(m0.m[i]) != _spread(m1.m[i]):
            fails.append("%s moments: instance %d has (m00, mu20 + mu02) %s, before %s" % (tag, i, _spread(m1.m[i]), _spread(m0.m[i])))
    i0, i1 = memo(ops, "B overlaps", lambda: ops.overlaps(img, oth)[0]), ops.overlaps(f, iso(oth))[0]
    if not _same(i0, i1):
        fails.append("%s overlaps: inter differs at %s" % (tag, np.argwhere(i0 != i1)[:4].tolist()))
    return fails


# ---- C: between families ----

def _image_set(M):
    return framed().img if M is None else M


def rel_split_merge(ops, M=None):
    """C1."""
    M, fails = _image_set(M), []
    n = len(M)
    tight = ops.tighten(M)
    for k in (4, 8):
        s, source = ops.split(M, k)
        t = ops.components(M, k)
        groups = [np.nonzero(source == i)[0] for i in range(n)]
        fails += diff_masks("C1 merge(split %d)" % k, ops.merge(s, groups), tight)
        counts = np.bincount(source, minlength=n) if len(source) else np.zeros(n, np.int64)
        if not (_same(s.areas, t.area) and _same(s.bounds, t.bbox) and len(s) == len(t.area) and _same(np.diff(t.comp_ptr), counts)):
            fails.append("C1 split %d: its areas, bounds or count are not the table of components" % k)
        for c in range(min(len(s), len(t.anchor))):
            if first_pixel(s, c) != tuple(int(v) for v in t.anchor[c]):
                fails.append("C1 components %d: the anchor %s of component %d is not its first pixel %s"
                             % (k, tuple(t.anchor[c]), c, first_pixel(s, c)))
        for i in range(n):
            for c in _per_instance(t.comp_ptr, i):
                x, y = int(t.anchor[c][0]) - int(M.bounds[i][0]), int(t.anchor[c][1]) - int(M.bounds[i][1])
                h, w = M.size(i)
                if not (0 <= x < w and 0 <= y < h and M.dense(i)[y, x]):
                    fails.append("C1 components %d: the anchor %s of component %d is no set pixel of instance %d"
                                 % (k, tuple(t.anchor[c]), c, i))
    return fails


def _sums(values, ptr):
    return [sum(int(values[j]) for j in _per_instance(ptr, i)) for i in range(len(ptr) - 1)]


def rel_counts(ops, M=None):
    """C2: six ways to count the pixels of every instance."""
    M = _image_set(M)
    run_ptr, runs = ops.rle_counts(M, H, W)
    counts = collections.OrderedDict()
    counts["tighten"] = [int(v) for v in ops.tighten(M).areas]
    counts["moments"] = [int(v) for v in ops.moments(M).m[:, 0]]
    counts["overlaps"] = [int(v) for v in np.diagonal(ops.overlaps(M)[0])]
    counts["rle"] = [sum(int(v) for v in runs[int(run_ptr[i]):int(run_ptr[i + 1])][1::2]) for i in range(len(M))]
    for k in (4, 8):
        ct, t = ops.contours(M, k), ops.components(M, k)
        counts["loops %d" % k] = _sums(ct.area, ct.loop_ptr)
        counts["components %d" % k] = _sums(t.area, t.comp_ptr)
    first = counts["tighten"]
    return ["C2: %s counts %s, tighten %s" % (name, c, first) for name, c in counts.items() if c != first]


def rel_loops(ops, M=None):
    """C3: the loops rasterised one by one and XORed are the instance; their numbers are those of the components."""
    M, fails = _image_set(M), []
    n = len(M)
    for k, other_k in ((4, 8), (8, 4)):
        ct = ops.contours(M, k)
        segs = [[[float(v) for v in ct.loop(j).reshape(-1)]] for j in range(len(ct.area))]
        r = ops.from_polygons(segs, H, W)
        holes = ops.combine(ops.fill_holes(M, other_k), M, "minus")
        t, th = ops.components(M, k), ops.components(holes, other_k)
        for i in range(n):
            acc = np.zeros((H, W), bool)
            for j in _per_instance(ct.loop_ptr, i):
                acc ^= r.full(j, H, W)
            if not np.array_equal(acc, M.full(i, H, W)):
                fails.append("C3 connectivity %d: the XOR of the loops of instance %d differs from it in %d pixels"
                             % (k, i, int((acc ^ M.full(i, H, W)).sum())))
            outer = sum(1 for j in _per_instance(ct.loop_ptr, i) if ct.area[j] > 0)
            inner = sum(1 for j in _per_instance(ct.loop_ptr, i) if ct.area[j] < 0)
            comps, hole_comps = int(t.comp_ptr[i + 1] - t.comp_ptr[i]), int(th.comp_ptr[i + 1] - th.comp_ptr[i])
            if outer != comps or inner != hole_comps or outer + inner != int(ct.loop_ptr[i + 1] - ct.loop_ptr[i]):
                fails.append("C3 connectivity %d: instance %d has %d outer loops for %d components, %d hole loops for %d holes"
                             % (k, i, outer, comps, inner, hole_comps))
    return fails


def rel_band(ops, M=None):
    """C4: the band at distance d is the mask minus d erosions by the 3 x 3 square, the disc of squared radius 2."""
    M, fails = _image_set(M), []
    e = M
    for d in (1, 2, 3):
        e = ops.morph(e, "erode", 2)
        if d != 2:
            fails += diff_masks("C4 d=%d" % d, ops.tighten(ops.boundary(M, H, W, d)), ops.tighten(ops.combine(M, e, "minus")))
    return fails


def rel_erode_distance(ops, M=None, r2s=(0, 2, 25, 100)):
    """C5: erode is a threshold of the distance map."""
    M, fails = _image_set(M), []
    d = ops.distance(M)
    for r2 in r2s:
        e = ops.morph(M, "erode", r2)
        if not _same(e.bounds, M.bounds):
            fails.append("C5 r2=%d: erode changed the bounds" % r2)
            continue
        for i in range(len(M)):
            if has_rows(M, i) and not np.array_equal(e.dense(i), d.map(i) > r2):
                fails.append("C5 r2=%d: erode of instance %d differs from {D > r2} in %d pixels"
                             % (r2, i, int((e.dense(i) ^ (d.map(i) > r2)).sum())))
    return fails


def rel_duality(ops, M=None):
    """C6: erosion is the complement of the dilation of the complement, inside a window that holds every bound grown by rho + 1."""
    M, fails = _image_set(M), []
    b = M.bounds[[has_rows(M, i) for i in range(len(M))]].astype(np.int64)
    for r2 in (2, 25):
        g = math.isqrt(r2) + 1
        wn = (int(b[:, 0].min()) - g, int(b[:, 1].min()) - g, int(b[:, 2].max()) + g, int(b[:, 3].max()) + g)
        grown = ops.morph(ops.combine(M, None, "not", wn), "dilate", r2)
        back = ops.combine(ops.combine(grown, None, "copy", wn), None, "not", wn)        # crop, then the complement
        fails += diff_masks("C6 r2=%d" % r2, ops.tighten(ops.morph(M, "erode", r2)), back)
    return fails


def rel_hull(ops, M=None):
    """C7."""
    M, fails = _image_set(M), []
    h = ops.hull(M)
    for name, pm in (("fill_holes", ops.fill_holes(M, 4)), ("boundary d=1", ops.boundary(M, H, W, 1))):
        g = ops.hull(pm)
        fails += diff_arrays("C7 hull(%s)" % name, [(f, getattr(g, f)) for f in g._fields], [(f, getattr(h, f)) for f in h._fields])
    areas = ops.tighten(M).areas
    for i in range(len(M)):
        if int(h.area2[i]) < 2 * int(areas[i]):
            fails.append("C7: instance %d has area2 %d below twice its area %d" % (i, h.area2[i], areas[i]))
    for k in (4, 8):
        ct = ops.contours(M, k)
        for i in range(len(M)):
            outer = {tuple(p) for j in _per_instance(ct.loop_ptr, i) if ct.area[j] > 0 for p in ct.loop(j).tolist()}
            lost = [tuple(p) for p in h.vertices(i).tolist() if tuple(p) not in outer]
            if lost:
                fails.append("C7 connectivity %d: the hull vertices %s of instance %d are on no outer loop" % (k, lost, i))
    return fails


def rel_overlaps_algebra(ops, M=None, oth=None):
    """C8: the overlaps are the areas of the algebra's intersections, the IoUs the quotients of its unions."""
    M, fails = _image_set(M), []
    oth = in_image(other()) if oth is None else oth
    inter, iou = ops.overlaps(M, oth)
    for j in range(len(oth)):
        one = oth.take([j])
        both, either = ops.combine(M, one, "and").areas, ops.combine(M, one, "or").areas
        if not _same(both, inter[:, j]):
            fails.append("C8: inter[:, %d] is %s, the areas of \"and\" %s" % (j, inter[:, j].tolist(), both.tolist()))
        want = np.array([float(int(a)) / float(int(u)) if u >= 1 else 0.0 for a, u in zip(both, either)], np.float64)
        if want.tobytes() != np.ascontiguousarray(iou[:, j]).tobytes():
            fails.append("C8: iou[:, %d] is not inter / the areas of \"or\" bit for bit" % j)
    return fails


def rel_layers(ops, M=None):
    """C9."""
    M, fails = _image_set(M), []
    lay = ops.layer(M)
    inter = ops.overlaps(lay)[0].copy()
    np.fill_diagonal(inter, 0)
    if inter.any():
        fails.append("C9: the layers overlap at %s" % np.argwhere(inter)[:4].tolist())
    everything = [np.arange(len(M))]
    fails += diff_masks("C9 union", ops.merge(lay, everything), ops.merge(M, everything))
    return fails


def rel_rle_round_trip(ops, M=None):
    """C10: on the corpus in the image, the corpus in its own frame (which leaves the image), a quarter turn, an unclipped dilation
    that leaves the image, and a split."""
    img, fails = _image_set(M), []
    tx, ty, _, _ = image_isometry(6)
    sets = [("in the image", img), ("in its own frame", framed().pm), ("isometry", ops.isometry(img, 6, tx, ty)),
            ("dilate", ops.morph(img, "dilate", 225)), ("split", ops.split(img, 8)[0])]
    for name, pm in sets:
        run_ptr, runs = ops.rle_counts(pm, H, W)
        fails += diff_masks("C10 %s" % name, ops.from_rle(run_ptr, runs, H, W), ops.combine(pm, None, "copy", _window_of_image(H, W)))
    return fails


def rel_resize(ops, M=None):
    """C11: twice the size."""
    M, fails = _image_set(M), []
    m2 = ops.resize(M, H, W, 2 * H, 2 * W)
    if not _same(m2.areas, 4 * ops.tighten(M).areas):
        fails.append("C11: the areas are %s, not four times %s" % (m2.areas.tolist(), ops.tighten(M).areas.tolist()))
    for k in (4, 8):
        c1, c2 = ops.contours(M, k), ops.contours(m2, k)
        fails += diff_arrays("C11 contours %d" % k, [("loop_ptr", c2.loop_ptr), ("vert_ptr", c2.vert_ptr), ("area", c2.area), ("xy", c2.xy)],
                             [("loop_ptr", c1.loop_ptr), ("vert_ptr", c1.vert_ptr), ("area", 4 * c1.area), ("xy", 2 * c1.xy)])
        if not _same(ops.components(M, k).comp_ptr, ops.components(m2, k).comp_ptr):
            fails.append("C11 components %d: the counts changed" % k)
    return fails


RELATIONS_C = collections.OrderedDict([
    ("C1", rel_split_merge), ("C2", rel_counts), ("C3", rel_loops), ("C4", rel_band), ("C5", rel_erode_distance), ("C6", rel_duality),
    ("C7", rel_hull), ("C8", rel_overlaps_algebra), ("C9", rel_layers), ("C10", rel_rle_round_trip), ("C11", rel_resize)])


# ---- D: producers as consumers ----

def raw_result(ops):
    """combine(base in the image, the first of other against every one, "minus") as the entry returned it: tight bounds, gap-free
    offsets, (0, 0, -1, -1) in the middle where the rectangle covers an instance."""
    return ops.combine(framed().img, in_image(other()).take([0]), "minus")


def rel_producers(ops, ref):
    """D: every entry of `ops` once on the raw result of ops.combine, against the same entry of `ref` on the same arrays."""
    R, oth = raw_result(ops), in_image(other())
    n, fails = len(R), []
    one = oth.take([3])
    tx, ty, _, _ = image_isometry(5)
    ct = ops.contours(R, 8)
    run_ptr, runs = ops.rle_counts(R, H, W)
    segs = [ct.polygons(i) for i in range(n)]
    empties = [i for i in range(n) if not has_rows(R, i)]
    groups = [list(range(n)), empties, [], list(range(0, n, 3)), empties[:1] + [0]]
    calls = [("tighten", (R,)), ("layer", (R,)), ("isometry", (R, 5, tx, ty)), ("resize", (R, H, W, 2 * H, 2 * W)),
             ("merge", (R, groups)), ("merge", (R, groups, True)),
             ("combine", (R, None, "not", _window_of_image(H, W))), ("combine", (R, None, "copy", (100, 40, 300, 150))),
             ("select", (R, 8, 5, 2)), ("split", (R, 4)), ("split", (R, 8)),
             ("contours", (R, 4)), ("simplify", (ct, 1.0)), ("from_polygons", (segs, H, W)),
             ("distance", (R,)), ("inscribed", (R,)), ("moments", (R,)), ("hull", (R,)), ("oriented", (R,)),
             ("boundary", (R, H, W, 2)), ("overlaps", (R,)), ("overlaps", (R, oth)), ("overlaps", (oth, R)), ("nms", (R, 0.3)),
             ("rle_counts", (R, H, W)), ("from_rle", (run_ptr, runs, H, W))]
    calls += [("combine", (R, one, op)) for op in ("and", "or", "xor", "minus")] + [("combine", (oth.take([0] * n), R, "minus"))]
    calls += [("components", (R, k)) for k in (4, 8)] + [("fill_holes", (R, k)) for k in (4, 8)]
    calls += [("morph", (R, op, 25)) for op in MORPH_OPS] + [("morph", (R, "dilate", 25, H, W))]
    assert sorted({c[0] for c in calls}) == sorted(ENTRIES)
    for name, args in calls:
        got, want = getattr(ops, name)(*args), getattr(ref, name)(*args)
        if name in ("distance", "moments", "hull", "oriented"):
            got, want = tuple(got), tuple(want)
        tag = "D %s%s" % (name, tuple(a for a in args if isinstance(a, (int, float, str))))
        fails += same_result(tag, got, want)
    return fails
