"""The relations between the packed-mask entries (tests/mask_cross_inputs.py) on the numpy statements, without a GPU: every relation
holds for the rules themselves, the corpus has the shapes the relations need, and the relations have teeth -- each of a handful of
subtly wrong entries, swapped into the namespace of statements, is reported.  tests/test_gpu_mask_cross.py runs the same relations
on the GPU entries."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_cross_inputs as X  # noqa: E402
from mnc_amd import boundary as BD  # noqa: E402
from mnc_amd import components as CC  # noqa: E402
from mnc_amd import contours as CT  # noqa: E402
from mnc_amd import distance as DT  # noqa: E402
from mnc_amd import masks as MK  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

OPS = X.NUMPY_OPS


def _report(fails):
    for f in fails:
        print(f)
    return fails


# ---- the relations hold for the rules ----

@pytest.mark.parametrize("l", X.LEFTS)
def test_reframing_changes_nothing(l):
    for frame in X.frames_of(l):
        assert _report(X.rel_reframe(OPS, *frame)) == []


@pytest.mark.parametrize("code", X.CODES)
def test_isometries_commute(code):
    assert _report(X.rel_isometry(OPS, code)) == []


@pytest.mark.parametrize("name", list(X.RELATIONS_C))
def test_between_families(name):
    assert _report(X.RELATIONS_C[name](OPS)) == []


def test_counts_and_overlaps_ignore_padding_bits():
    img = X.dirty(X.framed().img)
    assert _report(X.rel_counts(OPS, img)) == []
    assert _report(X.rel_overlaps_algebra(OPS, img, X.dirty(X.in_image(X.other())))) == []


def test_producers_as_consumers():
    assert _report(X.rel_producers(OPS, OPS)) == []
    assert sorted(k for k, v in OPS.calls.items() if v) == sorted(X.ENTRIES)


# ---- the corpus ----

def test_corpus_shapes():
    pm, img = X.base(), X.framed().img
    n = len(pm)
    assert n == 24 and len(X.other()) == 8
    tight = OPS.tighten(pm)
    sizes = [tight.size(i) for i in range(n)]
    assert {1, 63, 64, 65, 127, 128, 129} <= {w for _, w in sizes} and any(191 <= w <= 200 for _, w in sizes)
    assert {1, 2, 63, 64, 65, 70} <= {h for h, _ in sizes}
    assert (pm.bounds < 0).any() and (pm.bounds[:, 2] > 0).any()
    rows = [i for i in range(n) if X.has_rows(img, i)]
    b = img.bounds[rows]
    assert b[:, 0].min() == X.MARGIN and b[:, 1].min() == X.MARGIN                    # the margin, reached on every side
    assert b[:, 2].max() == X.W - 1 - X.MARGIN and b[:, 3].max() == X.H - 1 - X.MARGIN
    assert any(sizes[i] == (1, 1) and pm.areas[i] == 1 for i in range(n))             # a single pixel
    assert any(pm.areas[i] == np.prod(pm.size(i)) > 100 for i in range(n))            # a full rectangle
    assert any(X.has_rows(pm, i) and pm.areas[i] == 0 for i in range(n))              # rows and no set pixel
    rowless = [i for i in range(n) if tuple(pm.bounds[i]) == X.EMPTY]
    assert rowless and all(0 < i < n - 1 and X.has_rows(pm, i - 1) and X.has_rows(pm, i + 1) for i in rowless)
    assert (tight.bounds[rows] != pm.bounds[rows]).any(axis=1).sum() >= 2             # empty rows and columns inside a frame
    assert np.array_equal(X.in_image(tight).bounds[rows], OPS.tighten(img).bounds[rows])


def test_corpus_topology():
    img = X.framed().img
    n = len(img)
    c4, c8 = OPS.components(img, 4), OPS.components(img, 8)
    assert (np.diff(c4.comp_ptr) != np.diff(c8.comp_ptr)).sum() >= 4
    assert X.select_ties(c4) == [] and X.select_ties(c8) == []                        # what B asks of select(min_area=5, keep=2)
    ct = OPS.contours(img, 8)
    holes = [sum(1 for j in range(int(ct.loop_ptr[i]), int(ct.loop_ptr[i + 1])) if ct.area[j] < 0) for i in range(n)]
    assert sum(h > 0 for h in holes) >= 3
    # a hole that holds an island that holds a hole: filling the holes adds a region that has itself components of the instance
    ring = 16
    inner = OPS.combine(OPS.fill_holes(img, 4), img, "minus").take([ring])
    part, source = OPS.split(img.take([ring]), 8)
    inter = OPS.overlaps(OPS.fill_holes(inner, 4), part)[0][0]
    assert len(part) == 3 and (inter[1:] == part.areas[1:]).all() and inter[0] == 0 and holes[ring] == 2
    # an outline along columns 63|64 and 127|128 and along row 63|64 of the frame, and a corner touch at (128, 64)
    m = img.dense(17)
    assert (m[:20, 63] & ~m[:20, 64]).all() and (m[20:64, 127] & ~m[20:64, 128]).all() and (m[63, :128] & ~m[64, :128]).all()
    assert m[63, 127] and m[64, 128] and not m[63, 128] and not m[64, 127]


def test_corpus_keeps_the_morphology_busy():
    img = X.framed().img
    n = len(img)
    assert (OPS.morph(img, "erode", 25).areas > 0).sum() * 3 >= n
    band = OPS.boundary(img, X.H, X.W, 3)
    assert ((band.areas != img.areas) & (img.areas > 0)).sum() * 2 >= n
    for d in (1, 3):                                                                   # C4's margin
        assert X.MARGIN >= d
    assert (OPS.morph(img, "dilate", 225).bounds[:, :2] < 0).any()                     # C10's dilation leaves the image
    xy, r2 = OPS.inscribed(img)
    d = OPS.distance(img)
    assert sum((d.map(i) == r2[i]).sum() > 1 for i in range(n) if r2[i] > 0) >= 5      # ties for the inscribed disc


def test_the_raw_result_has_empty_instances_in_the_middle():
    img, R = X.framed().img, X.raw_result(OPS)
    gone = [i for i in range(len(R)) if img.areas[i] > 0 and tuple(R.bounds[i]) == X.EMPTY]
    assert len(gone) >= 3 and all(0 < i < len(R) - 1 for i in gone)
    assert any(R.areas[i + 1] > 0 and R.offsets[i + 1] == R.offsets[i] for i in gone)  # gap-free offsets past an empty instance
    assert (X.framed().pm.bounds < 0).any() and (R.areas > 0).sum() >= 12


def test_loosen_and_dirty_keep_the_pixels():
    pm = X.base()
    for l, t, dirt in ((1, 0, False), (64, 2, True)):
        c = X.framed(l, t, 70 - l, 1, dirt)
        for i in range(len(pm)):
            h, w = pm.size(i)
            if not X.has_rows(pm, i):
                assert tuple(c.pm.bounds[i]) == tuple(pm.bounds[i])
                continue
            assert tuple(c.pm.bounds[i] - pm.bounds[i]) == (-l, -t, 70 - l, 1)
            m = c.pm.dense(i)
            assert np.array_equal(m[t:t + h, l:l + w], pm.dense(i)) and m.sum() == pm.areas[i] == c.pm.areas[i]
        clean = X.framed(l, t, 70 - l, 1, False).pm
        assert np.array_equal(clean.bits, c.pm.bits) != dirt


# ---- teeth: subtly wrong entries are reported ----

def _words(w):
    return [(a, min(a + 64, w)) for a in range(0, w, 64)]


def _erode_in_words(pm, op, r2, H=None, W=None):
    """An erosion that treats each 64-column word of a row as isolated."""
    if op not in ("erode", 0):
        return DT.morph_numpy(pm, op, r2, H, W)
    dense = [np.concatenate([DT.erode_numpy(pm.dense(i)[:, a:b], r2) for a, b in _words(pm.size(i)[1])], axis=1)
             if X.has_rows(pm, i) else None for i in range(len(pm))]
    return PackedMasks.from_dense(pm.bounds, dense, pm.classes, pm.scores)


def _components_in_words(pm, connectivity=8):
    """A labelling that does not join pixels across a word."""
    comp_ptr, area, bbox, anchor = [0], [], [], []
    for i in range(len(pm)):
        found = []
        if X.has_rows(pm, i):
            m, x1, y1 = pm.dense(i), int(pm.bounds[i][0]), int(pm.bounds[i][1])
            for a, b in _words(m.shape[1]):
                labels, count = CC.label_numpy(m[:, a:b], connectivity)
                for c in range(1, count + 1):
                    ys, xs = np.nonzero(labels == c)
                    found.append(((int(ys[0]) + y1, int(xs[0]) + a + x1), len(ys),
                                  (int(xs.min()) + a + x1, int(ys.min()) + y1, int(xs.max()) + a + x1, int(ys.max()) + y1)))
        for (y, x), count, box in sorted(found):
            area.append(count), bbox.append(box), anchor.append((x, y))
        comp_ptr.append(len(area))
    return CC.Components(np.array(comp_ptr, np.int64), np.array(area, np.int64), np.array(bbox, np.int32).reshape(-1, 4),
                         np.array(anchor, np.int32).reshape(-1, 2))


def _boundary_in_blocks(pm, H, W, d):
    """A band whose erosion does not look across the edge of a block of 64 rows of the frame."""
    def erode(m):
        h, w = m.shape
        p = np.pad(m, ((0, 0), (d, d)))
        rows = np.ones((h, w), bool)
        for s in range(2 * d + 1):
            rows &= p[:, s:s + w]
        out = np.ones((h, w), bool)
        for a in range(0, h, 64):
            b = min(a + 64, h)
            q = np.concatenate((np.full((d, w), a > 0), rows[a:b], np.full((d, w), b < h)))
            for s in range(2 * d + 1):
                out[a:b] &= q[s:s + b - a]
        return out
    want = BD.boundary_numpy(pm, H, W, d)
    dense = [None] * len(want)
    for i in range(len(want)):
        if X.has_rows(want, i):
            x1, y1, x2, y2 = (int(v) for v in want.bounds[i])
            m = pm.full(i, H, W)[y1:y2 + 1, x1:x2 + 1]
            dense[i] = m & ~erode(m)
    return PackedMasks.from_dense(want.bounds, dense, pm.classes, pm.scores)


def _overlaps_with_padding(a, b=None):
    """Overlaps that count the padding bits of the last word of a row as pixels."""
    def wide(pm):
        bounds = pm.bounds.copy()
        for i in range(len(pm)):
            if X.has_rows(pm, i):
                bounds[i][2] = bounds[i][0] + (pm.size(i)[1] + 63) // 64 * 64 - 1
        return PackedMasks(bounds, pm.offsets, pm.areas, pm.classes, pm.scores, pm.bits)
    return MK.mask_overlaps_numpy(wide(a), None if b is None else wide(b))


def _inscribed_highest(pm):
    """The deepest pixel with ties to the highest (y, x)."""
    xy, r2 = DT.inscribed_numpy(pm)
    d = DT.distance_numpy(pm)
    for i in range(len(pm)):
        if r2[i] > 0:
            m = d.map(i)
            at = m.size - 1 - int(np.argmax(m.reshape(-1)[::-1]))
            xy[i] = (int(pm.bounds[i][0]) + at % m.shape[1], int(pm.bounds[i][1]) + at // m.shape[1])
    return xy, r2


def _contours_wrong_turn(pm, connectivity=8):
    """A trace that takes the other turn wherever two pixels touch at a corner alone."""
    return CT.contours_numpy(pm, 12 - connectivity)


def _contours_wrong_turn_at_words(pm, connectivity=8):
    """The same slip only in an instance with such a corner at the first bit of a word of its frame."""
    good, bad = CT.contours_numpy(pm, connectivity), CT.contours_numpy(pm, 12 - connectivity)
    loop_ptr, vert_ptr, area, xy = [0], [0], [], []
    for i in range(len(pm)):
        src = good
        if X.has_rows(pm, i):
            m = pm.dense(i)
            a, b, c, d = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
            alone = (a & d & ~b & ~c) | (b & c & ~a & ~d)
            if alone[:, 63::64].any():
                src = bad
        for j in range(int(src.loop_ptr[i]), int(src.loop_ptr[i + 1])):
            xy.extend(src.loop(j).tolist())
            vert_ptr.append(len(xy))
            area.append(int(src.area[j]))
        loop_ptr.append(len(area))
    return CT.Contours(loop_ptr, vert_ptr, area, np.array(xy, np.int32).reshape(-1, 2))


def _reframe_reports(ops, part, dirt=(False, True)):
    return [f for l in X.LEFTS for t in X.TOPS for d in dirt for f in X.rel_reframe(ops, l, t, d, [part])]


def test_teeth_erosion_that_isolates_words():
    ops = X.mutated(OPS, "erode in words", morph=_erode_in_words)
    assert _reframe_reports(ops, "morph") and X.rel_erode_distance(ops, r2s=(2, 25)) and X.rel_band(ops) and X.rel_duality(ops)
    assert any("code=%d" % code in f and "erode" in f for code in (1, 2) for f in X.rel_isometry(ops, code))


def test_teeth_components_that_isolate_words():
    ops = X.mutated(OPS, "components in words", components=_components_in_words)
    assert _reframe_reports(ops, "components") and X.rel_split_merge(ops) and X.rel_loops(ops)
    assert any("components" in f for f in X.rel_isometry(ops, 2))


def test_teeth_boundary_that_stops_at_a_block_of_rows():
    ops = X.mutated(OPS, "boundary in blocks", boundary=_boundary_in_blocks)
    assert _reframe_reports(ops, "boundary") and X.rel_band(ops)
    assert any("boundary" in f for f in X.rel_isometry(ops, 4))


def test_teeth_overlaps_that_trust_padding_bits():
    ops = X.mutated(OPS, "overlaps with padding", overlaps=_overlaps_with_padding)
    assert _reframe_reports(ops, "overlaps", dirt=(True,)) and _reframe_reports(ops, "overlaps", dirt=(False,)) == []
    img = X.dirty(X.framed().img)
    assert X.rel_counts(ops, img) and X.rel_overlaps_algebra(ops, img, X.dirty(X.in_image(X.other())))
    assert X.rel_counts(ops) == []                                                     # clean padding hides it


def test_teeth_inscribed_that_breaks_ties_the_other_way():
    ops = X.mutated(OPS, "inscribed highest", inscribed=_inscribed_highest)
    assert _reframe_reports(ops, "inscribed")
    assert not any("inscribed" in f for f in X.rel_isometry(ops, 6))                   # B compares r2 alone: it cannot see a tie


def test_teeth_contours_that_turn_the_wrong_way():
    ops = X.mutated(OPS, "contours wrong turn", contours=_contours_wrong_turn)
    assert X.rel_loops(ops) and X.rel_counts(ops) == []                                # the loops' areas still add up: C3 sees it
    ops =X.mutated(OPS, "contours wrong turn at words", contours=_contours_wrong_turn_at_words)
    assert _reframe_reports(ops, "contours") and X.rel_loops(ops)
