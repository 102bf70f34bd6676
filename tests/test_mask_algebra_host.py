"""The numpy statements of the set algebra of packed masks (mnc_amd.algebra.combine_numpy, merge_numpy, layer_numpy) pinned to facts
that do not come from them: the same operations on full(i, H, W) bool arrays, inclusion-exclusion against mask_overlaps_numpy, De
Morgan, the round trip with split_numpy, boundary_numpy at d = 1, and closed forms.  No GPU: tests/test_gpu_mask_algebra.py pins the
kernels to these statements.  That the word-boundary pairs of tests/mask_algebra_inputs.py can fail -- tight bounds that differ
from the loose frame on all four sides, empty results, funnel shifts that are not 0 -- is asserted here."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_algebra_inputs as AI  # noqa: E402
from mnc_amd import algebra as AL  # noqa: E402
from mnc_amd import components as CC  # noqa: E402
from mnc_amd import distance as DT  # noqa: E402
from mnc_amd.boundary import boundary_numpy  # noqa: E402
from mnc_amd.masks import PackedMasks, instance_masks_numpy, mask_overlaps_numpy  # noqa: E402

DENSE = {"and": np.logical_and, "or": np.logical_or, "xor": np.logical_xor, "minus": lambda p, q: p & ~q}


def shifted(pm, dx, dy):
    b = pm.bounds.copy()
    rows = (b[:, 2] >= b[:, 0]) & (b[:, 3] >= b[:, 1])
    b[rows] += np.array([dx, dy, dx, dy], np.int32)
    return PackedMasks(b, pm.offsets, pm.areas, pm.classes, pm.scores, pm.bits)


def in_image(name):
    """The pair of that name moved into an image that holds all of it -> (a, b, H, W)."""
    a, b = AI.get(name)
    lo = np.minimum(a.bounds[:, :2].min(axis=0), b.bounds[:, :2].min(axis=0))
    a, b = shifted(a, -int(lo[0]) + 2, -int(lo[1]) + 2), shifted(b, -int(lo[0]) + 2, -int(lo[1]) + 2)
    hi = np.maximum(a.bounds[:, 2:].max(axis=0), b.bounds[:, 2:].max(axis=0))
    return a, b, int(hi[1]) + 3, int(hi[0]) + 3


def tight_of(full):
    """bool [H, W] -> (bounds, crop) the way the statements tighten."""
    if not full.any():
        return (0, 0, -1, -1), np.zeros((0, 0), bool)
    ys, xs = np.nonzero(full.any(axis=1))[0], np.nonzero(full.any(axis=0))[0]
    return (xs[0], ys[0], xs[-1], ys[-1]), full[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]


def equals_dense(pm, fulls):
    assert AI.canonical(pm) and len(pm) == len(fulls)
    for i, full in enumerate(fulls):
        bounds, crop = tight_of(full)
        assert tuple(pm.bounds[i]) == tuple(bounds), i
        if crop.size:
            assert np.array_equal(pm.dense(i), crop), i
    return True


def union_of(pm, H, W):
    out = np.zeros((H, W), bool)
    for i in range(len(pm)):
        out |= pm.full(i, H, W)
    return out


# ---- dense arithmetic ----

@pytest.mark.parametrize("name", ["word", "relation"])
def test_every_op_equals_the_op_on_full_arrays_then_a_tight_crop(name):
    a, b, H, W = in_image(name)
    fa, fb = [a.full(i, H, W) for i in range(len(a))], [b.full(i, H, W) for i in range(len(b))]
    for op in AI.BINARY:
        got = AL.combine_numpy(a, b, op)
        assert equals_dense(got, [DENSE[op](p, q) for p, q in zip(fa, fb)]), op
        assert np.array_equal(got.classes, a.classes) and np.array_equal(got.scores, a.scores)
    assert equals_dense(AL.combine_numpy(a, None, "copy"), fa)
    assert equals_dense(AL.combine_numpy(a, None, "not", (0, 0, W - 1, H - 1)), [~p for p in fa])
    win = (40, 3, 300, 30)
    cut = np.zeros((H, W), bool)
    cut[win[1]:win[3] + 1, win[0]:win[2] + 1] = True
    assert equals_dense(AL.combine_numpy(a, b, "xor", win), [(p ^ q) & cut for p, q in zip(fa, fb)])
    assert equals_dense(AL.combine_numpy(a, b.take([3]), "or"), [p | fb[3] for p in fa])


# ---- inclusion-exclusion against mask_overlaps_numpy ----

def test_areas_obey_inclusion_exclusion_and_give_the_iou_of_overlaps():
    a, b = AI.get("word")
    idx = np.arange(0, len(a), 3)
    a, b = a.take(idx), b.take(idx)
    inter, iou = mask_overlaps_numpy(a, b)
    inter, iou = np.diagonal(inter), np.diagonal(iou)
    land, lor, lxor = (AL.combine_numpy(a, b, op).areas for op in ("and", "or", "xor"))
    assert inter.any() and np.array_equal(land, inter)
    assert np.array_equal(lor, a.areas + b.areas - inter)
    assert np.array_equal(lxor, lor - inter)
    some = lor > 0
    assert np.array_equal((land[some].astype(np.float64) / lor[some].astype(np.float64)).view(np.uint64), iou[some].view(np.uint64))
    assert not iou[~some].any()


# ---- complement ----

def test_de_morgan_holds_with_complement():
    a, b, H, W = in_image("relation")
    img = (0, 0, W - 1, H - 1)
    na, nb = AL.combine_numpy(a, None, "not", img), AL.combine_numpy(b, None, "not", img)
    assert AI.same_masks(AL.combine_numpy(AL.combine_numpy(a, b, "or"), None, "not", img), AL.combine_numpy(na, nb, "and"))
    assert AI.same_masks(AL.combine_numpy(AL.combine_numpy(a, b, "and"), None, "not", img), AL.combine_numpy(na, nb, "or"))
    assert AI.same_masks(AL.combine_numpy(na, None, "not", img), AL.combine_numpy(a, None, "copy"))


# ---- identities ----

def test_identities():
    a, _ = AI.get("word")
    tight = AL.combine_numpy(a, None, "copy")
    minus = AL.combine_numpy(a, a, "minus")
    assert not minus.areas.any() and minus.bits.size == 0 and (minus.bounds == (0, 0, -1, -1)).all()
    assert AI.same_masks(AL.combine_numpy(a, a, "or"), tight) and AI.same_masks(AL.combine_numpy(a, a, "and"), tight)
    assert np.array_equal(tight.areas, a.areas) and (tight.bounds != a.bounds).any()


def test_tighten_keeps_every_pixel_of_instance_masks():
    rng = np.random.default_rng(5)
    boxes = np.array([[3.2, 4.1, 80.7, 50.2, 0.9], [-7.0, -3.0, 66.0, 20.0, 0.8], [100.0, 10.0, 163.0, 40.0, 0.7]])
    masks = rng.random((3, 21, 21)).astype(np.float32)
    masks[0, :3] = masks[0, :, -4:] = 0.0
    pm = instance_masks_numpy(boxes, masks, 60, 170, clip=False, binarize_thresh=0.4, classes=[1, 2, 3])
    tight = AL.combine_numpy(pm, None, "copy")
    assert AI.canonical(tight) and np.array_equal(tight.areas, pm.areas) and (tight.bounds[0] != pm.bounds[0]).any()
    pm, tight = shifted(pm, 10, 10), shifted(tight, 10, 10)
    for i in range(3):
        assert np.array_equal(tight.full(i, 80, 190), pm.full(i, 80, 190))


# ---- round trip with split_numpy ----

def test_split_merged_back_by_its_groups_is_the_tightened_set():
    pm = AI.get("crowd").take(np.arange(0, 215, 5))
    parts, source = CC.split_numpy(pm, 8)
    assert len(parts) > len(pm)
    groups = [np.nonzero(source == i)[0] for i in range(len(pm))]
    merged = AL.merge_numpy(parts, *AL.groups_csr(groups))
    want = AL.combine_numpy(pm, None, "copy")
    assert np.array_equal(merged.bounds, want.bounds) and np.array_equal(merged.offsets, want.offsets)
    assert np.array_equal(merged.areas, want.areas) and np.array_equal(merged.bits, want.bits)


# ---- against boundary_numpy ----

def test_minus_the_erosion_is_the_boundary_at_distance_one():
    a, b, H, W = in_image("relation")
    for pm in (a, b):
        band = boundary_numpy(pm, H, W, 1)
        got = AL.combine_numpy(pm, DT.morph_numpy(pm, "erode", 2), "minus")
        assert got.areas.any() and AI.same_masks(got, AL.combine_numpy(band, None, "copy"))


# ---- layer_numpy ----

@pytest.mark.parametrize("name", ["blobs", "equal", "nested_up"])
def test_layers_are_disjoint_and_keep_the_union(name):
    pm = AI.get(name)
    if name == "blobs":
        pm = pm.take(np.arange(0, 300, 4))
    got = AI.reference((name, "layer-host"), lambda: AL.layer_numpy(pm))
    assert AI.canonical(got) and len(got) == len(pm)
    inter, _ = mask_overlaps_numpy(got)
    assert not (inter - np.diag(np.diagonal(inter))).any() and np.array_equal(np.diagonal(inter), got.areas)
    one = np.zeros(2, np.int64), np.arange(len(pm), dtype=np.int32)
    one[0][1] = len(pm)
    whole = AL.merge_numpy(pm, *one)
    assert got.areas.sum() == whole.areas[0] and (got.areas < pm.areas).any()
    assert AI.same_masks(AL.merge_numpy(got, *one), whole)


def test_equal_scores_the_lower_index_wins_and_identical_masks_leave_the_later_ones_empty():
    pm = AI.get("equal")
    got = AL.layer_numpy(pm)
    assert got.areas[0] == pm.areas[0] and (got.areas[1:] < pm.areas[1:]).all()
    assert AI.same_masks(got, AL.layer_numpy(pm, np.arange(8)))
    back = AL.layer_numpy(pm, np.arange(8)[::-1])
    assert back.areas[7] == pm.areas[7] and back.areas[0] < pm.areas[0]
    same = pm.take([2, 2, 2, 2])
    got = AL.layer_numpy(same)
    assert got.areas.tolist() == [int(pm.areas[2]), 0, 0, 0] and (got.bounds[1:] == (0, 0, -1, -1)).all()
    assert np.array_equal(AL.score_order(np.array([0.5, 0.9, 0.5, -0.0, 0.0], np.float32)), [1, 0, 2, 3, 4])
    with pytest.raises(ValueError):
        AL.layer_numpy(pm, [0, 1, 2, 3, 4, 5, 6, 6])
    with pytest.raises(ValueError):
        AL.score_order([0.1, float("nan")])


def test_nested_rectangles_give_rings_or_one_survivor():
    areas = AI.nested_areas()
    rings = AL.layer_numpy(AI.get("nested_up"))
    assert rings.areas.tolist() == (areas - np.append(areas[1:], 0)).tolist() and (rings.areas > 0).all()
    down = AL.layer_numpy(AI.get("nested_down"))
    assert down.areas.tolist() == [int(areas[0])] + [0] * 64


# ---- merge ----

def test_merge_by_class_equals_the_per_class_or_of_full():
    pm = AI.get("crowd")
    H, W = AI.IMAGE_H + 70, AI.IMAGE_W + 70
    pm = shifted(pm, 25, 15)
    distinct, groups = AL.class_groups(pm.classes)
    assert distinct.tolist() == [1, 2, 3]
    got = AL.merge_numpy(pm, *AL.groups_csr(groups))
    fulls = []
    for c in distinct:
        acc = np.zeros((H, W), bool)
        for i in np.nonzero(pm.classes == c)[0]:
            acc |= pm.full(i, H, W)
        fulls.append(acc)
    assert equals_dense(got, fulls) and got.classes.tolist() == [1, 2, 3]
    assert np.array_equal(got.scores, pm.scores[[g[0] for g in groups]])


def test_merge_groups_closed_forms_and_refusals():
    pm = AI.get("crowd")
    got = AL.merge_numpy(pm, *AL.groups_csr(AI.crowd_groups()))
    assert AI.canonical(got) and got.areas[0] == 0 and got.classes[0] == 0 and got.scores[0] == 0.0
    fwd, rev = got.take([3]), got.take([7])                                      # the same members in reverse order
    assert np.array_equal(fwd.bounds, rev.bounds) and np.array_equal(fwd.bits, rev.bits) and fwd.areas[0] == rev.areas[0] > 0
    assert got.areas[6] == AL.merge_numpy(pm, *AL.groups_csr([[3, 7]])).areas[0]  # repeats change nothing
    assert got.areas[8] == 0 and tuple(got.bounds[8]) == (0, 0, -1, -1)
    nested = AI.get("nested_up")
    inner = AL.merge_numpy(nested, *AL.groups_csr([np.arange(65)]), intersect=True)
    assert tuple(inner.bounds[0]) == tuple(nested.bounds[64]) and inner.areas[0] == AI.nested_areas()[64]
    a, b = AI.get("relation")
    both = AI.MI.pack([a.bounds[0], b.bounds[0]], [a.dense(0), b.dense(0)])
    assert AL.merge_numpy(both, *AL.groups_csr([[0, 1]]), intersect=True).areas[0] == 0          # disjoint masks
    assert AL.merge_numpy(pm, *AL.groups_csr([[1, 42]]), intersect=True).areas[0] == 0           # a member without rows
    assert len(AL.merge_numpy(pm, np.zeros(1, np.int64), np.zeros(0, np.int32))) == 0
    for group_ptr, members in (([1, 2], [0, 0]), ([0, 2, 1], [0, 0]), ([0, 1], [215]), ([0, 1], [-1]), ([0, 3], [0, 1])):
        with pytest.raises(ValueError):
            AL.merge_numpy(pm, np.array(group_ptr), np.array(members))


def test_combine_refusals():
    a, b = AI.get("relation")
    for args in ((a, b, "nand"), (a, None, "and"), (a, b.take([0, 1]), "or"), (a, None, "not"), (a, None, "copy", (5, 5, 4, 9)),
                 (a, None, "copy", (0, 0, 2 ** 24, 5)), (a, b, 6)):
        with pytest.raises(ValueError):
            AL.combine_numpy(*args)


# ---- the input sets can fail ----

def test_the_word_boundary_pairs_can_fail():
    a, b = AI.get("word")
    n = len(a)
    wa, ha = a.bounds[:, 2] - a.bounds[:, 0] + 1, a.bounds[:, 3] - a.bounds[:, 1] + 1
    dx, dy = b.bounds[:, 0] - a.bounds[:, 0], b.bounds[:, 1] - a.bounds[:, 1]
    assert set(wa.tolist()) == set(AI.WIDTHS) and set(ha.tolist()) == set(AI.HEIGHTS) and (a.bounds[:, 0] < 0).any()
    assert set(dx.tolist()) == set(AI.DXS) and set(dy.tolist()) == set(AI.DYS)
    assert {(int(w), int(d)) for w, d in zip(wa, dx)} == {(w, d) for w in AI.WIDTHS for d in AI.DXS}
    shrunk = empty = 0
    for op in AI.BINARY:
        got = AI.combined("word", op)
        for i in range(n):
            fa, fb = AL._box(a, i), AL._box(b, i)
            frame = AL._meet(fa, fb) if op == "and" else AL._hull(fa, fb) if op in ("or", "xor") else fa
            t = tuple(int(v) for v in got.bounds[i])
            empty += got.areas[i] == 0
            shrunk += got.areas[i] > 0 and t[0] > frame[0] and t[1] > frame[1] and t[2] < frame[2] and t[3] < frame[3]
    print("of %d results: %d tight on no side of the loose frame, %d empty; %d of %d pairs shifted" %
          (4 * n, shrunk, empty, int((dx % 64 != 0).sum()), n))
    assert 4 * shrunk >= 4 * n and 10 * empty >= 4 * n and 2 * int((dx % 64 != 0).sum()) >= n
