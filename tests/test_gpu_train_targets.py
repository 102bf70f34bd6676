"""The training-target entries on the GPU (csrc/mask_targets.hip: mnc_mask_targets, mnc_mask_pred_overlaps and the Python surfaces
over them) against the numpy statements (mnc_amd.targets.mask_targets_numpy and mask_pred_overlaps_numpy, which
tests/test_train_targets_host.py pins to the reference's own outputs), and the four layers on the fixture's inputs.  Every
comparison is exact, dtype and shape included; every device call is made twice and the bytes are equal; the raw calls keep canary
bytes around their outputs.  The cases are those of tests/train_target_inputs.py: the smallest at which a kernel can go wrong."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import test_train_targets_host as HT  # noqa: E402
import train_target_inputs as TI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import targets as T  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args, instance_masks, mask_overlaps  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
GUARD = 64
CANARY8 = 0x55
CANARY64 = 0x5555555555555555
same = HT.same


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(REPO, "tests", "golden", "reference_train_targets.npz"))


@pytest.fixture(scope="module")
def corpus():
    return PackedMasks.from_dense(*TI.gt_corpus())


def _targets(gt, boxes, index, S, thresh):
    """mask_targets twice, against the statement."""
    want = T.mask_targets_numpy(gt, boxes, index, S, thresh)
    first = gt.targets(boxes, index, S, thresh)
    assert same(first, want)
    assert T.mask_targets(gt, boxes, index, S, thresh).tobytes() == first.tobytes()
    return first


def _raw_targets(gt, boxes, index, S=21, thresh=0.4, K=None, G=None, null=()):
    """mnc_mask_targets as it is, the output between canaries -> (status, output, guards intact, output untouched)."""
    boxes, index = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4), np.ascontiguousarray(index, np.int32)
    cells = len(boxes) * max(min(S, 32), 1) ** 2
    buf = np.full(cells + 2 * GUARD, CANARY8, np.uint8)
    args = list(_set_args(gt))
    if G is not None:
        args[-1] = G
    args += [None if "boxes" in null else _lib.ptr(boxes), None if "index" in null else _lib.ptr(index), len(boxes) if K is None else K,
             S, float(thresh), None if "out" in null else buf[GUARD:].ctypes.data, 0]
    rc = _lib.load().mnc_mask_targets(*args)
    body = buf[GUARD:GUARD + cells]
    return rc, body, bool((buf[:GUARD] == CANARY8).all() and (buf[GUARD + cells:] == CANARY8).all()), bool((body == CANARY8).all())


# ---- mask_targets ----

@pytest.mark.parametrize("tag", sorted(TI.target_cases()))
def test_mask_targets_cases_equal_the_statement_and_the_reference(fixture, corpus, tag):
    """Identity, touching and disjoint boxes, 1 x 1 / 1 x W / H x 1 boxes, word edges of 63- to 129-wide instances, overhang on
    every side with negative coordinates, a 5 x 7 and a 300 x 200 box, the checkerboard on the threshold, empty instances, K = 0
    and 3000 rows on one instance."""
    c = TI.target_cases()[tag]
    got = _targets(corpus, c["ex_boxes"], c["gt_index"], c["S"], c["thresh"])
    assert same(got, HT.unpack(fixture, "tg_" + tag))
    if tag == "identity":                                  # the identity resize: mask >= thr
        assert same(got[0].astype(bool), corpus.dense(0))
    if tag == "checker":                                   # every cell is exactly 0.5 and >= keeps it
        assert got.all()
        assert not _targets(corpus, c["ex_boxes"], c["gt_index"], 21, float(np.nextafter(np.float32(0.5), np.float32(1)))).any()
    if tag == "touch":
        assert not got[0].any() and got[1:].any()
    if tag == "empty":
        assert not got.any()


@pytest.mark.parametrize("S", [1, 32])
def test_mask_targets_at_other_mask_sizes(corpus, S):
    for tag in ("identity", "thin", "words", "overhang", "scale", "checker"):
        c = TI.target_cases()[tag]
        _targets(corpus, c["ex_boxes"], c["gt_index"], S, c["thresh"])


def test_mask_targets_raw_call_keeps_its_canaries_and_k_zero_writes_nothing(corpus):
    c = TI.target_cases()["words"]
    rc, body, guards, untouched = _raw_targets(corpus, c["ex_boxes"], c["gt_index"])
    assert rc == 0 and guards and not untouched
    assert same(body.reshape(-1, 21, 21), T.mask_targets_numpy(corpus, c["ex_boxes"], c["gt_index"], 21, 0.4))
    rc, body, guards, untouched = _raw_targets(corpus, np.zeros((0, 4), np.int32), np.zeros(0, np.int32))
    assert rc == 0 and guards
    rc, body, guards, untouched = _raw_targets(corpus, c["ex_boxes"], c["gt_index"], K=0)
    assert rc == 0 and guards and untouched
    assert T.mask_targets(corpus, np.zeros((0, 4), np.int32), []).shape == (0, 21, 21)


def test_mask_targets_refusals_write_nothing(corpus):
    G = len(corpus)
    box, one = [[0, 0, 9, 9]], [0]
    bad = [dict(boxes=[[5, 0, 4, 9]]), dict(boxes=[[0, 7, 9, 6]]), dict(boxes=[[0, 0, 2 ** 24, 9]]), dict(boxes=[[-2 ** 24, 0, 9, 9]]),
           dict(boxes=[[0, 0, 8192, 8191]]), dict(index=[G]), dict(index=[-1]), dict(S=0), dict(S=33), dict(thresh=float("nan")),
           dict(K=-1), dict(K=65537), dict(G=-1), dict(null=("boxes",)), dict(null=("index",)), dict(null=("out",))]
    for kw in bad:
        args = dict(boxes=box, index=one)
        args.update(kw)
        rc, body, guards, untouched = _raw_targets(corpus, args.pop("boxes"), args.pop("index"), **args)
        assert rc == INVALID and guards and untouched, kw
    _raw_targets(corpus, box, [-1])
    assert b"gt_index[0] = -1" in _lib.load().mnc_last_error()
    with pytest.raises(ValueError):
        corpus.targets(np.array([[5, 0, 4, 9]]), one)
    # a set whose rows reach past its bytes is refused as mnc_mask_overlaps refuses it
    short = PackedMasks(corpus.bounds, corpus.offsets, corpus.areas, bits=corpus.bits[:-1])
    rc, body, guards, untouched = _raw_targets(short, box, one)
    assert rc == INVALID and untouched
    rc, body, guards, untouched = _raw_targets(corpus, box, one)
    assert rc == 0 and guards and not untouched


# ---- mask_pred_overlaps ----

def _composed(gt, boxes, preds, index, thresh):
    """What the existing device entries give composed: instance_masks(clip=False), mask_overlaps, picked at [k, gt_index[k]]."""
    pm = instance_masks(boxes, preds, 0, 0, clip=False, binarize_thresh=thresh)
    inter, iou = mask_overlaps(pm, gt)
    live = index >= 0
    pick = lambda a: np.where(live, a[np.arange(len(index)), np.maximum(index, 0)], 0).astype(a.dtype)      # noqa: E731
    return pick(inter), np.where(live, pm.areas, 0), pick(iou)


@pytest.mark.parametrize("tag", sorted(TI.label_cases()))
def test_pred_overlaps_cases_equal_the_statement_and_the_composed_entries(fixture, corpus, tag):
    """Boxes ending in .5, unclipped boxes partly and wholly outside the ground truth, widths 1, 64, 65 and 129, a background row
    between live rows; one 600 x 1000 box; predictions all 0, all 1 and on the threshold, both masks empty."""
    c = TI.label_cases()[tag]
    want = T.mask_pred_overlaps_numpy(corpus, c["boxes"], c["preds"], c["gt_index"], c["thresh"])
    first = corpus.pred_overlaps(c["boxes"], c["preds"], c["gt_index"], c["thresh"])
    again = T.mask_pred_overlaps(corpus, c["boxes"], c["preds"], c["gt_index"], c["thresh"])
    for a, b, w, o in zip(first, again, want, _composed(corpus, c["boxes"], c["preds"], c["gt_index"], c["thresh"])):
        assert same(a, w) and a.tobytes() == b.tobytes() and same(a, o)
    assert same(first[2], fixture["lb_%s_iou" % tag])
    if tag == "flat":
        assert first[1].tolist() == [0, 22 * 27, 22 * 27, 0] and first[2][3] == 0.0
    if tag == "boxes":
        assert first[0][10] == 0 and first[1][10] == 0 and first[0][5] == 0 and first[1][5] > 0


def _raw_pred(gt, boxes, preds, index, S=21, thresh=0.4, K=None, G=None, null=()):
    boxes, index = np.ascontiguousarray(boxes, np.float64).reshape(-1, 4), np.ascontiguousarray(index, np.int32)
    preds = np.ascontiguousarray(preds, np.float32)
    n = len(boxes)
    bufs = [np.full(n + 2, CANARY64, np.int64) for _ in range(2)]
    args = list(_set_args(gt))
    if G is not None:
        args[-1] = G
    args += [None if "boxes" in null else _lib.ptr(boxes), None if "preds" in null else _lib.ptr(preds),
             None if "index" in null else _lib.ptr(index), n if K is None else K, S, float(thresh)]
    args += [None if name in null else b[1:].ctypes.data for name, b in zip(("inter", "area"), bufs)] + [0]
    rc = _lib.load().mnc_mask_pred_overlaps(*args)
    guards = all(b[0] == CANARY64 and b[-1] == CANARY64 for b in bufs)
    return rc, [b[1:-1] for b in bufs], guards, all((b[1:-1] == CANARY64).all() for b in bufs)


def test_pred_overlaps_refusals_write_nothing(corpus):
    G = len(corpus)
    pred = np.zeros((1, 21, 21), np.float32)
    box, one = [[0.0, 0.0, 9.0, 9.0]], [0]
    bad = [dict(boxes=[[5.4, 0, 4.4, 9]]), dict(boxes=[[0, 7.2, 9, 6.1]]), dict(boxes=[[0, 0, 2.0 ** 24, 9]]), dict(boxes=[[-2.0 ** 24, 0, 9, 9]]),
           dict(boxes=[[0, 0, float("nan"), 9]]), dict(boxes=[[0, 0, 8192, 8191]]), dict(index=[G]), dict(index=[-2]), dict(S=0), dict(S=33),
           dict(K=-1), dict(K=65537), dict(G=-1), dict(null=("boxes",)), dict(null=("preds",)), dict(null=("index",)),
           dict(null=("inter",)), dict(null=("area",))]
    for kw in bad:
        args = dict(boxes=box, index=one)
        args.update(kw)
        rc, outs, guards, untouched = _raw_pred(corpus, args.pop("boxes"), pred, args.pop("index"), **args)
        assert rc == INVALID and guards and untouched, kw
    # a bad box is refused in a background row too, as instance_masks refuses it
    rc, outs, guards, untouched = _raw_pred(corpus, [[0, 0, 9, 9], [5.4, 0, 4.4, 9]], np.zeros((2, 21, 21), np.float32), [0, -1])
    assert rc == INVALID and guards and untouched
    with pytest.raises(ValueError):
        corpus.pred_overlaps([[5.4, 0, 4.4, 9]], pred, one)
    rc, outs, guards, untouched = _raw_pred(corpus, box, np.ones((1, 21, 21), np.float32), one)
    assert rc == 0 and guards and outs[1][0] == 100 and outs[0][0] == 0                 # instance 0 begins at (10, 20)
    rc, outs, guards, untouched = _raw_pred(corpus, box, pred, one, K=0)
    assert rc == 0 and guards and untouched
    assert [len(a) for a in T.mask_pred_overlaps(corpus, np.zeros((0, 4)), np.zeros((0, 21, 21), np.float32), [])] == [0, 0, 0]


def test_pred_overlaps_rows_without_ground_truth_only(corpus):
    """Nothing is launched for a call whose rows are all background: zeros."""
    got = corpus.pred_overlaps([[0.0, 0, 30, 30]] * 3, np.ones((3, 21, 21), np.float32), [-1, -1, -1])
    assert all(not a.any() for a in got) and got[2].dtype == np.float64


# ---- the layers ----

@pytest.mark.parametrize("scale", TI.SCALES)
def test_the_four_layers_on_the_gpu_equal_the_reference(fixture, scale):
    HT.layers_against_the_fixture(fixture, scale)
