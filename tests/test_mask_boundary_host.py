"""Boundary IoU of packed instance masks, the host side (mnc_amd/boundary.py: boundary_distance, boundary_numpy;
mnc_amd/coco_eval.py: match_boundary_numpy, CocoSegmEval(iou_type="boundary"); tools/eval_coco.py --cpu --iou-type boundary; the
argument checks of mnc_mask_boundary and mnc_mask_match_boundary that need no GPU).  The numpy statement is pinned to facts that do
not come from it: closed forms of rectangles, a brute-force window test, scipy's binary_erosion, and matching tables written out by
hand.  Every comparison is exact.

The word-boundary sets of tests/mask_boundary_inputs.py keep the issue's widths and distances, but not its 90 x 260 image for
every distance: a window of 2d + 1 rows does not fit 90 rows once d >= 45, and none of the widths holds 2 * 100 + 1 columns, so
that nothing could survive the erosion there.  The image's height grows with d and each set gains rectangles of at least 2d + 3 a
side; the condition on the inputs (a quarter of the instances with a non-empty E, two with an empty one) is asserted below."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_boundary_inputs as BI  # noqa: E402  (sets up the reference-shaped import paths)
from mnc_amd import _lib, boundary, coco_eval, rle  # noqa: E402
from mnc_amd.boundary import boundary_distance, boundary_numpy  # noqa: E402
from mnc_amd.coco_eval import CocoSegmEval, Match, match_boundary_numpy, match_numpy  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

MM, MI = BI.MM, BI.MI


def test_boundary_distance():
    assert [boundary_distance(H, W) for H, W in ((375, 500), (600, 1000), (64, 64), (20, 30))] == [12, 23, 2, 1]
    assert 0.02 * 625.0 == 12.5                                   # exactly half: rounded to even
    assert boundary_distance(1000, 1000, 1e-6) == 1 and boundary_distance(1, 1) == 1
    assert boundary_distance(600, 1000, 0.01) == 12 and boundary_distance(BI.SQ_H, BI.SQ_W) == BI.SQ_D


def _rect_boundary(H, W, box, d):
    """The closed form: the part of the rectangle inside the image minus that part inset by d on each side -> bool [H, W]."""
    x1, y1, x2, y2 = max(box[0], 0), max(box[1], 0), min(box[2], W - 1), min(box[3], H - 1)
    out = np.zeros((H, W), bool)
    out[y1:y2 + 1, x1:x2 + 1] = True
    out[y1 + d:y2 + 1 - d, x1 + d:x2 + 1 - d] = False
    return out


@pytest.mark.parametrize("box,d", [([40, 20, 89, 49], 4), ([60, 0, 109, 29], 4), ([0, 30, 49, 59], 7), ([150, 50, 199, 79], 3),
                                   ([-10, -5, 39, 24], 4), ([170, 60, 230, 100], 5), ([-3, -3, 202, 82], 6)])
def test_rectangle_gives_the_rectangle_minus_its_inset(box, d):
    H, W = 80, 200
    pm = MM.solid([box])
    got = boundary_numpy(pm, H, W, d)
    want = _rect_boundary(H, W, box, d)
    assert np.array_equal(got.full(0, H, W), want) and got.areas[0] == want.sum()
    a, b = min(box[2], W - 1) - max(box[0], 0) + 1, min(box[3], H - 1) - max(box[1], 0) + 1
    assert a > 2 * d and b > 2 * d and got.areas[0] == a * b - (a - 2 * d) * (b - 2 * d)


def test_rectangle_flush_with_the_top_edge_is_576():
    got = boundary_numpy(MM.solid([[60, 0, 109, 29]]), 80, 200, 4)           # 30 rows of 50 columns
    assert got.areas.tolist() == [576] and got.bounds.tolist() == [[60, 0, 109, 29]]


def test_full_image_gives_a_frame_and_a_thin_mask_is_its_own_boundary():
    H, W, d = 40, 70, 5
    got = boundary_numpy(MM.solid([[0, 0, W - 1, H - 1]]), H, W, d)
    frame = np.ones((H, W), bool)
    frame[d:H - d, d:W - d] = False
    assert np.array_equal(got.full(0, H, W), frame)
    thin = MM.solid([[3, 3, 3 + 2 * d - 1, 38], [3, 3, 60, 3 + 2 * d - 1], [10, 10, 10, 10]])       # w = 2d, h = 2d, one pixel
    got = boundary_numpy(thin, H, W, d)
    assert np.array_equal(got.bits, thin.bits) and np.array_equal(got.areas, thin.areas) and np.array_equal(got.bounds, thin.bounds)


def test_one_unset_pixel_adds_its_window():
    H, W, d = 60, 90, 3
    box = [10, 5, 79, 54]
    m = np.ones((50, 70), bool)
    m[25, 30] = False
    got = boundary_numpy(MI.pack([box], [m]), H, W, d)
    full = boundary_numpy(MM.solid([box]), H, W, d)
    assert got.areas[0] == full.areas[0] + (2 * d + 1) ** 2 - 1
    extra = got.full(0, H, W) & ~full.full(0, H, W)
    ys, xs = np.nonzero(extra)
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (5 + 25 - d, 5 + 25 + d, 10 + 30 - d, 10 + 30 + d)


def _blob_images():
    rng = np.random.default_rng(11)
    return [(H, W, BI.blob(rng, H, W, 6)) for H, W in ((20, 30), (40, 70)) for _ in range(3)]


def _brute(m, d):
    """p in E exactly when the whole (2d+1)^2 window is in the image and set."""
    H, W = m.shape
    e = np.zeros((H, W), bool)
    for y in range(d, H - d):
        for x in range(d, W - d):
            e[y, x] = m[y - d:y + d + 1, x - d:x + d + 1].all()
    return e


def _of_image(m, d):
    H, W = m.shape
    return boundary_numpy(MI.pack([[0, 0, W - 1, H - 1]], [m]), H, W, d).full(0, H, W)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_brute_force_on_blob_masks(d):
    for H, W, m in _blob_images():
        assert np.array_equal(_of_image(m, d), m & ~_brute(m, d)), (H, W)
        # the same blob as an instance whose bounds leave the image: what lies outside is cropped first
        pm = MI.pack([[-7, -4, W - 8, H - 5]], [m], dirty=True)
        inside = m[4:, 7:]
        assert np.array_equal(boundary_numpy(pm, H, W, d).full(0, H, W)[:H - 4, :W - 7], inside & ~_brute(inside, d))


def test_scipy_binary_erosion():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(13)
    cases = [(m, d) for _, _, m in _blob_images() for d in (1, 2, 3)]
    cases += [(BI.blob(rng, 70, 200, 10), 5), (BI.blob(rng, 33, 65, 2), 64), (np.ones((33, 65), bool), 16)]
    for m, d in cases:
        e = ndimage.binary_erosion(m, np.ones((3, 3), bool), iterations=d, border_value=0)
        assert np.array_equal(_of_image(m, d), m & ~e), (m.shape, d)


def test_layout_of_the_result():
    s, got = BI.reference("leaving", BI.leaving_set)
    pm, H, W = s.pm, s.H, s.W
    assert got.bounds.dtype == np.int32 and got.offsets.dtype == np.int64 and got.areas.dtype == np.int64 and got.bits.dtype == np.uint64
    at = 0
    for i in range(len(pm)):
        x1, y1, x2, y2 = (int(v) for v in pm.bounds[i])
        cx1, cy1, cx2, cy2 = max(x1, 0), max(y1, 0), min(x2, W - 1), min(y2, H - 1)
        gone = x2 < x1 or y2 < y1 or cx2 < cx1 or cy2 < cy1
        assert got.bounds[i].tolist() == ([0, 0, -1, -1] if gone else [cx1, cy1, cx2, cy2])          # clipped, not tightened
        assert got.offsets[i] == at and at % 8 == 0
        h, w = got.size(i)
        at += h * ((w + 63) // 64) * 8 if h and w else 0
        assert got.areas[i] == got.dense(i).sum() and (gone or got.areas[i] > 0)
        if h and w and w % 64:                                                                       # padding bits are 0
            rows = got.bits[int(got.offsets[i]) // 8:][:h * ((w + 63) // 64)].reshape(h, -1)
            assert not (rows[:, -1] >> np.uint64(w % 64)).any()
    assert at == got.bits.nbytes
    assert [got.bounds[i].tolist() for i in (8, 9, 12, 13)] == [[0, 0, -1, -1]] * 4 and got.areas[[8, 9, 12, 13]].tolist() == [0] * 4
    assert np.array_equal(got.classes, pm.classes) and np.array_equal(got.scores, pm.scores)
    # dirty input padding changes nothing
    clean = boundary_numpy(BI.leaving_set(dirty=False).pm, H, W, s.d)
    assert not np.array_equal(BI.leaving_set(dirty=False).pm.bits, pm.bits)
    assert all(np.array_equal(getattr(clean, f), getattr(got, f)) for f in PackedMasks.FIELDS)
    none = boundary_numpy(MM.solid([]), 5, 5, 1)
    assert len(none) == 0 and none.bits.size == 0


@pytest.mark.parametrize("d", BI.DISTANCES)
def test_word_boundary_sets_can_fail(d):
    """What keeps tests/test_gpu_mask_boundary.py from passing for nothing: every width, and enough that survives the erosion."""
    s, want = BI.reference(("widths", d), lambda: BI.width_set(d))
    widths = (s.pm.bounds[:, 2] - s.pm.bounds[:, 0] + 1).tolist()
    assert set(BI.WIDTHS) <= set(widths) and 20 <= len(s.pm) <= 28
    e = BI.eroded_areas(s, want)
    assert (e > 0).sum() * 4 >= len(s.pm) and (e == 0).sum() >= 2
    assert (s.pm.bounds[:, 0] % 64 != 0).any()


def test_tall_sets_can_fail():
    for d in BI.TALL_DISTANCES:
        s, want = BI.reference(("tall", d), lambda: BI.tall_set(d))
        assert [s.pm.size(i) for i in range(3)] == [(300, 70), (300, 70), (300, 300)]
        e = BI.eroded_areas(s, want)
        assert (e > 0).tolist() == {1: [True] * 3, 23: [True] * 3, 149: [False, False, True], 150: [False] * 3}[d]
    assert e.tolist() == [0, 0, 0] and BI.eroded_areas(*BI.reference(("tall", 149), None)).tolist() == [0, 0, 2]


# ---- matching ----

def _same(got, want):
    for f, g, w in zip(Match._fields, got, want):
        if w is None:
            assert g is None, f
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f
    return True


def test_rounded_square_matches_by_segm_and_not_by_boundary():
    c = BI.rounded_square()
    seg = match_numpy(c.dt, c.gt, return_iou=True, **c.kw)
    bnd, biou = match_boundary_numpy(c.dt, c.gt, BI.SQ_H, BI.SQ_W, return_iou=True, **c.kw)
    assert seg.iou[0, 0] >= 0.75 and biou[0, 0] < 0.5 and seg.iou[1, 0] == 1.0 and biou[1, 0] == 1.0
    assert seg.iou[0, 0] == 8740.0 / 10000.0                       # the detection lies inside the ground truth
    # T = [0.5, 0.75]: by segm the better-scored detection 0 takes the ground truth at both thresholds ...
    assert seg.rank.tolist() == [0, 1] and seg.dt_match.tolist() == [[[0, -1], [0, -1]]] and seg.gt_match.tolist() == [[[0], [0]]]
    # ... by boundary it matches at none, and detection 1 takes it
    assert bnd.rank.tolist() == [0, 1] and bnd.dt_match.tolist() == [[[-1, 0], [-1, 0]]] and bnd.gt_match.tolist() == [[[1], [1]]]
    assert bnd.dt_ignore.tolist() == [[[0, 0], [0, 0]]] and bnd.gt_ignore.tolist() == [[0]]
    assert np.array_equal(bnd.iou, np.minimum(seg.iou, biou)) and bnd.iou[0, 0] == biou[0, 0]
    at_all = match_boundary_numpy(c.dt, c.gt, BI.SQ_H, BI.SQ_W, **dict(c.kw, iou_thrs=coco_eval.IOU_THRS))
    assert (at_all.dt_match[0, :, 0] == -1).all() and at_all.iou is None


def test_crowd_union_is_the_area_of_the_detection_s_band():
    c = BI.crowd_case()
    m, biou = match_boundary_numpy(c.dt, c.gt, 100, 100, d=2, return_iou=True, **c.kw)
    assert boundary_numpy(c.dt, 100, 100, 2).areas.tolist() == [144]
    assert biou.tolist() == [[76.0 / 144.0]] and m.iou.tolist() == [[76.0 / 144.0]]           # (the mask IoU is 400 / 400)
    assert m.dt_match.tolist() == [[[0], [-1]]] and m.dt_ignore.tolist() == [[[1], [0]]] and m.gt_ignore.tolist() == [[1]]
    # not a crowd: the union is that of the two bands, 144 + 384 - 76
    plain, biou = match_boundary_numpy(c.dt, c.gt, 100, 100, d=2, return_iou=True, **dict(c.kw, iscrowd=[0]))
    assert biou.tolist() == [[76.0 / 452.0]] and plain.dt_match.tolist() == [[[-1], [-1]]]


@pytest.mark.parametrize("name", ["threshold", "identical_gts", "crowd", "max_det", "classes", "no_detections", "no_ground_truths"])
def test_objects_no_wider_than_2d_match_as_by_segm(name):
    c = MM.hand_cases()[name]                                      # every mask is at most 10 pixels wide or high
    got, biou = match_boundary_numpy(c.dt, c.gt, MM.H, MM.W, d=5, return_iou=True, **c.kw)
    want = match_numpy(c.dt, c.gt, return_iou=True, **c.kw)
    assert _same(got, want) and np.array_equal(biou, want.iou)


@pytest.mark.parametrize("seed", BI.BIG_SEEDS)
def test_random_sets_differ_between_the_two_measures(seed):
    c, H, W, d = BI.big_random_set(seed)
    seg = match_numpy(c.dt, c.gt, **c.kw)
    bnd = match_boundary_numpy(c.dt, c.gt, H, W, d=d, **c.kw)
    assert BI.differing(seg, bnd) >= 5 and (bnd.dt_match[0, 0] >= 0).sum() >= 5
    assert np.asarray(c.kw["iscrowd"]).sum() >= 1 and np.array_equal(seg.rank, bnd.rank) and np.array_equal(seg.gt_ignore, bnd.gt_ignore)


def _min_iou_evaluator(sets):
    """The evaluator fed the pre-computed min-IoU by hand: _match_tables on np.minimum of the two IoU tables, then accumulate."""
    records = []
    for c, H, W in sets:
        d = boundary_distance(H, W)
        bd, bg = boundary_numpy(c.dt, H, W, d), boundary_numpy(c.gt, H, W, d)

        def low(crowd, c=c, bd=bd, bg=bg):
            return np.minimum(coco_eval.iou_numpy(c.dt, c.gt, crowd), coco_eval.iou_numpy(bd, bg, crowd))

        m = coco_eval._match_tables(c.dt, c.gt, c.kw["iscrowd"], c.kw["ignore"], c.kw.get("eval_area"), None, None, 100, False, "test",
                                    coco_eval._choose_loop, low)
        records.append(coco_eval.image_record(c.dt, c.gt, m))
    return coco_eval.summarize(coco_eval.accumulate(records))


def test_evaluator_by_boundary():
    sets = [BI.big_random_set(s)[:3] for s in BI.BIG_SEEDS] + [BI.frame(MM.RANDOM_SEEDS[0])]
    ev, seg = CocoSegmEval(device=False, iou_type="boundary"), CocoSegmEval(device=False)
    for i, (c, H, W) in enumerate(sets):
        ev.add(i, c.dt, c.gt, c.kw["iscrowd"], c.kw["ignore"], c.kw.get("eval_area"), image_size=(H, W))
        seg.add(i, c.dt, c.gt, c.kw["iscrowd"], c.kw["ignore"], c.kw.get("eval_area"), image_size=None)       # ignored by segm
    want = _min_iou_evaluator(sets)
    got = ev.summarize()
    assert list(got.values()) == list(want.values()) and len(got) == 12
    assert 0 < got["AP"] < seg.summarize()["AP"] < 1
    with pytest.raises(ValueError):
        CocoSegmEval(device=False, iou_type="boundary").add(0, sets[0][0].dt, sets[0][0].gt, sets[0][0].kw["iscrowd"])
    with pytest.raises(ValueError):
        CocoSegmEval(device=False, iou_type="bbox")


def test_eval_coco_cpu_boundary_equals_the_evaluator_fed_directly(tmp_path):
    gt_path, dt_path, sets = BI.coco_files(tmp_path)
    out_path = str(tmp_path / "stats.json")
    r = BI.tool("--gt", gt_path, "--dt", dt_path, "--cpu", "--iou-type", "boundary", "--out", out_path)
    assert r.returncode == 0, r.stderr[-2000:]
    ev = CocoSegmEval(device=False, classes=[1, 2, 3], iou_type="boundary")
    for name, (c, H, W, d) in sets.items():
        assert boundary_distance(H, W) == 7                         # the tool takes the distance from the file's image sizes
        dt = rle.masks_from_rle_numpy(rle.mask_rle_numpy(c.dt, H, W), c.dt.classes, c.dt.scores)
        gt = rle.masks_from_rle_numpy(rle.mask_rle_numpy(c.gt, H, W), c.gt.classes)
        ev.add(name, dt, gt, c.kw["iscrowd"], c.kw["ignore"], c.gt.areas.astype(np.float64), image_size=(H, W))
    want = ev.summarize()
    with open(out_path) as f:
        got = json.load(f)
    assert [got["stats"][k] for k in want] == list(want.values())
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(" Average")]
    assert lines == ev.lines() and len(lines) == 12
    segm = BI.tool("--gt", gt_path, "--dt", dt_path, "--cpu")
    assert segm.returncode == 0 and segm.stdout != r.stdout
    wide = BI.tool("--gt", gt_path, "--dt", dt_path, "--cpu", "--iou-type", "boundary", "--dilation-ratio", "0.5")
    assert wide.returncode == 0 and wide.stdout == segm.stdout      # bands as wide as the objects: the masks themselves


# ---- the C entries, without a GPU ----

def _boundary_rc(pm, H=50, W=50, d=2, bits="room", **over):
    n = over.get("n", len(pm))
    bounds, offsets, areas = np.zeros((max(n, 1), 4), np.int32), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    need = ctypes.c_size_t(77)
    room = np.zeros(4096, np.uint64) if isinstance(bits, str) else bits
    src = pm.bits if pm.bits.size else np.zeros(1, np.uint64)
    try:
        rc = _lib.call("mnc_mask_boundary", _lib.ptr(pm.bounds), _lib.ptr(pm.offsets), _lib.ptr(src), int(pm.bits.nbytes), n, H, W, d,
                       _lib.ptr(bounds), _lib.ptr(offsets), None if bits is None else _lib.ptr(areas), _lib.ptr(room),
                       over.get("cap", room.nbytes if room is not None else 0), ctypes.addressof(need), 0)
    except _lib.MncError as e:
        rc = e.code
    return rc, bounds, offsets, need.value


def test_boundary_refusals_and_the_sizing_call():
    INVALID = 1
    pm = MM.solid([[5, 5, 14, 14]])
    for kw in ({"d": 0}, {"d": 1025}, {"d": -1}, {"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"n": -1}, {"n": 2049}):
        assert _boundary_rc(pm, **kw)[0] == INVALID, kw
    for field, value in (("bounds", [[0, 0, 2 ** 24, 0]]), ("offsets", [4]), ("offsets", [8]), ("offsets", [-8])):
        bad = MM.solid([[0, 0, 0, 0]])
        bad._host[field] = np.array(value, bad._host[field].dtype)
        assert _boundary_rc(bad)[0] == INVALID, field
    huge = PackedMasks([[0, 0, 2 ** 13, 2 ** 13]], [0], [0], bits=np.zeros(1, np.uint64))
    assert _boundary_rc(huge, bits=None)[0] == INVALID                                              # more than 2^26 pixels
    # bits == NULL: bounds, offsets and the size from the host alone -- nothing is launched, no GPU is needed
    s, want = BI.reference("leaving", BI.leaving_set)
    rc, bounds, offsets, need = _boundary_rc(s.pm, s.H, s.W, s.d, bits=None)
    assert rc == 0 and need == want.bits.nbytes and np.array_equal(bounds, want.bounds) and np.array_equal(offsets, want.offsets)
    got = boundary.boundary_call(s.pm, s.H, s.W, s.d)
    assert got[3] == need and np.array_equal(got[0], want.bounds)
    # too little room: refused with the size set
    small = np.full(need // 8 - 1, 0x5555555555555555, np.uint64)
    rc, bounds, _, size = _boundary_rc(s.pm, s.H, s.W, s.d, bits=small)
    assert rc == INVALID and size == need and (small == np.uint64(0x5555555555555555)).all() and np.array_equal(bounds, want.bounds)
    # n == 0, and a set that lies wholly outside the image: before any device work
    assert _boundary_rc(MM.solid([]))[0] == 0 and _boundary_rc(MM.solid([]))[3] == 0
    outside = MM.solid([[60, 60, 70, 70], [-9, 0, -1, 5]])
    rc, bounds, offsets, need = _boundary_rc(outside)
    assert rc == 0 and need == 0 and bounds.tolist() == [[0, 0, -1, -1]] * 2 and offsets.tolist() == [0, 0]
    none = boundary.boundary(MM.solid([]), 5, 5)
    assert len(none) == 0 and none.bits.size == 0
    gone = PackedMasks.boundary(outside, 50, 50, 2)
    assert gone.bounds.tolist() == [[0, 0, -1, -1]] * 2 and gone.areas.tolist() == [0, 0] and gone.bits.size == 0
    for bad in ({"d": 0}, {"d": 1025}, {"H": 0}, {"W": 40000}):
        with pytest.raises(ValueError):
            boundary_numpy(pm, **dict({"H": 50, "W": 50, "d": 2}, **bad))
        with pytest.raises(ValueError):
            boundary.boundary(pm, **dict({"H": 50, "W": 50, "d": 2}, **bad))


def _match_rc(dt, gt, kw, H=80, W=210, d=2, **over):
    """mnc_mask_match_boundary as it is, with single arguments replaced -> (the return code, the five tables)."""
    thrs = np.array(kw.get("iou_thrs", coco_eval.IOU_THRS), np.float64)
    rngs = np.array(kw.get("area_rngs", coco_eval.AREA_RNGS), np.float64).reshape(-1, 2)
    crowd = np.array(kw.get("iscrowd", np.zeros(len(gt))), np.uint8)
    ign = np.array(kw.get("ignore", np.zeros(len(gt))), np.uint8)
    area = np.array(gt.areas, np.float64)
    scores = np.array(over.get("scores", dt.scores), np.float32)
    D, G = over.get("nd", len(dt)), over.get("ng", len(gt))
    size = max(len(dt), 1) * max(len(gt), 1) * 16 * 8
    out = [np.zeros(size, t) for t in (np.int32, np.int32, np.uint8, np.int32, np.uint8)]
    ptrs = [_lib.ptr(o) for o in out]
    if over.get("null_output") is not None:
        ptrs[over["null_output"]] = None
    args = (_set_args(dt)[:5] + (D, _lib.ptr(dt.classes), _lib.ptr(scores)) + _set_args(gt)[:5] +
            (G, _lib.ptr(gt.classes), _lib.ptr(crowd), _lib.ptr(ign), _lib.ptr(area), _lib.ptr(thrs), over.get("T", len(thrs)),
             _lib.ptr(rngs), over.get("A", len(rngs)), over.get("max_det", kw.get("max_det", 100)), H, W, d) + tuple(ptrs) + (None, None, 0))
    try:
        return _lib.call("mnc_mask_match_boundary", *args), out
    except _lib.MncError as e:
        assert not any(o.any() for o in out)                      # refused before anything was written
        return e.code, out


def test_match_boundary_refusals():
    c = MM.hand_cases()["identical_gts"]
    INVALID = 1

    def rc(kw=None, **over):
        return _match_rc(c.dt, c.gt, dict(c.kw, **(kw or {})), **over)[0]

    assert rc(d=0) == INVALID and rc(d=1025) == INVALID and rc(H=0) == INVALID and rc(W=0) == INVALID
    assert rc(H=32769) == INVALID and rc(W=32769) == INVALID
    assert rc(nd=-1) == INVALID and rc(nd=2049) == INVALID and rc(ng=-1) == INVALID and rc(ng=2049) == INVALID
    assert rc(T=0) == INVALID and rc(T=17) == INVALID and rc(A=0) == INVALID and rc(A=9) == INVALID
    assert rc(max_det=0) == INVALID and rc(max_det=2049) == INVALID and rc(scores=[0.5, float("nan")]) == INVALID
    assert rc({"iou_thrs": [float("nan")]}) == INVALID and rc({"area_rngs": [[2.0, 1.0]]}) == INVALID
    assert rc({"iscrowd": [0, 2]}) == INVALID and rc({"ignore": [255, 0]}) == INVALID
    for k in range(5):
        assert rc(null_output=k) == INVALID
    bad = MM.solid([[0, 0, 0, 0]], [1], [0.5])
    bad._host["offsets"] = np.array([4], np.int64)
    assert _match_rc(bad, c.gt, c.kw)[0] == INVALID and _match_rc(c.dt, bad, dict(c.kw, iscrowd=[0]))[0] == INVALID
    for bad_kw in ({"d": 0}, {"d": 1025}):
        with pytest.raises(ValueError):
            match_boundary_numpy(c.dt, c.gt, 80, 210, **dict(c.kw, **bad_kw))
        with pytest.raises(ValueError):
            coco_eval.match_boundary(c.dt, c.gt, 80, 210, **dict(c.kw, **bad_kw))


@pytest.mark.parametrize("name", ["no_detections", "no_ground_truths", "nothing"])
def test_empty_sets_return_before_any_device_work(name):
    c = MM.hand_cases()[name]
    want = match_numpy(c.dt, c.gt, return_iou=True, **c.kw)
    code, out = _match_rc(c.dt, c.gt, c.kw)
    assert code == 0
    for got, w in zip(out, want[:5]):
        assert np.array_equal(got[:w.size], w.reshape(-1)), name
    got, biou = coco_eval.match_boundary(c.dt, c.gt, 80, 210, return_iou=True, **c.kw)
    assert _same(got, want) and biou.shape == want.iou.shape and biou.dtype == np.float64
    assert _same(c.dt.match_boundary(c.gt, 80, 210, **c.kw), want._replace(iou=None))
    host = match_boundary_numpy(c.dt, c.gt, 80, 210, return_iou=True, **c.kw)
    assert _same(host[0], want) and np.array_equal(host[1], biou)


def test_header_declares_and_library_exports_the_entries():
    decls = _lib.parse_header()
    lib = _lib.load()
    for name, nargs in (("mnc_mask_boundary", 15), ("mnc_mask_match_boundary", 34), ("mnc_mask_boundary_timing", 2)):
        assert name in decls and len(decls[name][1]) == nargs and decls[name][0] is ctypes.c_int
        assert getattr(lib, name) is not None
    assert decls["mnc_mask_match_boundary"][2][:23] == decls["mnc_mask_match"][2][:23]
    assert decls["mnc_mask_match_boundary"][2][23:] == ["H", "W", "d", "rank", "dt_match", "dt_ignore", "gt_match", "gt_ignore", "iou",
                                                        "biou", "device_id"]
    assert decls["mnc_mask_boundary"][2] == ["bounds", "offsets", "bits", "bytes", "n", "H", "W", "d", "out_bounds", "out_offsets",
                                             "out_areas", "out_bits", "bits_cap", "bits_bytes", "device_id"]
    last = ctypes.c_double(0.0)
    assert _lib.call("mnc_mask_boundary_timing", 1, None) == 0                       # switching on forgets the figure kept
    assert _lib.call("mnc_mask_boundary_timing", 0, ctypes.addressof(last)) == 0 and last.value == -1.0
    for fn in ("mask_boundary", "mask_match_boundary"):
        assert callable(getattr(MT, fn))
    assert callable(PackedMasks.boundary) and callable(PackedMasks.match_boundary)
