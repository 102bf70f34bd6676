"""The boundary bands of packed instance masks and the matching on min(mask IoU, boundary IoU) on the GPU (csrc/mask_boundary.hip,
csrc/mask_match.hip: mnc_mask_boundary, mnc_mask_match_boundary and the Python surfaces over them) against the numpy statements
(mnc_amd.boundary.boundary_numpy, mnc_amd.coco_eval.match_boundary_numpy, which tests/test_mask_boundary_host.py pins to facts that
do not come from them).  Every comparison is exact.  The sets are those of tests/mask_boundary_inputs.py; that the word-boundary
sets can fail (a quarter of their instances keep something after the erosion) is asserted of the numpy statement in the host test,
which also says why their image is not 90 x 260 at every distance."""
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_boundary_inputs as BI  # noqa: E402
from mnc_amd import _lib, boundary, coco_eval  # noqa: E402
from mnc_amd.coco_eval import CocoSegmEval, Match, match_boundary, match_boundary_numpy, match_numpy  # noqa: E402
from mnc_amd.instances import HEAD_BYTES, InstanceBlock, records_from_lists  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

MM, MI, RI = BI.MM, BI.MI, BI.RI
_WANT = {}


def _same_masks(got, want):
    for f in PackedMasks.FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
    return True


def _same(got, want):
    for f, g, w in zip(Match._fields, got, want):
        if w is None:
            assert g is None, f
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f
    return True


def _check(s, want):
    got = boundary.boundary(s.pm, s.H, s.W, s.d)
    assert _same_masks(got, want)
    return got


@pytest.mark.parametrize("d", BI.DISTANCES)
def test_word_boundary_widths(d):
    s, want = BI.reference(("widths", d), lambda: BI.width_set(d))
    assert set(BI.WIDTHS) <= set((s.pm.bounds[:, 2] - s.pm.bounds[:, 0] + 1).tolist())
    assert (BI.eroded_areas(s, want) > 0).sum() * 4 >= len(s.pm)
    _check(s, want)


@pytest.mark.parametrize("d", BI.TALL_DISTANCES)
def test_tall_narrow_instances(d):
    s, want = BI.reference(("tall", d), lambda: BI.tall_set(d))
    got = _check(s, want)
    if d == 150:                                                   # everything erodes: the masks themselves
        assert np.array_equal(got.bits, s.pm.bits)


@pytest.mark.parametrize("d", [3, 40, 70])
def test_bounds_leaving_the_image(d):
    s, want = BI.reference(("leaving", d), lambda: BI.leaving_set(d))
    assert sorted(set((-s.pm.bounds[:4, 0] % 64).tolist())) == [1, 63]                 # unaligned source shifts
    assert want.bounds[8].tolist() == [0, 0, -1, -1] and want.bounds[7].tolist() == [0, 0, s.W - 1, s.H - 1]
    got = _check(s, want)
    assert (got.areas[[8, 9, 10, 11, 12, 13]] == 0).all()
    clean = BI.leaving_set(d, dirty=False)                         # the dirty padding of the input changed nothing
    assert not np.array_equal(clean.pm.bits, s.pm.bits) and _same_masks(boundary.boundary(clean.pm, s.H, s.W, d), want)


def test_real_size_and_repeatability():
    s, want = BI.reference("real", BI.real_set)
    assert (s.H, s.W, s.d) == (600, 1000, boundary.boundary_distance(600, 1000)) and len(s.pm) == 10
    assert (BI.eroded_areas(s, want) > 0).sum() >= 2 and (s.pm.bounds[:, 0] < 0).any()
    got = _check(s, want)
    again = s.pm.boundary(s.H, s.W)                               # d from the image; the same bytes from run to run
    assert all(getattr(again, f).tobytes() == getattr(got, f).tobytes() for f in PackedMasks.FIELDS)
    assert _same_masks(MT.mask_boundary(s.pm, s.H, s.W), want) and _same_masks(MT.mask_boundary(s.pm, s.H, s.W, s.d), want)


def test_room_to_spare_stays_as_it_was():
    s, want = BI.reference(("leaving", 3), lambda: BI.leaving_set(3))
    need = want.bits.nbytes
    roomy = np.full(need // 8 + 4, 0x5555555555555555, np.uint64)
    bounds, offsets, areas, size = boundary.boundary_call(s.pm, s.H, s.W, s.d, roomy)
    assert size == need and np.array_equal(roomy[:need // 8], want.bits) and (roomy[need // 8:] == np.uint64(0x5555555555555555)).all()
    assert np.array_equal(areas, want.areas) and np.array_equal(bounds, want.bounds) and np.array_equal(offsets, want.offsets)


# ---- matching ----

def _want(key, make):
    """(Case, H, W, d), the numpy tables with both IoU tables, and the segm tables -- computed once."""
    if key not in _WANT:
        c, H, W, d = make()
        m, biou = match_boundary_numpy(c.dt, c.gt, H, W, d=d, return_iou=True, **c.kw)
        _WANT[key] = (c, H, W, d, m, biou, match_numpy(c.dt, c.gt, **c.kw))
    return _WANT[key]


def _match_checks(c, H, W, d, want, biou):
    got, gb = match_boundary(c.dt, c.gt, H, W, d=d, return_iou=True, **c.kw)
    assert _same(got, want) and gb.dtype == biou.dtype and gb.shape == biou.shape and np.array_equal(gb, biou)
    assert _same(match_boundary(c.dt, c.gt, H, W, d=d, **c.kw), want._replace(iou=None))           # without the IoU outputs
    return got


@pytest.mark.parametrize("name", ["rounded_square", "crowd_band"] + list(MM.hand_cases()))
def test_hand_made_cases(name):
    if name == "rounded_square":
        make = lambda: (BI.rounded_square(), BI.SQ_H, BI.SQ_W, None)  # noqa: E731
    elif name == "crowd_band":
        make = lambda: (BI.crowd_case(), 100, 100, 2)  # noqa: E731
    else:
        make = lambda: (MM.hand_cases()[name], MM.H, MM.W, 2)  # noqa: E731
    c, H, W, d, want, biou, _ = _want(name, make)
    _match_checks(c, H, W, d, want, biou)
    assert _same(c.dt.match_boundary(c.gt, H, W, d=d, **c.kw), want._replace(iou=None))
    m, b = MT.mask_match_boundary(c.dt, c.gt, H, W, d=d, return_iou=True, **c.kw)
    assert _same(m, want) and np.array_equal(b, biou)
    if name == "rounded_square":
        assert want.dt_match.tolist() == [[[-1, 0], [-1, 0]]] and biou[0, 0] < 0.5 <= 0.75 <= want.iou[1, 0]


@pytest.mark.parametrize("n_gt,n_dt", [(65, 65), (70, 130), (129, 130)])
def test_more_than_one_chunk_of_ground_truths(n_gt, n_dt):
    c, H, W, d, want, biou, _ = _want((n_gt, n_dt), lambda: (MM.chunk_set(n_gt, n_dt, n_gt), MM.H + 2, MM.W + 2, 2))
    assert (c.gt.classes == 1).sum() == n_gt and (want.dt_match[0, 0] >= 64).sum() > 0
    assert (biou != want.iou).any()
    _match_checks(c, H, W, d, want, biou)


@pytest.mark.parametrize("seed", MM.RANDOM_SEEDS)
def test_random_sets_of_the_segm_tests(seed):
    c, H, W, d, want, biou, _ = _want(seed, lambda: BI.frame(seed) + (2,))
    assert np.asarray(c.kw["iscrowd"]).sum() >= 2 and np.asarray(c.kw["ignore"]).sum() >= 1 and (biou != want.iou).any()
    _match_checks(c, H, W, d, want, biou)


@pytest.mark.parametrize("seed", BI.BIG_SEEDS)
def test_random_sets_on_which_the_measures_differ(seed):
    c, H, W, d, want, biou, seg = _want(("big", seed), lambda: BI.big_random_set(seed))
    assert BI.differing(seg, want) >= 5                            # the input condition, of the host statement
    got = _match_checks(c, H, W, d, want, biou)
    assert BI.differing(seg, got) >= 5
    # d from the image and another ratio
    for kw in ({}, {"ratio": 0.05}):
        assert _same(match_boundary(c.dt, c.gt, H, W, return_iou=True, **dict(c.kw, **kw))[0],
                     match_boundary_numpy(c.dt, c.gt, H, W, return_iou=True, **dict(c.kw, **kw))[0])
    dirty = MI.pack(c.dt.bounds.tolist(), [c.dt.dense(i) for i in range(len(c.dt))], c.dt.classes, c.dt.scores, dirty=True)
    assert not np.array_equal(dirty.bits, c.dt.bits)
    assert _same(match_boundary(dirty, c.gt, H, W, d=d, return_iou=True, **c.kw)[0], want)


def test_segm_matching_is_as_it_was_beside_a_boundary_call():
    c, H, W, d, want, biou, seg = _want(("big", BI.BIG_SEEDS[0]), lambda: BI.big_random_set(BI.BIG_SEEDS[0]))
    assert _same(coco_eval.match(c.dt, c.gt, **c.kw), seg)
    _match_checks(c, H, W, d, want, biou)
    assert _same(coco_eval.match(c.dt, c.gt, **c.kw), seg)


def _block(rec, counts, cap):
    from mnc_amd.engine import _Ctx
    ctx = _Ctx(0)
    blk = InstanceBlock(types.SimpleNamespace(_ctx=ctx), 21, RI.S, 100, 300)
    assert blk.rows_cap >= cap
    head = np.zeros(HEAD_BYTES // 4, np.int32)
    head[:len(counts)] = counts
    raw = np.concatenate((head.view(np.uint8), np.ascontiguousarray(rec).reshape(-1).view(np.uint8)))
    _lib.call("mnc_h2d", ctx.h, blk.ptr, _lib.ptr(raw), raw.nbytes)
    return blk, ctx


def test_device_resident_result_gives_the_tables_of_its_host_copy():
    rng = np.random.default_rng(71)
    h, w = 70, 200
    list_mask, list_box = RI.class_lists(rng, w, h, 0.5)
    cap = 200
    rec, total = records_from_lists(list_mask, list_box, cap, RI.S)
    blk, ctx = _block(rec, [total] + [len(b) for b in list_box], cap)
    try:
        view = blk.view()
        flat = PackedMasks(**view.masks(h, w, score_thresh=0.0).fetch().arrays())
        gt = flat.take(np.arange(0, len(flat), 2))
        crowd = (np.arange(len(gt)) % 5 == 1).astype(np.uint8)
        pm = view.masks(h, w, score_thresh=0.0)
        assert "bits" not in pm._host and pm._device() is not None
        want, biou = match_boundary_numpy(flat, gt, h, w, crowd, d=2, return_iou=True)
        got, gb = pm.match_boundary(gt, h, w, crowd, d=2, return_iou=True)
        assert _same(got, want) and np.array_equal(gb, biou) and (want.dt_match[0, 0] >= 0).sum() >= len(gt) // 2
        assert _same_masks(pm.boundary(h, w, 2), boundary.boundary_numpy(flat, h, w, 2))
    finally:
        blk.release()
        ctx.close()


def test_evaluator_on_the_device_equals_the_host_s():
    dev, cpu = CocoSegmEval(device=True, iou_type="boundary"), CocoSegmEval(device=False, iou_type="boundary")
    sets = [BI.big_random_set(s)[:3] for s in BI.BIG_SEEDS] + [BI.frame(MM.RANDOM_SEEDS[0])]
    for i, (c, H, W) in enumerate(sets):
        for ev in (dev, cpu):
            ev.add(i, c.dt, c.gt, c.kw["iscrowd"], c.kw["ignore"], c.kw.get("eval_area"), image_size=(H, W))
    dev.summarize()
    cpu.summarize()
    assert dev.stats.dtype == np.float64 and dev.stats.shape == (12,) and np.array_equal(dev.stats, cpu.stats)
    assert np.array_equal(dev.eval["precision"], cpu.eval["precision"]) and np.array_equal(dev.eval["recall"], cpu.eval["recall"])
    assert 0 < cpu.stats[0] < 1


def test_eval_coco_boundary_on_the_gpu_prints_the_cpu_lines(tmp_path):
    gt, dt, _ = BI.coco_files(tmp_path)
    dev = BI.tool("--gt", gt, "--dt", dt, "--iou-type", "boundary")
    cpu = BI.tool("--gt", gt, "--dt", dt, "--iou-type", "boundary", "--cpu")
    assert dev.returncode == 0 and cpu.returncode == 0, (dev.stderr[-2000:], cpu.stderr[-2000:])
    assert dev.stdout == cpu.stdout and len([ln for ln in dev.stdout.splitlines() if ln.startswith(" Average")]) == 12
