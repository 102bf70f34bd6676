"""The contingency table of two label maps on the GPU (csrc/label_pairs.hip: mnc_label_pairs and the Python surfaces over it --
pairs.label_pairs, pairs.confusion, panoptic.pq_image, PanopticEval) against the numpy statements of mnc_amd.pairs and
mnc_amd.panoptic, which tests/test_label_pairs_host.py pins to scikit-learn, np.bincount, a double loop and a brute force.  Every
comparison is exact, field by field, dtype and shape included.  The maps are those of tests/label_pairs_inputs.py: the smallest at
which a kernel can go wrong."""
import ctypes
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
from mnc_amd import _lib  # noqa: E402
from mnc_amd import pairs as PR  # noqa: E402
from mnc_amd import panoptic as PQ  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY32 = np.int32(0x55555555)
CANARY64 = np.int64(0x5555555555555555)


class GlobalPlan(object):
    """mnc_label_pairs_plan(1) while it is open: every table is counted in device memory."""

    def __enter__(self):
        PR.plan(True)

    def __exit__(self, *exc):
        PR.plan(False)


def raw(a, b, cap_ids, cap_pairs):
    """mnc_label_pairs as it is, on canary-filled outputs -> (status, na, nb, m, a_ids, b_ids, ia, ib, count, message)."""
    a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    H, W = a.shape
    a_ids, b_ids = np.full(max(cap_ids, 1), CANARY32), np.full(max(cap_ids, 1), CANARY32)
    ia, ib, count = np.full(max(cap_pairs, 1), CANARY32), np.full(max(cap_pairs, 1), CANARY32), np.full(max(cap_pairs, 1), CANARY64)
    na, nb, m = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    lib = _lib.load()
    rc = lib.mnc_label_pairs(_lib.ptr(a), _lib.ptr(b), H, W, cap_ids, cap_pairs, ctypes.addressof(na), _lib.ptr(a_ids),
                             ctypes.addressof(nb), _lib.ptr(b_ids), ctypes.addressof(m), _lib.ptr(ia), _lib.ptr(ib), _lib.ptr(count), 0)
    return rc, na.value, nb.value, m.value, a_ids, b_ids, ia, ib, count, lib.mnc_last_error().decode()


def untouched(r):
    return all((arr == CANARY32).all() for arr in r[4:8]) and (r[8] == CANARY64).all()


# ---- the table ----

@pytest.mark.parametrize("name", sorted(PI.CASES))
def test_label_pairs_equals_the_statement(name):
    """Widths 1, 63, 64, 65, 130 and heights 1, 2, 65; totals of 201, 1027 and 7 pixels; values 31 / 32 / 33 and 2^24 - 1 in either
    map; a run across lanes, waves and workgroups; runs of length one; 2^20 pixels of one pair; 128 x 128 and 128 x 129 cells; tables
    of one row and one column; non-zero cells on both sides of cell 65536; 2^22 cells; the blobs, the edge set, superpixels."""
    a, b = PI.get(name)
    got, want = PR.label_pairs(a, b), PI.reference(name)
    assert PI.same_pairs(got, want)
    if name == "one_pair":
        assert got.count.tolist() == [2 ** 20] and got.a_ids.tolist() == [3] and got.b_ids.tolist() == [9]
    if name == "lds_exact":
        assert got.a_ids.size * got.b_ids.size == PR.LDS_CELLS == len(got)
    if name == "lds_above":
        assert got.a_ids.size * got.b_ids.size == PR.LDS_CELLS + 128 and len(got) == PR.LDS_CELLS + 1
    if name == "straddle":
        cells = got.ia.astype(np.int64) * got.b_ids.size + got.ib
        assert 65535 in cells and 65536 in cells and got.b_ids.size == 300
    if name == "most_cells":
        assert got.a_ids.size * got.b_ids.size == 2 ** 22


@pytest.mark.parametrize("name", ["one_pair", "lds_exact", "long_runs", "alternating", "size_65x130", "one_row", "one_column", "tail_3x67"])
def test_the_two_plans_give_the_same_integers(name):
    """Tables of at most LDS_CELLS cells, counted in device memory instead."""
    a, b = PI.get(name)
    want = PI.reference(name)
    assert want.a_ids.size * want.b_ids.size <= PR.LDS_CELLS
    with GlobalPlan():
        got = PR.label_pairs(a, b)
    assert PI.same_pairs(got, want)
    assert _lib.load().mnc_label_pairs_plan(2) == INVALID and PI.same_pairs(PR.label_pairs(a, b), want)


def test_two_runs_give_the_same_bytes():
    for name in ("one_pair", "most_cells", "superpixels"):
        a, b = PI.get(name)
        first, second = PR.label_pairs(a, b), PR.label_pairs(a, b)
        for f in PR.LabelPairs.FIELDS:
            assert getattr(first, f).tobytes() == getattr(second, f).tobytes()


def test_other_dtypes():
    a, b = PI.get("size_2x65")
    for dtype in (np.uint8, np.uint16, np.int64):
        assert PI.same_pairs(PR.label_pairs(a.astype(dtype), b.astype(np.int64)), PI.reference("size_2x65"))
    with pytest.raises(ValueError, match=r"not in \[0, 16777216\)"):
        PR.label_pairs(a.astype(np.int64) + 2 ** 32, b)              # (refused before the cast, which would wrap it into range)


# ---- refusals ----

def test_one_id_past_the_cells_is_refused_with_the_numbers():
    a, b = PI.get("most_cells_plus_one")
    with pytest.raises(ValueError, match="2048 x 2049.*4196352"):
        PR.label_pairs(a, b)
    r = raw(a, b, 65536, a.size)
    assert r[0] == INVALID and (r[1], r[2], r[3]) == (2048, 2049, -7) and untouched(r) and "4196352" in r[9]
    ids = np.arange(65540, dtype=np.int32).reshape(4, 16385)
    with pytest.raises(ValueError, match="65540 and 1 distinct values"):
        PR.label_pairs(ids, np.zeros_like(ids))
    r = raw(PI.get("size_2x65")[0], PI.get("size_2x65")[1], 3, 130)       # cap_ids below the values of a
    want = PI.reference("size_2x65")
    assert r[0] == INVALID and (r[1], r[2]) == (want.a_ids.size, want.b_ids.size) and untouched(r)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("value", [-1, 2 ** 24, -2 ** 31, 2 ** 31 - 1])
def test_a_value_out_of_range_is_refused_and_nothing_is_written(which, value):
    a, b = (m.copy() for m in PI.get("size_65x130"))
    (a if which == "a" else b)[64, 129] = value
    r = raw(a, b, 65536, a.size)
    assert r[0] == INVALID and (r[1], r[2], r[3]) == (-7, -7, -7) and untouched(r)
    assert "%s[64][129]=%d not in [0, 16777216)" % (which, value) in r[9]
    with pytest.raises(ValueError, match=r"\[64\]\[129\]=%d not in \[0, 16777216\)" % value):
        PR.label_pairs(a, b)


def test_cap_pairs_one_short_is_refused_with_the_number():
    a, b = PI.get("size_65x130")
    want = PI.reference("size_65x130")
    r = raw(a, b, 64, len(want) - 1)
    assert r[0] == INVALID and (r[1], r[2], r[3]) == (want.a_ids.size, want.b_ids.size, len(want)) and untouched(r)
    r = raw(a, b, 64, len(want))
    assert r[0] == 0 and r[3] == len(want) and np.array_equal(r[8][:len(want)], want.count) and np.array_equal(r[6][:len(want)], want.ia)
    assert np.array_equal(r[4][:r[1]], want.a_ids) and (r[4][r[1]:] == CANARY32).all() and (r[5][r[2]:] == CANARY32).all()


def test_what_the_host_refuses_before_any_launch():
    a, b = PI.get("size_2x65")
    lib = _lib.load()
    na, nb, m = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    out = [np.full(200, CANARY32) for _ in range(4)] + [np.full(200, CANARY64)]
    ids_a, ids_b, ia, ib, cnt = (_lib.ptr(o) for o in out)
    P = ctypes.addressof
    calls = {
        "null a": (None, _lib.ptr(b), 2, 65, 200, 200, P(na), ids_a, P(nb), ids_b, P(m), ia, ib, cnt, 0),
        "null b": (_lib.ptr(a), None, 2, 65, 200, 200, P(na), ids_a, P(nb), ids_b, P(m), ia, ib, cnt, 0),
        "null na": (_lib.ptr(a), _lib.ptr(b), 2, 65, 200, 200, None, ids_a, P(nb), ids_b, P(m), ia, ib, cnt, 0),
        "null n_pairs": (_lib.ptr(a), _lib.ptr(b), 2, 65, 200, 200, P(na), ids_a, P(nb), ids_b, None, ia, ib, cnt, 0),
        "null count": (_lib.ptr(a), _lib.ptr(b), 2, 65, 200, 200, P(na), ids_a, P(nb), ids_b, P(m), ia, ib, None, 0),
        "null ids": (_lib.ptr(a), _lib.ptr(b), 2, 65, 200, 200, P(na), None, P(nb), ids_b, P(m), ia, ib, cnt, 0),
        "H 0": (_lib.ptr(a), _lib.ptr(b), 0, 65, 200, 200, P(na), ids_a, P(nb), ids_b, P(m), ia, ib, cnt, 0),
        "W past the side": (_lib.ptr(a), _lib.ptr(b), 1, 32769, 200, 200, P(na), ids_a, P(nb), ids_b, P(m), ia, ib, cnt, 0),
        "too many pixels": (_lib.ptr(a), _lib.ptr(b), 32768, 32768, 200, 200, P(na), ids_a, P(nb), ids_b, P(m), ia, ib, cnt, 0),
        "cap_ids < 0": (_lib.ptr(a), _lib.ptr(b), 2, 65, -1, 200, P(na), ids_a, P(nb), ids_b, P(m), ia, ib, cnt, 0),
        "cap_pairs < 0": (_lib.ptr(a), _lib.ptr(b), 2, 65, 200, -1, P(na), ids_a, P(nb), ids_b, P(m), ia, ib, cnt, 0),
    }
    for what, args in calls.items():
        assert lib.mnc_label_pairs(*args) == INVALID, what
        assert (na.value, nb.value, m.value) == (-7, -7, -7), what
        assert all((o == (CANARY64 if o.dtype == np.int64 else CANARY32)).all() for o in out), what
    with pytest.raises(ValueError, match="shape"):
        PR.label_pairs(a, b[:, :-1])


# ---- the tie to the existing kernels ----

@pytest.mark.parametrize("name", ["blobs", "edge"])
def test_overlaps_of_the_instances_are_the_table_without_its_background(name):
    a, b = PI.get(name)
    assert (a == 0).any() and (b == 0).any()
    t = PR.label_pairs(a, b)
    assert t.a_ids[0] == 0 and t.b_ids[0] == 0
    inter, _ = PackedMasks.from_labels(a)[0].overlaps(PackedMasks.from_labels(b)[0])
    assert inter.dtype == np.int64 and np.array_equal(inter, t.dense()[1:, 1:])


# ---- the scores ----

def test_confusion_equals_its_numpy_form():
    gt, pred = PI.class_pair()
    got, want = PR.confusion(gt, pred, 21), PR.confusion(gt, pred, 21, device=False)
    assert got.dtype == want.dtype == np.int64 and got.shape == want.shape == (21, 21) and np.array_equal(got, want)
    assert PR.semantic_scores(got) == PR.semantic_scores(want)
    assert np.array_equal(PR.confusion(gt.astype(np.uint8), pred.astype(np.uint8), 21), want)
    with pytest.raises(ValueError, match="gt value 255"):
        PR.confusion(gt, pred, 21, ignore=None)


@pytest.mark.parametrize("seed", range(6))
def test_pq_image_equals_its_numpy_form(seed):
    scene = PI.random_scene(seed)
    assert PQ.pq_image(*(scene + (PI.CATEGORIES,))) == PQ.pq_image_numpy(*(scene + (PI.CATEGORIES,)))
    assert PQ.pq_image(*(scene + (PI.CATEGORIES,)), device=False) == PQ.pq_image_numpy(*(scene + (PI.CATEGORIES,)))


def test_panoptic_eval_equals_its_numpy_form():
    dev, host = PQ.PanopticEval(PI.CATEGORIES), PQ.PanopticEval(PI.CATEGORIES, device=False)
    for k in range(6):
        assert dev.add(k, *PI.random_scene(k)) == host.add(k, *PI.random_scene(k))
    assert dev.summarize() == host.summarize() and dev.lines() == host.lines()
    a, b = PI.get("blobs")                                               # a scene of 245 segments a side
    cats = {c: {"isthing": int(c < 15)} for c in range(1, 21)}
    gs = [PI.seg(i, i % 20 + 1, int(i % 17 == 0)) for i in np.unique(a) if i]
    ps = [PI.seg(i, i % 20 + 1) for i in np.unique(b) if i]
    assert PQ.pq_image(a, gs, b, ps, cats) == PQ.pq_image_numpy(a, gs, b, ps, cats)


def test_a_written_panoptic_result_scores_one_against_itself(tmp_path):
    """pm.to_labels through tools/demo.py --save-panoptic's writer, back through tools/eval_panoptic.py's reader."""
    import demo
    import eval_panoptic
    pm, H, W = LI.sets()["equal"]
    pm = pm.take(np.arange(len(pm)))
    pm.classes[:] = np.arange(len(pm)) % 20 + 1
    entry = demo._save_panoptic(str(tmp_path), "im", (H, W, 3), pm)
    path = str(tmp_path / "panoptic.json")
    with open(path, "w") as f:
        json.dump({"annotations": [entry], "categories": [{"id": k + 1, "name": "c%d" % k, "isthing": 1} for k in range(20)]}, f)
    maps, _ = eval_panoptic.read_panoptic(path, str(tmp_path))
    assert np.array_equal(maps["im"][0], pm.to_labels(H, W))
    ev = eval_panoptic.evaluate(path, str(tmp_path), path, str(tmp_path))
    out = ev.summarize()
    assert out["All"]["pq"] == out["All"]["sq"] == out["All"]["rq"] == 1.0 and out["All"]["n"] >= 1
    assert out == eval_panoptic.evaluate(path, str(tmp_path), path, str(tmp_path), cpu=True).summarize()
