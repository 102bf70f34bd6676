"""COCO run-length encoding of packed masks, the parts that need no GPU (mnc_amd/rle.py): the numpy statements of the counts and of
the way back, and the vectorised string codec against a literal transcription of maskApi.c's two loops.  Every comparison is
exact."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_rle_inputs as RI  # noqa: E402
from mnc_amd import rle  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402
from transform import mask_transform as MT  # noqa: E402


@pytest.mark.parametrize("rows, counts, string", RI.HAND)
def test_hand_cases(rows, counts, string):
    m = np.array(rows, bool)
    H, W = m.shape
    pm = RI.whole([m])
    run_ptr, runs = rle.rle_counts_numpy(pm, H, W)
    assert run_ptr.dtype == np.int64 and runs.dtype == np.uint32
    assert run_ptr.tolist() == [0, len(counts)] and runs.tolist() == counts
    assert RI.c_rle_to_string(counts) == string and RI.c_rle_fr_string(string) == counts      # the transcription itself
    assert rle.counts_to_string(counts) == string
    assert rle.string_to_counts(string).tolist() == counts and rle.string_to_counts(string.encode()).tolist() == counts
    assert rle.mask_rle_numpy(pm, H, W) == [{"size": [H, W], "counts": string}]
    back = rle.masks_from_rle_numpy([{"size": [H, W], "counts": string}])
    assert np.array_equal(back.full(0, H, W), m)


def _codec_cases():
    rng = np.random.default_rng(5)
    cases = [[0], [7], [5, 9], [5, 9, 11], [2 ** 30], [0, 2 ** 30], [2 ** 25, 2 ** 25 + 3, 2 ** 26, 1, 2 ** 29]]
    # the differences -1, -16, -17, 15, 16 (and their neighbours) at the fourth entry and later
    for d in (-1, -16, -17, 15, 16, -15, 17, -32, 31, 32, -33, 0, -1024, 1023, 1024):
        cases.append([3, 3000, 5000, 3000 + d, 5000 + d, 3000 + 2 * d])
    for _ in range(30):
        n = int(rng.integers(1, 40))
        scale = rng.choice([4, 40, 2 ** 10, 2 ** 20, 2 ** 26, 2 ** 30])
        cases.append(rng.integers(0, scale + 1, n).tolist())
    return cases


def test_codec_equals_the_c_loops():
    long_entries = 0
    for counts in _codec_cases():
        want = RI.c_rle_to_string(counts)
        assert rle.counts_to_string(counts) == want, counts
        assert rle.counts_to_string(np.array(counts, np.uint32)) == want
        assert RI.c_rle_fr_string(want) == counts
        got = rle.string_to_counts(want)
        assert got.dtype == np.uint32 and got.tolist() == counts, counts
        long_entries += len(want) >= 6 * len(counts)
    assert long_entries >= 2                                                   # values >= 2^25 take six or seven characters
    assert len(RI.c_rle_to_string([2 ** 30])) == 7 and len(RI.c_rle_to_string([2 ** 25])) == 6
    assert rle.counts_to_string([]) == "" and rle.string_to_counts("").tolist() == []
    for bad in ("P", "0\x7f", "/"):                                            # ends inside an entry; characters outside the code
        with pytest.raises(ValueError):
            rle.string_to_counts(bad)


@pytest.mark.parametrize("H, W", [(1, 1), (1, 65), (63, 1), (64, 64), (65, 129), (129, 63)])
def test_numpy_statement_on_clipped_sets(H, W):
    pm = RI.size_set(H, W)
    run_ptr, runs = rle.rle_counts_numpy(pm, H, W)
    assert run_ptr[0] == 0 and len(runs) == run_ptr[-1]
    for i in range(len(pm)):
        c = runs[run_ptr[i]:run_ptr[i + 1]].astype(np.int64)
        assert c.sum() == H * W and c[1::2].sum() == pm.areas[i] and (c[1:] > 0).all()
    assert runs[run_ptr[3]:run_ptr[4]].tolist() == [H * W] and runs[run_ptr[4]:run_ptr[5]].tolist() == [0, H * W]
    back = rle.masks_from_counts_numpy(run_ptr, runs, H, W)
    assert np.array_equal(back.areas, pm.areas) and back.bounds[3].tolist() == [0, 0, -1, -1] and back.size(3) == (0, 0)
    assert (back.offsets % 8 == 0).all() and back.offsets[0] == 0
    for i in range(len(pm)):
        assert np.array_equal(back.full(i, H, W), pm.full(i, H, W))
        if pm.areas[i]:
            ys, xs = np.nonzero(pm.full(i, H, W))
            assert back.bounds[i].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]
    again = rle.rle_counts_numpy(back, H, W)
    assert np.array_equal(again[0], run_ptr) and np.array_equal(again[1], runs)
    assert all(np.array_equal(a, b) for a, b in zip(MT.rle_counts_numpy(pm, H, W), (run_ptr, runs)))


def test_numpy_statement_on_bounds_that_leave_the_image():
    H, W = 70, 200
    pm, dirty = RI.leaving(H, W), RI.leaving(H, W, dirty=True)
    run_ptr, runs = rle.rle_counts_numpy(pm, H, W)
    for i in range(len(pm)):
        c = runs[run_ptr[i]:run_ptr[i + 1]].astype(np.int64)
        assert c.sum() == H * W and c[1::2].sum() == pm.full(i, H, W).sum()
    assert [runs[run_ptr[i]:run_ptr[i + 1]].tolist() for i in (5, 9, 10, 11)] == [[H * W]] * 4
    got = rle.rle_counts_numpy(dirty, H, W)
    assert np.array_equal(got[0], run_ptr) and np.array_equal(got[1], runs)
    back = MT.masks_from_counts_numpy(run_ptr, runs, H, W)
    assert all(np.array_equal(back.full(i, H, W), pm.full(i, H, W)) for i in range(len(pm)))


def test_numpy_statement_on_low_masks_on_the_last_rows():
    H, W = 65, 140
    sets = RI.bottom_rows(H, W)
    run_ptr, runs = rle.rle_counts_numpy(sets[0], H, W)
    assert run_ptr.tolist() == [0, 23] and runs.tolist() == [10 * H + H - 1] + [1, H - 1] * 10 + [1, (W - 21) * H]
    for pm in sets:
        run_ptr, runs = rle.rle_counts_numpy(pm, H, W)
        back = rle.masks_from_counts_numpy(run_ptr, runs, H, W)
        assert all(np.array_equal(back.full(i, H, W), pm.full(i, H, W)) for i in range(len(pm)))


def test_zero_length_runs_decode_and_reencode_canonically():
    H, W = 5, 4
    canonical = [3, 4, 6, 7]                                                   # 20 pixels
    loose = [0, 0, 3, 2, 0, 2, 6, 0, 0, 7, 0]                                  # the same pixels, with runs of length 0
    a = rle.masks_from_counts_numpy([0, len(canonical)], canonical, H, W)
    b = rle.masks_from_counts_numpy([0, len(loose)], loose, H, W)
    assert np.array_equal(a.full(0, H, W), b.full(0, H, W)) and a.areas[0] == b.areas[0] == 11
    assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in PackedMasks.FIELDS)
    assert rle.rle_counts_numpy(b, H, W)[1].tolist() == canonical
    lead = rle.masks_from_counts_numpy([0, 2], [0, 20], H, W)
    assert lead.bounds[0].tolist() == [0, 0, 3, 4] and rle.rle_counts_numpy(lead, H, W)[1].tolist() == [0, 20]


def test_argument_checks_that_need_no_gpu():
    with pytest.raises(ValueError):
        rle.masks_from_counts_numpy([0, 2], [3, 4], 2, 4)                      # sums to 7, not 8
    with pytest.raises(ValueError):
        rle.masks_from_counts_numpy([0, 2], [3, 6], 2, 4)                      # ... to 9
    with pytest.raises(ValueError):
        rle.masks_from_counts_numpy([0, 0], [], 2, 4)                          # a mask without counts
    with pytest.raises(ValueError):
        rle.masks_from_counts_numpy([2, 1], [8, 8], 2, 4)                      # a decreasing run_ptr
    with pytest.raises(ValueError):
        rle.masks_from_counts_numpy([0, 1], [0], 0, 4)
    with pytest.raises(ValueError):
        rle.rle_counts_numpy(RI.size_set(3, 3), 3, 32769)
    mixed = [{"size": [2, 4], "counts": "8"}, {"size": [4, 2], "counts": "8"}]
    with pytest.raises(ValueError):
        rle.counts_of_rles(mixed)
    with pytest.raises(ValueError):
        PackedMasks.from_rle(mixed)                                            # refused before the library is looked for
    with pytest.raises(ValueError):
        rle.counts_of_rles([{"size": [2, 4], "counts": [9, -1]}])
    run_ptr, runs, H, W = rle.counts_of_rles([{"size": [2, 4], "counts": "8"}, {"size": [2, 4], "counts": b"26"},
                                              {"size": [2, 4], "counts": [0, 8]}])
    assert (H, W) == (2, 4) and run_ptr.tolist() == [0, 1, 3, 5] and runs.tolist() == [8, 2, 6, 0, 8]
    assert all(hasattr(MT, name) for name in ("mask_rle", "masks_from_rle", "rle_counts_numpy", "masks_from_counts_numpy"))


def test_demo_coco_entries_from_the_numpy_statement():
    import demo
    H, W = 70, 200
    pm = RI.mixed()
    entries = demo._coco_results("im0", (H, W, 3), pm, cpu=True)
    assert len(entries) == len(pm) and set(entries[0]) == {"image_id", "category_id", "segmentation", "bbox", "score"}
    strings = rle.mask_rle_numpy(pm, H, W)
    for i, e in enumerate(entries):
        assert e["image_id"] == "im0" and e["category_id"] == pm.classes[i] and e["score"] == float(pm.scores[i])
        assert e["segmentation"] == strings[i]
        ys, xs = np.nonzero(pm.full(i, H, W))
        assert e["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]      # the tight box of the pixels
    none = demo._coco_results("im0", (H, W, 3), RI.whole([np.zeros((H, W), bool)]), cpu=True)
    assert none[0]["bbox"] == [0, 0, 0, 0] and none[0]["segmentation"]["counts"] == rle.counts_to_string([H * W])
