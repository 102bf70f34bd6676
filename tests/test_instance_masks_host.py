"""Per-instance binary masks at image resolution, the host side (mnc_amd/masks.py, transform.mask_transform.instance_masks_numpy,
the argument checks of mnc_instance_masks): the numpy statement of the rule against an independent loop and against the
reference's own golden instance label map, the packed format's accessors, and the checks that need no GPU.  Exact everywhere."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import golden_inputs as GI  # noqa: E402
import render_inputs as RI  # noqa: E402  (sets up the reference-shaped import paths)
from mnc_amd import _lib  # noqa: E402
from mnc_amd.masks import PackedMasks, from_lists, instance_masks_call  # noqa: E402
from mnc_config import cfg  # noqa: E402
from transform.mask_transform import instance_masks_numpy  # noqa: E402
from utils.blob import resize_to  # noqa: E402
from utils.voc_eval import pack_sds_gt  # noqa: E402

S = RI.S


def _independent(box, mask, H, W, clip, thr):
    """-> (bounds, bool [h, w]): the rule written out once more, without the packed format."""
    b = np.round(np.asarray(box, np.float64)[:4]).astype(int)
    if clip:
        b = np.array(RI.rounded_box(box, W, H))
    return b, resize_to(np.asarray(mask, np.float32), b[2] - b[0] + 1, b[3] - b[1] + 1) >= np.float32(thr)


def _random_boxes(rng, n, H, W):
    out = []
    while len(out) < n:
        x = np.sort(rng.uniform(-9, W + 9, 2))
        y = np.sort(rng.uniform(-9, H + 9, 2))
        if len(out) % 5 == 0:                                # coordinates at x.5: half to even
            x, y = np.floor(x) + 0.5, np.floor(y) + 0.5
        # (a box wholly outside the image is one pixel wide or high once clipped: still valid)
        out.append([x[0], y[0], x[1], y[1]])
    return np.array(out)


@pytest.mark.parametrize("clip", [True, False])
def test_numpy_form_equals_an_independent_loop(clip):
    rng = np.random.default_rng(21 + clip)
    H, W = 60, 110
    boxes = _random_boxes(rng, 40, H, W)
    masks = np.stack([RI._mask(rng, int(rng.integers(0, 4))) for _ in range(len(boxes))])
    for thr in (cfg.BINARIZE_THRESH, 0.55):
        pm = instance_masks_numpy(boxes, masks, H, W, clip=clip, binarize_thresh=thr)
        assert len(pm) == len(boxes) and pm.bits.dtype == np.uint64
        nbytes = 0
        for i in range(len(boxes)):
            b, m = _independent(boxes[i], masks[i], H, W, clip, thr)
            assert np.array_equal(pm.bounds[i], b) and pm.offsets[i] == nbytes and pm.areas[i] == m.sum()
            assert pm.dense(i).dtype == bool and np.array_equal(pm.dense(i), m)
            nbytes += m.shape[0] * ((m.shape[1] + 63) // 64) * 8
        assert pm.bits.nbytes == nbytes
    if not clip:
        assert (pm.bounds[:, 0] < 0).any() and (pm.bounds[:, 2] > W - 1).any()      # bounds leave the image


def test_accessors_round_trip_on_both_sides_of_8_and_64():
    rng = np.random.default_rng(2)
    H, W = 40, 150
    widths = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129]
    boxes = np.array([[3.0, 2.0 + k, 3.0 + w - 1, 2.0 + k + (k % 4) * 6] for k, w in enumerate(widths)])
    masks = np.stack([RI._mask(rng, k % 4) for k in range(len(widths))])
    pm = instance_masks_numpy(boxes, masks, H, W, clip=True)
    gts = []
    for i, w in enumerate(widths):
        b, m = _independent(boxes[i], masks[i], H, W, True, cfg.BINARIZE_THRESH)
        assert pm.size(i) == m.shape and m.shape[1] == w
        assert np.array_equal(pm.dense(i), m)
        full = np.zeros((H, W), bool)
        full[b[1]:b[3] + 1, b[0]:b[2] + 1] = m
        assert np.array_equal(pm.full(i, H, W), full)
        rows = pm.as_sds_gt(i)
        assert rows.dtype == np.uint8 and np.array_equal(rows, np.packbits(m, axis=1, bitorder="little"))
        # padding bits of the 8-byte rows are zero: the words hold nothing but the mask
        words = pm.bits[pm.offsets[i] // 8:pm.offsets[i] // 8 + m.shape[0] * ((w + 63) // 64)]
        assert int(sum(bin(int(x)).count("1") for x in words)) == m.sum()
        gts.append({"mask_bound": b.astype(np.float64), "mask": m})
    # the project's ground-truth packing of the same masks: the same rows
    bounds, offsets, bits, areas, _ = pack_sds_gt(gts)
    assert np.array_equal(bounds, pm.bounds) and np.array_equal(areas, pm.areas)
    assert np.array_equal(bits, np.concatenate([pm.as_sds_gt(i).ravel() for i in range(len(pm))]))
    # unclipped bounds: full() keeps what lies inside the image
    out = instance_masks_numpy(np.array([[-6.0, -4.0, 20.0, 12.0], [140.0, 30.0, 160.0, 50.0]]), masks[:2], H, W, clip=False)
    for i in range(2):
        b, m = _independent([[-6.0, -4.0, 20.0, 12.0], [140.0, 30.0, 160.0, 50.0]][i], masks[i], H, W, False, cfg.BINARIZE_THRESH)
        canvas = np.zeros((H + 40, W + 40), bool)
        canvas[b[1] + 20:b[3] + 21, b[0] + 20:b[2] + 21] = m
        assert np.array_equal(out.full(i, H, W), canvas[20:20 + H, 20:20 + W])
    # the file form tools/demo.py --save-masks writes
    assert sorted(pm.arrays()) == sorted(PackedMasks.FIELDS)


def test_painting_the_masks_in_order_gives_the_references_instance_map():
    """The pin to the reference's own output: its _convert_pred_to_image paints instance i as i + 1, in list order."""
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_eval_outputs.npz"))
    case = GI.sds_case()
    for ii in (0, 3):
        H, W = case["images"][ii]["im"].shape[:2]
        pred = GI.vis_pred_dict(case, ii)
        pm = instance_masks_numpy(np.stack([np.asarray(b, np.float64) for b in pred["boxes"]]), np.stack(pred["masks"]), H, W,
                                  clip=True, classes=pred["cls_name"])
        assert len(pm) == len(pred["boxes"]) > 2 and np.array_equal(pm.classes, pred["cls_name"])
        inst = np.zeros((H, W), ref["vis_inst_%d" % ii].dtype)
        for i in range(len(pm)):
            inst[pm.full(i, H, W)] = i + 1
        assert np.array_equal(inst, ref["vis_inst_%d" % ii])


def test_from_lists_keeps_get_vis_dicts_rows():
    import demo
    rng = np.random.default_rng(4)
    list_mask, list_box = RI.class_lists(rng, 200, 120, 0.5)
    pred = demo.get_vis_dict(list_box, list_mask, "x", tuple("c%d" % i for i in range(1, 21)), 0.5)
    boxes, masks, classes = from_lists(list_mask, list_box, 0.5)
    assert len(boxes) == len(pred["boxes"]) > 3 and np.array_equal(classes, pred["cls_name"])
    assert np.array_equal(boxes, np.stack(pred["boxes"])) and np.array_equal(masks, np.stack(pred["masks"]))
    assert len(from_lists(list_mask, list_box, 0.0)[0]) == sum(len(b) for b in list_box)


def test_argument_checks_need_no_gpu():
    rng = np.random.default_rng(3)
    mk = np.stack([RI._mask(rng, 1) for _ in range(3)]).reshape(3, -1)
    good = np.array([[5.0, 6.0, 40.0, 50.0], [20.0, 10.0, 70.0, 30.0], [1.0, 1.0, 9.0, 9.0]])
    inverted = good.copy()
    inverted[1] = [50.0, 10.0, 10.0, 40.0]
    H, W = 60, 80
    # sizes alone: nothing is launched, so this runs without a device
    bounds, offsets, _, need = instance_masks_call(good, mk, 3, S, H, W, True, 0.4)
    want = instance_masks_numpy(good, mk.reshape(3, S, S), H, W)
    assert np.array_equal(bounds, want.bounds) and np.array_equal(offsets, want.offsets) and need == want.bits.nbytes
    assert instance_masks_call(good[:0], mk[:0], 0, S, H, W, True, 0.4, np.zeros(1, np.uint64))[3] == 0         # n == 0
    too_big = np.array([[0.0, 0.0, 9000.0, 9000.0]])
    for args in ((inverted, mk, 3, S, H, W, True), (inverted, mk, 3, S, H, W, False),
                 (good, np.zeros((3, 33 * 33), np.float32), 3, 33, H, W, True), (good, mk, 3, 0, H, W, True),
                 (good, mk, 3, S, 0, W, True), (good, mk, 3, S, H, 32769, True), (good * 2.0 ** 23, mk, 3, S, H, W, False),
                 (too_big, mk[:1], 1, S, H, W, False)):
        with pytest.raises(_lib.MncError) as e:
            instance_masks_call(*(args + (0.4, np.zeros(need // 8, np.uint64))))
        assert e.value.code == 1, args[2:]                                    # MNC_ERR_INVALID
    with pytest.raises(_lib.MncError) as e:                                   # a capacity that is too small
        instance_masks_call(good, mk, 3, S, H, W, True, 0.4, np.zeros(need // 8 - 1, np.uint64))
    assert e.value.code == 1 and "bits_cap" in str(e.value)
    # the numpy form refuses the same boxes and sizes
    for boxes, masks in ((inverted, mk.reshape(3, S, S)), (good, np.zeros((3, 33, 33), np.float32))):
        with pytest.raises(ValueError):
            instance_masks_numpy(boxes, masks, H, W)


def test_the_library_exports_the_three_entries():
    import mnc_amd.masks  # noqa: F401
    decls = _lib.parse_header()
    lib = _lib.load()
    for name in ("mnc_instance_masks", "mnc_mask_records", "mnc_net_masks"):
        assert name in decls and getattr(lib, name) is not None
    assert decls["mnc_instance_masks"][2][-1] == "device_id" and decls["mnc_mask_records"][2][-2:] == ["d_info", "d_bits"]
