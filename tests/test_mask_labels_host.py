"""The numpy statements of mnc_amd.labels (from_labels_numpy, to_labels_numpy and the panoptic helpers) against facts that do not come
from them: scipy.ndimage.find_objects, np.bincount, label[box] == id through PackedMasks.from_dense, utils.voc_eval.parse_inst on
.mat files in SBD's nesting, the backward painting loop written out bit by bit, the two round trips -- the second one through the
statements of mnc_amd.algebra -- and the tools that write the formats.  No GPU is needed or touched."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import mask_algebra_inputs as AI  # noqa: E402
import mask_labels_inputs as LI  # noqa: E402
from mnc_amd import labels as LB  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

ALL_MAPS = sorted(LI.MAPS)


@pytest.mark.parametrize("name", ALL_MAPS)
def test_from_labels_against_find_objects_bincount_and_from_dense(name):
    from scipy import ndimage
    label = LI.get(name)
    pm, ids = LI.from_ref(name)
    assert ids.dtype == np.int32 and np.array_equal(ids, np.setdiff1d(np.unique(label), [0]))
    slices = ndimage.find_objects(label)
    counts = np.bincount(label.reshape(-1))
    bounds, dense = [], []
    for i in ids:
        sy, sx = slices[int(i) - 1]
        bounds.append([sx.start, sy.start, sx.stop - 1, sy.stop - 1])
        dense.append(label[sy, sx] == i)
    assert np.array_equal(pm.areas, counts[ids])
    want = PackedMasks.from_dense(np.array(bounds, np.int32).reshape(-1, 4), dense)
    assert AI.same_masks(pm, want) and AI.canonical(pm)
    assert not pm.scores.any() and not pm.classes.any()


def test_background_forms_and_classes():
    label = LI.get("full_row")
    every, ids = LB.from_labels_numpy(label, background=None)
    assert ids[0] == 0 and len(every) == len(LI.from_ref("full_row")[0]) + 1 and every.areas.sum() == label.size
    voc = label.copy()
    voc[0, :5] = 255
    pm, ids = LB.from_labels_numpy(voc, background=(0, 255))
    assert 255 not in ids and 0 not in ids and np.array_equal(ids, np.setdiff1d(np.unique(voc), [0, 255]))
    none, ids = LB.from_labels_numpy(np.zeros((3, 70), np.int32))
    assert len(none) == 0 and ids.shape == (0,) and none.bits.size == 0
    inst, cls = LI.class_maps()
    pm, ids = LB.from_labels_numpy(inst, cls)
    assert [int(c) for c in pm.classes] == [(int(i) * 7) % 20 + 1 for i in ids]
    table = {int(i): int(i) + 100 for i in ids}
    assert np.array_equal(LB.from_labels_numpy(inst, classes=table)[0].classes, ids + 100)
    assert np.array_equal(LB.from_labels_numpy(inst, classes=np.arange(int(ids.max()) + 1) * 2)[0].classes, ids * 2)
    del table[int(ids[1])]
    with pytest.raises(ValueError, match="no entry for id %d" % ids[1]):
        LB.from_labels_numpy(inst, classes=table)


def test_refusals():
    assert len(LB.from_labels_numpy(LI.labels_2048())[0]) == 2048
    with pytest.raises(ValueError, match="2049 instances"):
        LB.from_labels_numpy(LI.get("labels_2049"))
    with pytest.raises(ValueError, match="%d instances" % LI.SUPERPIXEL_LABELS):
        LB.from_labels_numpy(LI.get("superpixels"))
    assert len(LI.from_ref("superpixels_part")[0]) == 1659
    big = np.zeros((2, 3), np.int64)
    big[1, 1] = 2 ** 24
    with pytest.raises(ValueError, match="16777216"):
        LB.from_labels_numpy(big)
    big[1, 1] = -1
    with pytest.raises(ValueError, match="-1"):
        LB.from_labels_numpy(big)
    inst, cls, first = LI.mixed_class_maps()
    with pytest.raises(ValueError, match="instance %d has" % first):
        LB.from_labels_numpy(inst, cls)
    with pytest.raises(ValueError):
        LB.from_labels_numpy(np.zeros((0, 5), np.int32))
    with pytest.raises(ValueError):
        LB.from_labels_numpy(np.zeros((1, 32769), np.int32))
    with pytest.raises(ValueError):
        LB.from_labels_numpy(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        LB.from_labels_numpy(np.zeros((4, 4), np.int32), background=range(9))
    with pytest.raises(ValueError):
        LB.to_labels_numpy(AI.get("equal"), 10, 10, order=[0, 0, 1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError):
        LB.to_labels_numpy(AI.get("equal"), 10, 10, values=[1, 2])


def _write_sbd(devkit, name, inst, cls):
    import scipy.io as sio
    os.makedirs(os.path.join(devkit, "inst"), exist_ok=True)
    os.makedirs(os.path.join(devkit, "cls"), exist_ok=True)
    sio.savemat(os.path.join(devkit, "inst", name + ".mat"), {"GTinst": {"Segmentation": inst.astype(np.uint8)}})
    sio.savemat(os.path.join(devkit, "cls", name + ".mat"), {"GTcls": {"Segmentation": cls.astype(np.uint8)}})


def _devkit(tmp_path):
    devkit = str(tmp_path / "sbd")
    inst, cls = LI.class_maps()
    _write_sbd(devkit, "2008_000001", inst, cls)
    _write_sbd(devkit, "2008_000002", inst[::-1, ::-1].copy(), cls[::-1, ::-1].copy())
    with open(os.path.join(devkit, "val.txt"), "w") as f:
        f.write("2008_000001\n2008_000002\n")
    return devkit


def test_parse_inst_maps_against_parse_inst(tmp_path):
    import scipy.io as sio
    from utils.voc_eval import parse_inst, parse_inst_maps
    devkit = _devkit(tmp_path)
    for name in ("2008_000001", "2008_000002"):
        want = parse_inst(name, devkit)
        inst = sio.loadmat(os.path.join(devkit, "inst", name + ".mat"))["GTinst"]["Segmentation"][0][0]
        cls = sio.loadmat(os.path.join(devkit, "cls", name + ".mat"))["GTcls"]["Segmentation"][0][0]
        got = parse_inst_maps(inst, cls)
        assert len(got) == len(want) == 9
        for g, w in zip(got, want):
            assert sorted(g) == sorted(w)
            for key in w:
                a, b = np.asarray(g[key]), np.asarray(w[key])
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), key


SETS = sorted(LI.sets())


@pytest.mark.parametrize("name", SETS)
def test_to_labels_against_the_painting_loop(name):
    pm, H, W = LI.sets()[name]
    n = len(pm)
    from mnc_amd.algebra import score_order
    rng = np.random.default_rng(7)
    cases = [(None, None, 0), (pm.classes, None, -3)]
    if n:
        cases.append((rng.integers(-2 ** 31, 2 ** 31, n), rng.permutation(n), 2 ** 31 - 1))
    for values, order, background in cases:
        got = LB.to_labels_numpy(pm, H, W, values, order, background)
        want = LI.paint(pm, H, W, np.arange(1, n + 1) if values is None else values,
                        score_order(pm.scores) if order is None else order, background)
        assert got.dtype == np.int32 and got.shape == (H, W) and np.array_equal(got, want)


@pytest.mark.parametrize("name", ALL_MAPS)
def test_round_trip_from_a_map(name):
    label = LI.get(name)
    pm, ids = LI.from_ref(name)
    back = LB.to_labels_numpy(pm, label.shape[0], label.shape[1], values=ids, order=np.arange(len(pm)))
    assert np.array_equal(back[label != 0], label[label != 0]) and not back[label == 0].any()


@pytest.mark.parametrize("name,size", [("blobs", LI.BLOBS_SIZE), ("edge", LI.EDGE_SIZE)])
def test_round_trip_from_a_set(name, size):
    pm = AI.get(name)
    pm = pm[0] if isinstance(pm, tuple) else pm
    H, W = size
    assert (pm.bounds[:, 0] < 0).any() and (pm.bounds[:, 2] >= W).any() and (pm.bounds[:, 3] >= H).any()   # instances cross the edge
    seg = LB.to_labels_numpy(pm, H, W)
    got, ids = LB.from_labels_numpy(seg, classes={i + 1: int(c) for i, c in enumerate(pm.classes)})
    want, kept = LI.disjoint_ref(pm, H, W)
    assert len(kept) == LI.SURVIVORS[name] and len(pm) in (300, 1025) and np.array_equal(ids, kept + 1)
    for f in ("bounds", "offsets", "areas", "classes", "bits"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
    assert np.array_equal(np.bincount(seg.reshape(-1), minlength=len(pm) + 1)[1:][kept], want.areas)
    assert np.bincount(seg.reshape(-1), minlength=len(pm) + 1)[1:].sum() == want.areas.sum()


def test_panoptic_ids_and_segments_info():
    for x in (0, 255, 256, 65536, 2 ** 24 - 1):
        rgb = LB.id_to_rgb(x)
        assert rgb.dtype == np.uint8 and rgb.shape == (3,) and int(LB.rgb_to_id(rgb)) == x
    assert LB.id_to_rgb(np.array([[1, 256], [65536, 65793]])).tolist() == [[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 1, 1]]]
    with pytest.raises(ValueError):
        LB.id_to_rgb(2 ** 24)
    inst, cls = LI.class_maps()
    pm, ids = LB.from_labels_numpy(inst, cls)
    info = LB.segments_info(pm, ids)
    assert [s["id"] for s in info] == ids.tolist() and all(s["iscrowd"] == 0 for s in info)
    for k, s in enumerate(info):
        x, y, w, h = s["bbox"]
        assert s["area"] == int((inst == ids[k]).sum()) == int((inst[y:y + h, x:x + w] == ids[k]).sum())
        assert s["category_id"] == int(cls[inst == ids[k]][0])


def test_sbd_to_coco_is_read_by_eval_coco(tmp_path):
    import eval_coco
    import sbd_to_coco
    from mnc_amd import rle
    devkit, out = _devkit(tmp_path), str(tmp_path / "gt.json")
    sbd_to_coco.main(["--devkit", devkit, "--image-set", os.path.join(devkit, "val.txt"), "--out", out, "--cpu"])
    with open(out) as f:
        gt = json.load(f)
    assert [im["id"] for im in gt["images"]] == ["2008_000001", "2008_000002"] and len(gt["categories"]) == 20
    assert [a["id"] for a in gt["annotations"]] == list(range(1, 19)) and all(a["iscrowd"] == 0 for a in gt["annotations"])
    inst, cls = LI.class_maps()
    want, _ = LB.from_labels_numpy(inst, cls)
    first = [a for a in gt["annotations"] if a["image_id"] == "2008_000001"]
    run_ptr, runs, _, _ = rle.counts_of_rles([a["segmentation"] for a in first])
    back = rle.masks_from_counts_numpy(run_ptr, runs, inst.shape[0], inst.shape[1], [a["category_id"] for a in first], np.zeros(9))
    assert AI.same_masks(back, want)
    assert [a["area"] for a in first] == want.areas.tolist()
    assert [a["bbox"] for a in first] == [[int(b[0]), int(b[1]), int(b[2] - b[0] + 1), int(b[3] - b[1] + 1)] for b in want.bounds]
    # the ground truth scored against itself through eval_coco's own loader: every instance is found
    results = [{"image_id": a["image_id"], "category_id": a["category_id"], "segmentation": a["segmentation"], "score": 0.9}
               for a in gt["annotations"]]
    ev = eval_coco.evaluate(gt, results, cpu=True)
    assert ev.stats[0] == 1.0


def test_panoptic_png_decodes_to_the_label_map(tmp_path):
    from PIL import Image
    import demo
    pm, H, W = LI.sets()["equal"]
    entry = demo._save_panoptic(str(tmp_path), "im", (H, W, 3), pm, cpu=True)
    png = np.asarray(Image.open(str(tmp_path / "im.png")).convert("RGB"))
    want = LB.to_labels_numpy(pm, H, W)
    assert np.array_equal(LB.rgb_to_id(png), want)
    assert entry["file_name"] == "im.png" and [s["id"] for s in entry["segments_info"]] == sorted(set(want.reshape(-1).tolist()) - {0})
    assert [s["area"] for s in entry["segments_info"]] == [int((want == s["id"]).sum()) for s in entry["segments_info"]]
