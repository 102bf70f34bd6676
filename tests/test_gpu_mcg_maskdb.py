"""The MCG proposal maskdb on the GPU (csrc/mcg_maskdb.hip, mnc_mcg_maskdb, db/mcg_maskdb.py:mcg_maskdb_device): bit for bit what
the REFERENCE'S OWN tools/prepare_mcg_maskdb.py wrote (tests/golden/reference_mcg_maskdb.npz), equality with the numpy form on a
VOC-sized random image and on the engineered edge cases at three mask sizes, the statuses the call reports, the tool, and
`--task cfm` end to end from a tool-written maskdb and from cfg.TEST.MCG_RAW_DIR alone.  Integers and exact doubles: there is no
tolerance anywhere.  Every GPU step runs in this one process."""
import os
import pickle
import sys

import numpy as np
import pytest
import scipy.io

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import golden_inputs as GI  # noqa: E402
import mcg_inputs as MI  # noqa: E402
import _init_paths  # noqa: F401,E402
from mnc_amd import _lib, models, synth  # noqa: E402
from db import mcg_maskdb as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _equal(got, want, what):
    for key in ("boxes", "masks"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5])


def _csr(im):
    ptr, ids = MI.to_csr(im["labels"])
    return im["superpixels"].astype(np.int32), ptr, ids


def test_device_equals_the_reference():
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_mcg_maskdb.npz"))
    for seed in MI.GOLDEN_SEEDS:
        im = MI.engineered_image(seed)
        for top_k in (-1, MI.GOLDEN_TOP_K):
            got = M.mcg_maskdb_device(*_csr(im), mask_size=21, top_k=top_k)
            want = {k: ref["%s_k%d_%s" % (im["name"], top_k, k)] for k in ("boxes", "masks")}
            assert want["boxes"].dtype == np.float64 and want["masks"].dtype == np.uint8
            _equal(got, want, (im["name"], top_k))


@pytest.mark.parametrize("mask_size", [21, 14, 32])
def test_device_equals_the_numpy_form(mask_size):
    big = MI.random_image(375, 500, 11, 2000, 40, seed=5)
    n_sp = int(big["superpixels"].max())
    assert 1300 <= n_sp <= 1800 and len(big["labels"]) == 2000
    for im in (big, MI.engineered_image(0), MI.engineered_image(3)):
        sp, ptr, ids = _csr(im)
        want = M.mcg_maskdb_numpy(sp, ptr, ids, mask_size=mask_size)
        got = M.mcg_maskdb_device(sp, ptr, ids, mask_size=mask_size)
        assert got["masks"].shape == (len(im["labels"]), mask_size, mask_size) and 0 < want["masks"].mean() < 1
        _equal(got, want, (im["name"], mask_size))
        cut = M.mcg_maskdb_device(sp, ptr, ids, mask_size=mask_size, top_k=9)
        _equal(cut, {k: v[:9] for k, v in want.items()}, (im["name"], mask_size, "top_k"))


def test_uint16_input_and_a_one_pixel_map():
    im = MI.engineered_image(0)
    ptr, ids = MI.to_csr(im["labels"])
    _equal(M.mcg_maskdb_device(im["superpixels"], ptr, ids), M.mcg_maskdb_numpy(im["superpixels"], ptr, ids), "uint16")
    one = M.mcg_maskdb_device(np.array([[7]], np.uint16), np.array([0, 1], np.int32), np.array([7], np.int32))
    assert one["boxes"].tolist() == [[0.0, 0.0, 0.0, 0.0]] and one["masks"].all()
    zero_id = M.mcg_maskdb_device(np.array([[0, 3], [3, 0]], np.int32), np.array([0, 1, 2], np.int32), np.array([0, 3], np.int32), 2)
    assert zero_id["masks"].tolist() == [[[1, 0], [0, 1]], [[0, 1], [1, 0]]]


def test_no_proposals():
    sp = MI.engineered_image(0)["superpixels"]
    for top_k in (-1, 0):
        lists = [] if top_k == -1 else [[1], [2]]
        db = M.mcg_maskdb_device(sp, *MI.to_csr(lists), mask_size=21, top_k=top_k)
        assert db["boxes"].shape == (0, 4) and db["boxes"].dtype == np.float64
        assert db["masks"].shape == (0, 21, 21) and db["masks"].dtype == np.uint8


def _raw_call(sp, H, W, ptr, ids, n, S):
    boxes, masks = np.zeros((max(n, 1), 4)), np.zeros((max(n, 1), 32 * 32), np.uint8)
    return _lib.call("mnc_mcg_maskdb", _lib.ptr(sp), H, W, _lib.ptr(ptr), _lib.ptr(ids), n, S, _lib.ptr(boxes), _lib.ptr(masks), 0)


def test_invalid_arguments_are_refused_before_any_launch():
    sp = MI.engineered_image(0)["superpixels"].astype(np.int32)
    H, W = sp.shape
    a, b = int(sp[0, 0]), int(sp[-1, -1])
    ptr, ids = MI.to_csr([[a, b], [b]])
    bad_map = sp.copy()
    bad_map[200, 300] = 70000
    cases = [((sp, H, W, ptr, np.array([a, 70000, b], np.int32), 2, 21), "label ids"),
             ((bad_map, H, W, ptr, ids, 2, 21), "superpixel ids"),
             ((sp, H, W, np.array([0, 3, 2], np.int32), ids, 2, 21), "label_ptr"),
             ((sp, H, W, ptr, ids, 2, 33), "mask_size"),
             ((sp, 0, W, ptr, ids, 2, 21), "H=0")]
    for args, text in cases:
        with pytest.raises(_lib.MncError) as e:
            _raw_call(*args)
        assert e.value.code == 1 and text in str(e.value), text
        assert text in _lib.load().mnc_last_error().decode()
    with pytest.raises(_lib.MncError, match="label ids"):            # the same through the Python form
        M.mcg_maskdb_device(sp, ptr, np.array([a, 70000, b], np.int32))
    assert _raw_call(sp, H, W, ptr, ids, 2, 21) == 0 and _lib.load().mnc_last_error() == b""


def test_an_empty_union_is_a_status_naming_the_first_such_proposal():
    im = MI.engineered_image(0)
    sp = im["superpixels"].astype(np.int32)
    a, b = int(sp[0, 0]), int(sp[-1, -1])
    gap = im["labels"][im["tags"]["nowhere_gap"]][1]
    assert gap not in np.unique(sp) and gap < sp.max()
    for lists, first in [([[a], [b], [a, b], []], 3), ([[a], [MI.NOWHERE_ID]], 1), ([[gap, gap], [a]], 0),
                         ([[a], [b], [MI.NOWHERE_ID], [a], [b], [], [gap]], 2)]:
        with pytest.raises(_lib.MncError) as e:
            M.mcg_maskdb_device(sp, *MI.to_csr(lists))
        assert e.value.code == 1 and "proposal %d covers no pixel" % first in str(e.value), (lists, str(e.value))
        with pytest.raises(ValueError, match="proposal %d " % first):                  # the numpy form agrees
            M.mcg_maskdb_numpy(sp, *MI.to_csr(lists))
    # the empty proposals lie behind the cut: not computed, no error; and the device is fine afterwards
    lists = [[a], [b], [MI.NOWHERE_ID]]
    _equal(M.mcg_maskdb_device(sp, *MI.to_csr(lists), top_k=2), M.mcg_maskdb_numpy(sp, *MI.to_csr(lists), top_k=2), "cut")


def _tool(*args):
    import prepare_mcg_maskdb
    assert prepare_mcg_maskdb.main([str(a) for a in args]) == 0


def test_tool_device_form_writes_the_same_files_as_cpu(tmp_path):
    images = [MI.engineered_image(s) for s in MI.GOLDEN_SEEDS] + [MI.random_image(120, 150, 9, 50, 5, seed=2)]
    raw = str(tmp_path / "MCG-raw")
    for im in images:
        MI.write_mcg_raw(raw, im)
    lst = tmp_path / "val.txt"
    lst.write_text("".join(im["name"] + "\n" for im in images))
    for top_k in (-1, 20):
        dev, cpu = tmp_path / ("dev%d" % top_k), tmp_path / ("cpu%d" % top_k)
        _tool("--input", raw, "--output", dev, "--db", "val", "--list", lst, "--top_k", top_k)
        _tool("--input", raw, "--output", cpu, "--db", "val", "--list", lst, "--top_k", top_k, "--cpu")
        for im in images:
            a, b = (scipy.io.loadmat(str(d / (im["name"] + ".mat"))) for d in (dev, cpu))
            assert sorted(k for k in a if not k.startswith("__")) == ["boxes", "masks"]
            _equal(a, b, (im["name"], top_k))
            assert len(a["boxes"]) == (len(im["labels"]) if top_k == -1 else top_k)


def test_cfm_task_from_a_tool_written_maskdb_and_from_mcg_raw_dir(tmp_path, monkeypatch):
    """`--task cfm` on the reduced-width CFM net over the synthetic SDS devkit, with MCG-raw files for its images: one run reads
    the maskdb directory the tool wrote, one run has only cfg.TEST.MCG_RAW_DIR; the result pickles are equal."""
    from caffeWrapper.TesterWrapper import TesterWrapper
    from datasets.pascal_voc_seg import PascalVOCSeg
    from mnc_config import cfg
    case = GI.sds_case()
    root = str(tmp_path / "VOCdevkitSDS")
    GI.write_sds_devkit(root, case)
    raw = str(tmp_path / "MCG-raw")
    for ii, rec in enumerate(case["images"]):
        H, W = rec["im"].shape[:2]
        MI.write_mcg_raw(raw, MI.random_image(H, W, 8, 36, 7, seed=40 + ii, name=rec["name"]))
    maskdb, empty = tmp_path / "maskdb", tmp_path / "no_maskdb"
    empty.mkdir()
    _tool("--input", raw, "--output", maskdb, "--db", "val", "--list", os.path.join(root, "val.txt"))
    assert sorted(os.listdir(str(maskdb))) == sorted(rec["name"] + ".mat" for rec in case["images"])
    for k, v in GI.CFM_CFG.items():
        monkeypatch.setitem(cfg.TEST, k, v)
    path = models.write_cfm_test_prototxt(width_div=8)
    w = synth.synthetic_weights(path, seed=4)
    results = []
    for run, (maskdb_dir, raw_dir) in enumerate([(str(maskdb), ""), (str(empty), raw)]):
        monkeypatch.setattr(cfg, "ROOT_DIR", str(tmp_path / ("run%d" % run)))
        monkeypatch.setitem(cfg.TEST, "MCG_MASKDB_DIR", maskdb_dir)
        monkeypatch.setitem(cfg.TEST, "MCG_RAW_DIR", raw_dir)
        imdb = PascalVOCSeg("val", "2012", root, image_ext=".npy")
        t = TesterWrapper(path, imdb, w, "cfm")
        try:
            assert not os.path.isfile(os.path.join(t.output_dir, "res_boxes.pkl"))
            with np.errstate(all="ignore"):
                res = t.get_result()
            assert set(res) == {0.5, 0.7}
            with open(os.path.join(t.output_dir, "res_boxes.pkl"), "rb") as f:
                boxes = pickle.load(f)
            with open(os.path.join(t.output_dir, "res_masks.pkl"), "rb") as f:
                masks = pickle.load(f)
            results.append((boxes, masks))
        finally:
            t.net.close()
    assert os.listdir(str(empty)) == []                              # nothing was written on the fly
    (b0, m0), (b1, m1) = results
    total = 0
    for c in range(1, 21):
        for i in range(len(case["images"])):
            assert np.array_equal(b0[c][i], b1[c][i]) and np.array_equal(m0[c][i], m1[c][i]), (c, i)
            total += len(b0[c][i])
    assert total > 0
    monkeypatch.setitem(cfg.TEST, "MCG_RAW_DIR", "")                 # the key empty and no file: today's FileNotFoundError
    monkeypatch.setitem(cfg.TEST, "MCG_MASKDB_DIR", str(empty))
    t = TesterWrapper.__new__(TesterWrapper)
    t.imdb = PascalVOCSeg("val", "2012", root, image_ext=".npy")
    with pytest.raises(FileNotFoundError):
        t._load_mcg_maskdb(0)
