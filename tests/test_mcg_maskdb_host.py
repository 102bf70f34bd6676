"""The MCG proposal maskdb without a GPU (db/mcg_maskdb.py, tools/prepare_mcg_maskdb.py, TesterWrapper._load_mcg_maskdb): the numpy
form against what the REFERENCE'S OWN tools/prepare_mcg_maskdb.py wrote for the engineered images of tests/mcg_inputs.py
(tests/golden/make_golden_mcg.py -> reference_mcg_maskdb.npz), the pinned nearest index rule, the reader, the tool, the tester's
on-the-fly path with the device form replaced by the numpy form, and the argument checks of mnc_mcg_maskdb that run before any
device work."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import scipy.io

import mcg_inputs as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _init_paths  # noqa: F401,E402
from db import mcg_maskdb as M  # noqa: E402

TOOL = os.path.join(ROOT, "tools", "prepare_mcg_maskdb.py")


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "reference_mcg_maskdb.npz")))


@pytest.fixture(scope="module")
def images():
    return [MI.engineered_image(s) for s in MI.GOLDEN_SEEDS]


def _same(db, ref, name, top_k):
    for key in ("boxes", "masks"):
        want = ref["%s_k%d_%s" % (name, top_k, key)]
        assert db[key].dtype == want.dtype and db[key].shape == want.shape and np.array_equal(db[key], want), (name, top_k, key)


def _exact_integer_rule(sp, ids, box, S=21):
    x1, y1, x2, y2 = (int(v) for v in box)
    w, h = x2 - x1 + 1, y2 - y1 + 1
    P = np.isin(sp, ids)
    return P[(y1 + np.arange(S) * h // S)[:, None], (x1 + np.arange(S) * w // S)[None, :]].astype(np.uint8)


def test_engineered_images_contain_the_cases(images):
    """The set holds, by construction, every case the kernel has to get right."""
    for im in images:
        sp = im["superpixels"].astype(np.int32)
        assert sp.dtype == np.int32 and im["superpixels"].dtype == np.uint16 and min(sp.shape) >= 400 and sp.min() >= 1
        ptr, ids = MI.to_csr(im["labels"])
        db = M.mcg_maskdb_numpy(sp, ptr, ids)
        b = db["boxes"].astype(np.int64)
        widths, heights = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
        for s in MI.TRAP_SIZES:                                     # the sizes where the index rules differ
            assert s in widths and s in heights, s
        for tag, extent in im["extents"].items():
            assert tuple(b[im["tags"][tag]]) == extent, tag
        t = im["tags"]
        assert widths[t["small"]] < 21 and heights[t["small"]] < 21
        assert widths[t["equal"]] == 21 and heights[t["equal"]] == 21
        assert (widths[t["whole"]], heights[t["whole"]]) == (MI.ENG_W, MI.ENG_H)
        assert widths[t["thin_w"]] == 1 and heights[t["thin_w"]] > 21 and heights[t["thin_h"]] == 1 and widths[t["thin_h"]] > 21
        dup = im["labels"][t["duplicates"]]
        assert len(set(dup)) < len(dup)
        present = set(np.unique(sp).tolist())
        for tag in ("nowhere_high", "nowhere_gap"):
            lst = im["labels"][t[tag]]
            assert sum(i not in present for i in lst) == 1 and sum(i in present for i in lst) >= 2
        assert max(im["labels"][t["nowhere_high"]]) > sp.max() > max(im["labels"][t["nowhere_gap"]])
        assert b[t["left"], 0] == 0 and b[t["top"], 1] == 0 and b[t["right"], 2] == MI.ENG_W - 1 and b[t["bottom"], 3] == MI.ENG_H - 1
        # the trap proposals are sensitive to the rule: the exact integer rule gives another mask for at least one of them
        differs = [not np.array_equal(db["masks"][t[tag]], _exact_integer_rule(sp, im["labels"][t[tag]], b[t[tag]]))
                   for tag in ("trap0", "trap1", "trap2", "trap3")]
        assert any(differs)
        assert 0 < db["masks"].mean() < 1


def test_numpy_form_equals_the_reference(images, ref):
    for im in images:
        ptr, ids = MI.to_csr(im["labels"])
        for top_k in (-1, MI.GOLDEN_TOP_K):
            db = M.mcg_maskdb_numpy(im["superpixels"].astype(np.int32), ptr, ids, mask_size=21, top_k=top_k)
            _same(db, ref, im["name"], top_k)
            assert len(db["boxes"]) == (len(im["labels"]) if top_k == -1 else top_k)
    assert ref["mcg_eng_0_k-1_boxes"].dtype == np.float64 and ref["mcg_eng_0_k-1_masks"].dtype == np.uint8


def test_nearest_index_rule_is_the_two_step_form():
    differ_exact = 0
    for w in range(1, 4097):
        got = M.nearest_src_index(21, w)
        want = [min(int(math.floor(dx * (1.0 / (21.0 / w)))), w - 1) for dx in range(21)]
        assert got.tolist() == want, w
        differ_exact += sum(a != dx * w // 21 for dx, a in enumerate(want))
    assert int(M.nearest_src_index(21, 87)[7]) == 28 and 7 * 87 // 21 == 29        # the trap itself
    assert differ_exact == 569
    assert M.nearest_src_index(21, 1).tolist() == [0] * 21 and M.nearest_src_index(21, 21).tolist() == list(range(21))


def test_numpy_form_raises_on_an_empty_union(images):
    sp = images[0]["superpixels"].astype(np.int32)
    for lists in ([[int(sp[0, 0])], []], [[int(sp[0, 0])], [MI.NOWHERE_ID]]):
        ptr, ids = MI.to_csr(lists)
        with pytest.raises(ValueError, match="proposal 1"):
            M.mcg_maskdb_numpy(sp, ptr, ids)
        assert len(M.mcg_maskdb_numpy(sp, ptr, ids, top_k=1)["boxes"]) == 1       # proposals after the cut are not computed


def test_read_mcg_raw_round_trips(images, tmp_path):
    for im in images:
        path = MI.write_mcg_raw(str(tmp_path), im)
        raw = scipy.io.loadmat(path)
        assert raw["superpixels"].dtype == np.uint16 and raw["superpixels"].flags["F_CONTIGUOUS"]
        assert raw["labels"].shape == (len(im["labels"]), 1) and raw["labels"][3][0].dtype == np.uint16
        sp, ptr, ids = M.read_mcg_raw(path)
        assert sp.dtype == np.int32 and sp.flags["C_CONTIGUOUS"] and np.array_equal(sp, im["superpixels"])
        want_ptr, want_ids = MI.to_csr(im["labels"])
        assert ptr.dtype == np.int32 and ids.dtype == np.int32 and ids.flags["C_CONTIGUOUS"]
        assert np.array_equal(ptr, want_ptr) and np.array_equal(ids, want_ids)


def _run_tool(*args):
    return subprocess.run([sys.executable, TOOL] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT)


def test_tool_cpu_writes_the_reference_files(images, ref, tmp_path):
    raw = str(tmp_path / "MCG-raw")
    for im in images:
        MI.write_mcg_raw(raw, im)
    lst = tmp_path / "val.txt"
    lst.write_text("".join(im["name"] + "\n" for im in images))
    for top_k in (-1, MI.GOLDEN_TOP_K):
        out = tmp_path / ("out_%d" % top_k)
        r = _run_tool("--input", raw, "--output", out, "--db", "val", "--list", lst, "--top_k", top_k, "--cpu")
        assert r.returncode == 0, r.stderr
        for im in images:
            db = scipy.io.loadmat(str(out / (im["name"] + ".mat")))
            assert sorted(k for k in db if not k.startswith("__")) == ["boxes", "masks"]
            _same(db, ref, im["name"], top_k)
    # files that exist are skipped: a marker in place of the first image's file survives, the missing one is written
    out = tmp_path / "out_skip"
    out.mkdir()
    marker = out / (images[0]["name"] + ".mat")
    marker.write_bytes(b"already here")
    r = _run_tool("--input", raw, "--output", out, "--db", "val", "--list", lst, "--cpu", "--para_job", 2)
    assert r.returncode == 0, r.stderr
    assert marker.read_bytes() == b"already here"
    _same(scipy.io.loadmat(str(out / (images[1]["name"] + ".mat"))), ref, images[1]["name"], -1)


def test_tool_refuses_the_training_branch(tmp_path):
    for args in (("--db", "train"), ()):                           # the reference's default is train as well
        r = _run_tool("--input", tmp_path, "--output", tmp_path / "o", *args)
        assert r.returncode != 0 and "out of scope" in r.stderr and "train" in r.stderr
        assert not (tmp_path / "o").exists()


def test_tester_builds_the_maskdb_on_the_fly(images, ref, tmp_path, monkeypatch):
    import fake_backend
    fake_backend.install(monkeypatch)
    from caffeWrapper.TesterWrapper import TesterWrapper
    from mnc_config import cfg
    assert cfg.TEST.MCG_RAW_DIR == ""
    raw, maskdb = str(tmp_path / "MCG-raw"), tmp_path / "maskdb"
    maskdb.mkdir()
    for im in images:
        MI.write_mcg_raw(raw, im)
    t = TesterWrapper.__new__(TesterWrapper)
    t.imdb = types.SimpleNamespace(_image_index=[im["name"] for im in images])
    monkeypatch.setitem(cfg.TEST, "MCG_MASKDB_DIR", str(maskdb))
    with pytest.raises(FileNotFoundError):                          # the key empty: today's behaviour
        t._load_mcg_maskdb(0)
    calls = []

    def numpy_form(sp, ptr, ids, mask_size=21, top_k=-1, device_id=None):
        calls.append(mask_size)
        return M.mcg_maskdb_numpy(sp, ptr, ids, mask_size=mask_size, top_k=top_k)
    monkeypatch.setattr(M, "mcg_maskdb_device", numpy_form)
    monkeypatch.setitem(cfg.TEST, "MCG_RAW_DIR", raw)
    for i, im in enumerate(images):
        db = t._load_mcg_maskdb(i)
        _same(db, ref, im["name"], -1)
        written = str(tmp_path / (im["name"] + "_tool.mat"))
        M.write_maskdb(written, db)
        loaded = scipy.io.loadmat(written)
        for key in ("boxes", "masks"):                              # the dict equals loadmat of the file the tool writes
            assert db[key].dtype == loaded[key].dtype and np.array_equal(db[key], loaded[key])
    assert calls == [21, 21] and os.listdir(str(maskdb)) == []      # nothing is written
    # an existing maskdb file takes precedence over MCG_RAW_DIR
    scipy.io.savemat(str(maskdb / (images[0]["name"] + ".mat")), {"boxes": np.full((2, 4), 5.0), "masks": np.ones((2, 21, 21), bool)})
    db = t._load_mcg_maskdb(0)
    assert len(calls) == 2 and db["boxes"].shape == (2, 4) and np.all(db["boxes"] == 5.0)


def test_entry_is_declared_exported_and_checks_its_arguments_first():
    """mnc_mcg_maskdb: the prototype, the symbol, and every MNC_ERR_INVALID case that is decided before any device work (so they
    behave the same with and without a GPU); n == 0 needs no device either."""
    from mnc_amd import _lib
    decls = _lib.parse_header()
    assert decls["mnc_mcg_maskdb"][2] == ["superpixels", "H", "W", "label_ptr", "label_ids", "n", "mask_size", "boxes", "masks",
                                          "device_id"]
    _lib.load()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T mnc_mcg_maskdb" in syms
    sp = np.arange(1, 13, dtype=np.int32).reshape(3, 4)
    ptr, ids = np.array([0, 2, 3], np.int32), np.array([1, 2, 7], np.int32)

    def call(sp=sp, H=3, W=4, ptr=ptr, ids=ids, n=2, S=21):
        boxes, masks = np.zeros((max(n, 1), 4)), np.zeros((max(n, 1), 32 * 32), np.uint8)
        return _lib.call("mnc_mcg_maskdb", _lib.ptr(sp), H, W, _lib.ptr(ptr), _lib.ptr(ids), n, S, _lib.ptr(boxes), _lib.ptr(masks), 0)

    assert call(n=0) == 0
    bad_sp = sp.copy()
    bad_sp[1, 1] = 70000
    for kw, text in [({"ids": np.array([1, 70000, 7], np.int32)}, "label ids"), ({"sp": bad_sp}, "superpixel ids"),
                     ({"sp": -sp}, "superpixel ids"), ({"ptr": np.array([0, 3, 2], np.int32)}, "label_ptr"),
                     ({"ptr": np.array([1, 2, 3], np.int32)}, "label_ptr"), ({"S": 33}, "mask_size"), ({"S": 0}, "mask_size"),
                     ({"H": 0}, "H="), ({"W": 40000}, "W="), ({"n": -1}, "n=")]:
        with pytest.raises(_lib.MncError) as e:
            call(**kw)
        assert e.value.code == 1 and text in str(e.value), kw
