"""CPU side of the GPU rendering (csrc/render.hip): the order-free per-pixel rule the kernel evaluates IS the reference's
sequential painting, the blend rule IS Pillow's, and the switch is off by default and leaves the host path alone."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import golden_inputs as GI  # noqa: E402
import render_inputs as RI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_config import cfg  # noqa: E402
from utils import vis_seg  # noqa: E402


def test_rule_equals_the_sequential_painting_on_the_golden_cases():
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_eval_outputs.npz"))
    case = GI.sds_case()
    for ii in (0, 3):
        H, W = case["images"][ii]["im"].shape[:2]
        pred = GI.vis_pred_dict(case, ii)
        want = vis_seg._convert_pred_to_image(W, H, pred)
        got = RI.rule_images(W, H, pred, cfg.BINARIZE_THRESH)
        assert np.array_equal(want[0], ref["vis_inst_%d" % ii]) and np.array_equal(want[1], ref["vis_cls_%d" % ii])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_rule_equals_the_sequential_painting_on_random_cases():
    cases = RI.all_cases()
    assert len(cases) >= 200
    cov = RI.coverage(cases)
    assert all(cov.values()), cov
    assert {(H, W) for W, H, _, _ in cases} >= set(RI.BIG_SIZES)
    bad = []
    for k, (W, H, pred, _) in enumerate(cases):
        want = vis_seg._convert_pred_to_image(W, H, pred)
        got = RI.rule_images(W, H, pred, cfg.BINARIZE_THRESH)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            bad.append(k)
    assert not bad, bad


def test_blend_rule_equals_pillow_on_all_pairs():
    from PIL import Image
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, 1)
    b = np.repeat(np.arange(256, dtype=np.uint8)[None, :], 256, 0)
    a3, b3 = np.stack([a] * 3, -1), np.stack([b] * 3, -1)
    for alpha in (0.8, 0.5, 0.0, 1.0):
        want = np.asarray(Image.blend(Image.fromarray(a3).convert("RGBA"), Image.fromarray(b3).convert("RGBA"), alpha))
        got = RI.blend_rule(a3, b3, alpha)
        assert np.array_equal(got, want[:, :, :3]), alpha
        assert (want[:, :, 3] == 255).all()


def test_voc_colour_bits_need_three_rounds_below_256():
    """render.hip computes a colour from label bits 0..8 only: for labels below 256 the map's rounds j >= 3 add nothing."""
    cm = vis_seg._get_voc_color_map().astype(int)
    for label in range(256):
        r = g = b = 0
        cid = label
        for j in range(3):
            r |= ((cid >> 0) & 1) << (7 - j)
            g |= ((cid >> 1) & 1) << (7 - j)
            b |= ((cid >> 2) & 1) << (7 - j)
            cid >>= 3
        assert (r, g, b) == tuple(cm[label])


def test_switch_is_off_and_the_host_path_never_touches_the_library(tmp_path, monkeypatch):
    import pickle
    from PIL import Image
    assert cfg.TEST.USE_GPU_VIS is False

    def boom(*a, **k):
        raise AssertionError("the host visualisation called into the library")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    W, H, pred, _ = RI.random_case(40)
    names = ["img0"]
    gt = tmp_path / "gt" / "img"
    gt.mkdir(parents=True)
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).save(str(gt / "img0.png"))
    out = tmp_path / "out"
    out.mkdir()
    cls_names = ["__background__"] + ["c%d" % i for i in range(1, 21)]
    det = [[np.zeros((0, 5))] for _ in cls_names]
    seg = [[np.zeros((0, 1, RI.S, RI.S), np.float32)] for _ in cls_names]
    for box, m, c in zip(pred["boxes"], pred["masks"], pred["cls_name"]):
        det[c][0] = np.vstack((det[c][0], np.asarray(box, np.float64)[None]))
        seg[c][0] = np.concatenate((seg[c][0], m[None, None]))
    with open(str(out / "res_boxes.pkl"), "wb") as f:
        pickle.dump(det, f)
    with open(str(out / "res_masks.pkl"), "wb") as f:
        pickle.dump(seg, f)
    vis_seg.vis_seg(names, cls_names, str(out), str(tmp_path / "gt"), image_ext=".png")
    assert Image.open(str(out / "SegRes" / "img0.png")).size == (W, H)


def test_header_declares_the_render_entries():
    decls = _lib.parse_header()
    for name in ("mnc_render_instances", "mnc_render_records", "mnc_net_render"):
        assert name in decls
    assert decls["mnc_render_records"][2][-1] == "d_kept" and decls["mnc_render_instances"][2][-1] == "device_id"
