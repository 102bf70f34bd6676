#!/usr/bin/env python3
"""Golden maskdb entries produced by RUNNING THE REFERENCE'S OWN tools/prepare_mcg_maskdb.py:process_roidb(..., 'val') where the
reference lies (same in-memory python-2 -> 3 patching and stubs as make_golden.py / make_golden_eval.py), on the two engineered
MCG-raw images of tests/mcg_inputs.py, once with top_k = -1 and once with top_k = mcg_inputs.GOLDEN_TOP_K.  What scipy.io.loadmat
gives back for the files it wrote is stored: <name>_k<top_k>_boxes (float64 [n, 4]) and _masks (uint8 [n, 21, 21]).

cv2 is absent: cv2.resize(..., interpolation=cv2.INTER_NEAREST) is the few lines below, OpenCV's resizeNN written with Python
floats (the inverse scale 1.0 / (dst / src) formed in two steps, then floor, clamped to the last source index).  Nothing of the
package under test is imported, so the golden does not pass through the code it checks.

    python tests/golden/make_golden_mcg.py        -> tests/golden/reference_mcg_maskdb.npz
"""
import math
import os
import sys
import tempfile
import types

import numpy as np
import scipy.io

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_eval as MGE  # noqa: E402
import mcg_inputs as MI  # noqa: E402

INTER_NEAREST = 0


def resize_nearest(src, dsize, dst=None, fx=None, fy=None, interpolation=None):
    assert interpolation == INTER_NEAREST and src.ndim == 2
    dw, dh = dsize
    sh, sw = src.shape
    ifx, ify = 1.0 / (float(dw) / sw), 1.0 / (float(dh) / sh)
    sx = [min(int(math.floor(x * ifx)), sw - 1) for x in range(dw)]
    sy = [min(int(math.floor(y * ify)), sh - 1) for y in range(dh)]
    return src[np.array(sy)[:, None], np.array(sx)[None, :]]


def main():
    MG.install_reference()
    sys.modules["cv2"].resize = resize_nearest
    sys.modules["cv2"].INTER_NEAREST = INTER_NEAREST
    MG._stub("datasets")
    MG._stub("datasets.pascal_voc_seg", PascalVOCSeg=None)
    if "PIL" not in sys.modules:
        try:
            import PIL  # noqa: F401
        except ImportError:
            MG._stub("PIL")
    path = os.path.join(MG.REF, "tools", "prepare_mcg_maskdb.py")
    mod = types.ModuleType("ref_prepare_mcg_maskdb")
    mod.__file__ = path
    with open(path) as f:
        src = MGE._py3_more(f.read()).replace("dtype=np.bool)", "dtype=bool)")
    exec(compile(src, path, "exec"), mod.__dict__)          # __name__ is not '__main__': only the definitions run
    g = {}
    with tempfile.TemporaryDirectory() as root:
        raw = os.path.join(root, "MCG-raw")
        images = [MI.engineered_image(s) for s in MI.GOLDEN_SEEDS]
        for im in images:
            MI.write_mcg_raw(raw, im)
        for top_k in (-1, MI.GOLDEN_TOP_K):
            out = os.path.join(root, "out_%d" % top_k)
            os.makedirs(out)
            mod.file_list = [im["name"] for im in images]
            mod.input_dir, mod.output_dir, mod.mask_size, mod.top_k = raw, out, 21, top_k
            mod.process_roidb(0, len(images), "val")
            for im in images:
                db = scipy.io.loadmat(os.path.join(out, im["name"] + ".mat"))
                g["%s_k%d_boxes" % (im["name"], top_k)] = db["boxes"]
                g["%s_k%d_masks" % (im["name"], top_k)] = db["masks"]
    np.savez_compressed(os.path.join(HERE, "reference_mcg_maskdb.npz"), **g)
    for k, v in g.items():
        print(k, v.shape, v.dtype, int(v.sum()))


if __name__ == "__main__":
    main()
