"""Shared deterministic polygon segmentations for tests/test_mask_poly_host.py and tests/test_gpu_mask_poly.py: small images placed
where csrc/mask_poly.hip can go wrong -- widths around the 64-column word, both windings and every start vertex of one shape,
steep and shallow edges walked in both directions, repeated vertices and polygons of one and two vertices, polygons that leave
the image on every side or lie outside it, a star whose walk is longer than one workgroup, annotations of several overlapping
polygons, an annotation without polygons, 65 annotations in one call.  The numpy statement of every case is computed once."""
import collections
import json
import math
import os
import subprocess
import sys

import numpy as np

from mnc_amd import polygons, rle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = collections.namedtuple("Case", "name segs H W")

WIDTHS = (1, 63, 64, 65, 130)
HEIGHTS = (1, 5, 37)


def rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def star(cx, cy, r_out, r_in, k, phase=0.1):
    """k vertices alternating between two radii."""
    out = []
    for j in range(k):
        r, a = (r_out if j % 2 == 0 else r_in), phase + 2 * math.pi * j / k
        out += [cx + r * math.cos(a), cy + r * math.sin(a)]
    return out


def rotations(xy):
    """Every start vertex of both windings."""
    pts = np.asarray(xy, np.float64).reshape(-1, 2)
    out = []
    for p in (pts, pts[::-1]):
        out += [np.roll(p, s, axis=0).reshape(-1).tolist() for s in range(len(p))]
    return out


def _size_case(H, W):
    segs = [[[-0.5, -0.5, W + 0.5, -0.5, W / 2.0, H + 0.5]],                      # a triangle over the whole image
            [rect(max(W - 6, 0), 0, W, H)],                                       # the last columns, to the image's edge
            [rect(60.3, 0.2, 67.6, H - 0.3)],                                     # across the first word boundary (where there is one)
            [[0.0, 0.0, W * 1.0, H * 0.6, W * 0.4, H * 1.0]],
            [rect(-3, -3, W + 3, H + 3)],                                         # everything
            [rect(62, 1, 66, 3), rect(126, 0, 131, H + 2)]]
    return Case("size_%dx%d" % (H, W), segs, H, W)


def _build():
    cases = [_size_case(H, W) for H in HEIGHTS for W in WIDTHS]
    shape = [5.3, 4.1, 58.7, 9.6, 66.2, 30.9, 31.4, 35.2, 3.8, 21.7]
    cases.append(Case("windings_and_starts", [[p] for p in rotations(shape)], 37, 70))
    # steep and shallow edges, each walked from both ends (a quadrilateral's four edges go right, down, left, up)
    slopes = [[[2.0, 3.0, 60.0, 9.0, 55.0, 33.0, 6.0, 27.0]], [[6.0, 27.0, 55.0, 33.0, 60.0, 9.0, 2.0, 3.0]],
              [[10.0, 1.0, 17.0, 36.0, 9.0, 30.0]], [[9.0, 30.0, 17.0, 36.0, 10.0, 1.0]],
              [[3.0, 3.0, 33.0, 33.0, 3.0, 33.0]], [[3.0, 33.0, 33.0, 33.0, 3.0, 3.0]]]          # dx == dy
    cases.append(Case("slopes_and_flips", slopes, 40, 66))
    degenerate = [[[7.0, 7.0]], [[3.0, 4.0, 30.0, 20.0]], [[5.0, 5.0, 5.0, 5.0, 25.0, 5.0, 25.0, 5.0, 25.0, 25.0, 5.0, 25.0, 5.0, 25.0]],
                  [[4.0, 4.0, 4.0, 4.0, 4.0, 4.0]], [[2.0, 2.0, 20.0, 2.0, 2.0, 2.0, 20.0, 2.0]]]
    cases.append(Case("degenerate", degenerate, 30, 40))
    halves = [[[1.5, 1.5, 20.5, 1.5, 20.5, 10.5, 1.5, 10.5]], [[0.1, 0.9, 33.33, 2.71828, 64.9, 17.0001, 12.345, 28.999]],
              [[2.0, 2.0, 9.0, 2.0, 9.0, 9.0, 2.0, 9.0]], [[2.4999, 2.5001, 9.5, 2.4999, 9.4999, 9.5001, 2.5, 9.5]],
              [[63.5, 0.5, 64.5, 0.5, 64.5, 28.5, 63.5, 28.5]]]
    cases.append(Case("half_integers_and_doubles", halves, 29, 66))
    H, W = 37, 70
    sides = [[[-20.0, 5.0, 30.0, 8.0, 25.0, 30.0, -15.0, 25.0]],                  # left
             [[40.0, 5.0, 95.0, 9.0, 90.0, 30.0, 45.0, 28.0]],                    # right
             [[10.0, -15.0, 50.0, -12.0, 45.0, 20.0, 15.0, 18.0]],                # top
             [[10.0, 20.0, 50.0, 22.0, 45.0, 60.0, 15.0, 55.0]],                  # bottom
             [[-10.0, -10.0, 80.0, -8.0, 85.0, 50.0, -12.0, 45.0]],               # all four
             [[30.0, 30.0, 80.0, 36.0, 75.0, 50.0, 35.0, 55.0]],                  # the bottom right corner
             [[-30.0, 5.0, -5.0, 8.0, -8.0, 30.0]], [[80.0, 5.0, 95.0, 8.0, 90.0, 30.0]],      # outside: left, right
             [[10.0, -30.0, 50.0, -25.0, 30.0, -5.0]], [[10.0, 45.0, 50.0, 50.0, 30.0, 70.0]],  # above, below
             [[-50.0, -50.0, -10.0, -40.0, -30.0, -10.0]]]
    cases.append(Case("leaving_and_outside", sides, H, W))
    cases.append(Case("star_300", [[star(100.2, 90.7, 88.0, 35.0, 300)]], 180, 200))
    unions = [[rect(5, 5, 30, 20), rect(20, 10, 50, 30)],                         # overlapping: a union, not a cancellation
              [star(30.0, 18.0, 17.0, 6.0, 10), rect(25, 12, 66, 24), [20.0, 1.0, 69.0, 3.0, 40.0, 36.0]],
              [rect(2, 2, 6, 6), rect(62, 30, 68, 36)],                           # far apart: different words, different rows
              [],
              [rect(10, 10, 20, 20), rect(10, 10, 20, 20)],
              [rect(-10, 50, -5, 60), rect(3, 3, 9, 9)]]                          # one polygon outside, one inside
    cases.append(Case("unions", unions, H, W))
    rng = np.random.default_rng(65)
    many = []
    for i in range(65):
        k = int(rng.integers(3, 8))
        c = rng.uniform((0, 0), (130, 37))
        pts = c + rng.uniform(-14, 14, (k, 2))
        many.append([] if i == 31 else [pts.reshape(-1).tolist()] + ([rect(*(c.tolist() + (c + 3).tolist()))] if i % 5 == 0 else []))
    cases.append(Case("sixty_five", many, 37, 130))
    return cases


CASES = _build()
IDS = [c.name for c in CASES]
_REFERENCE = {}


def reference(case):
    """masks_from_polygons_numpy of the case, computed once and shared (nobody changes it)."""
    if case.name not in _REFERENCE:
        _REFERENCE[case.name] = polygons.masks_from_polygons_numpy(case.segs, case.H, case.W)
    return _REFERENCE[case.name]


def clamped_and_carried(case):
    """-> (crossings clamped to y == H, columns whose first pixel has an odd number of toggles before it) over the case."""
    clamped = carried = 0
    for polys in case.segs:
        for xy in polys:
            x, y = polygons.polygon_crossings_numpy(xy, case.H, case.W)
            clamped += int((y == case.H).sum())
            before = np.bincount((x * case.H + y) // case.H, minlength=case.W + 1)     # the toggles whose position lies in column c
            carried += int((np.cumsum(before)[:case.W - 1] & 1).sum())               # ... in the columns before c + 1
    return clamped, carried


def coco_files(tmp_path):
    """A small ground-truth file with polygon segmentations and one crowd RLE, the same file with the polygons rasterised to RLE
    by the numpy statement, and a results file (RLE results and one polygon result) -> (gt, gt rasterised, dt, dt rasterised)."""
    H, W = 37, 70
    case = {c.name: c for c in CASES}["unions"]
    gts = [s for s in case.segs if s] + [[star(40.0, 18.0, 16.0, 7.0, 12)], [rect(50, 5, 68, 30)]]
    crowd = rle.mask_rle_numpy(polygons.masks_from_polygons_numpy([[rect(0, 20, 70, 37)]], H, W), H, W)[0]
    anns = [{"id": k + 1, "image_id": "im0", "category_id": 1 + k % 2, "segmentation": s, "iscrowd": 0} for k, s in enumerate(gts)]
    anns[0]["area"] = 900.0                                                        # the others take the area from the mask
    anns.append({"id": len(anns) + 1, "image_id": "im0", "category_id": 1, "segmentation": crowd, "iscrowd": 1})
    rng = np.random.default_rng(9)
    dts = []
    for k, s in enumerate(gts + gts):                                              # every ground truth jittered twice
        moved = [(np.asarray(p, np.float64) + rng.uniform(-3, 3)).tolist() for p in s]
        dts.append({"image_id": "im0", "category_id": 1 + k % 2, "segmentation": moved, "score": float(rng.uniform(0.1, 1.0))})
    images = [{"id": "im0", "height": H, "width": W}, {"id": "im1", "height": 9, "width": 9}]

    def rasterised(entries):
        out = []
        for e in entries:
            e = dict(e)
            if isinstance(e["segmentation"], list):
                e["segmentation"] = rle.mask_rle_numpy(polygons.masks_from_polygons_numpy([e["segmentation"]], H, W), H, W)[0]
            out.append(e)
        return out

    paths = []
    for name, body in (("gt", anns), ("gt_rle", rasterised(anns))):
        paths.append(str(tmp_path / (name + ".json")))
        with open(paths[-1], "w") as f:
            json.dump({"images": images, "categories": [{"id": 1}, {"id": 2}], "annotations": body}, f)
    for name, body in (("dt", dts[:3] + rasterised(dts[3:])), ("dt_rle", rasterised(dts))):
        paths.append(str(tmp_path / (name + ".json")))
        with open(paths[-1], "w") as f:
            json.dump(body, f)
    return paths


def tool(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "tools", "eval_coco.py")] + list(args), capture_output=True, text=True,
                          cwd=REPO)


_facts = [clamped_and_carried(c) for c in CASES if c.name in ("leaving_and_outside", "size_5x65")]
assert any(f[0] > 0 for f in _facts), "no case has a crossing clamped to yd == H"
assert any(f[1] > 0 for f in _facts), "no case carries an odd parity into a column"
