"""Inputs of the image-space voting fixtures (cpu_mask_voting, cfg.TEST.USE_GPU_MASK_MERGE = False): shared by
tests/golden/make_golden_image_voting.py, which runs the reference on them, and the tests, which regenerate them and check their
digests against the ones stored next to the outputs.

Every case is a dict: boxes [n,4] float32 (original-image pixels), masks [n,1,21,21] float32, scores [n,21] float32, H, W and
max_per_image.  The hand-built cases cover what the seeded voting cases of golden_inputs.py do not reach."""
import hashlib

import numpy as np

import golden_inputs as GI

K = 21
S = 21


def _case(boxes, masks, scores, H, W, max_per_image):
    return {"boxes": np.ascontiguousarray(boxes, np.float32), "masks": np.ascontiguousarray(masks, np.float32),
            "scores": np.ascontiguousarray(scores, np.float32), "H": int(H), "W": int(W), "max_per_image": int(max_per_image)}


def _blob(rng, n):
    return GI._blob_masks(rng, n, S)


def ties_case(seed=41):
    """Exact score ties inside the keep lists: 12 boxes on a grid (NMS keeps them all) and 4 low-scored near-copies.  Class 4
    has five boxes at 0.75 and max_per_image = 4, so its tie group straddles the cut (the rule "stable ascending, reversed" picks
    the LAST four in keep order); class 7 has two more at 0.75, so the global threshold 0.75 lets 6 > max_per_image rows through.
    16 boxes: every keep list is shorter than 17, where the reference's own argsort is stable."""
    rng = np.random.default_rng(seed)
    H, W = 90, 130
    boxes = []
    for gy in range(3):
        for gx in range(4):
            x0, y0 = gx * 32 + rng.uniform(0, 4), gy * 30 + rng.uniform(0, 4)
            boxes.append([x0, y0, x0 + rng.uniform(18, 26), y0 + rng.uniform(16, 24)])
    for src in (0, 3, 6, 9):
        boxes.append([v + rng.uniform(-1.5, 1.5) for v in boxes[src]])
    boxes = np.clip(np.array(boxes), 0, [W - 1, H - 1, W - 1, H - 1])
    scores = rng.uniform(0.0, 0.5, (16, K)).astype(np.float32)
    scores[12:, :] = rng.uniform(0.0, 0.2, (4, K))
    scores[[0, 3, 6, 9, 11], 4] = np.float32(0.75)
    scores[[1, 4], 4] = np.float32(0.6)
    scores[[2, 10], 7] = np.float32(0.75)
    return _case(boxes, _blob(rng, 16), scores, H, W, 4)


def centre_case(seed=42):
    """A result whose aggregate never reaches 0.4: three copies of one box whose masks are above 0.4 on disjoint thirds, with
    class-2 weights of about 1/3 each -> no canvas pixel >= 0.4, the box falls back to the Python-2 centre pixel (W // 2, H // 2)
    of an odd-sized image, whose canvas value (about 1/3) is then resampled.  Three more boxes elsewhere."""
    rng = np.random.default_rng(seed)
    H, W = 101, 77
    box = [20.0, 30.0, 60.0, 70.0]
    boxes = np.array([box, box, box, [2.0, 3.0, 25.0, 20.0], [50.0, 75.0, 74.0, 99.0], [5.0, 60.0, 30.0, 95.0]])
    masks = _blob(rng, 6)
    for i, (a, b) in enumerate(((0, 6), (8, 13), (15, 21))):     # gaps: the resized thirds never overlap above 0.4
        m = np.full((S, S), 0.1, np.float32)
        m[:, a:b] = 0.9
        masks[i, 0] = m
    scores = rng.uniform(0.001, 0.02, (6, K)).astype(np.float32)
    scores[:3, 2] = np.array([0.5, 0.49, 0.48], np.float32)
    return _case(boxes, masks, scores, H, W, 100)


def borders_case(seed=43):
    """Boxes touching every image border, the whole image, 1-pixel-wide and 1-pixel-high boxes, and coordinates on .5 (np.round
    rounds half to even), each with two jittered companions so that candidate sets have several members."""
    rng = np.random.default_rng(seed)
    H, W = 64, 96
    base = np.array([[0, 0, 30, 20], [W - 26, 0, W - 1, 18], [0, H - 16, 22, H - 1], [W - 31, H - 21, W - 1, H - 1],
                     [0, 0, W - 1, H - 1], [40, 10, 40, 50], [10, 30, 70, 30], [12.5, 7.5, 33.5, 28.5], [0.4, 0.5, 5.5, 1.5],
                     [60.5, 40.5, 61.5, 41.5]], np.float64)
    boxes = [base]
    for _ in range(2):
        j = base + rng.normal(0, 0.3, base.shape)
        j[:, 2] = np.maximum(j[:, 2], j[:, 0])
        j[:, 3] = np.maximum(j[:, 3], j[:, 1])
        boxes.append(j)
    boxes = np.concatenate(boxes, 0)
    boxes = np.clip(boxes, 0, [W - 1, H - 1, W - 1, H - 1])
    n = boxes.shape[0]
    logits = rng.normal(0, 1.0, (n, K))
    logits[np.arange(n), 1 + np.arange(n) % (K - 1)] += 3.0
    return _case(boxes, _blob(rng, n), GI._softmax_rows(logits), H, W, 100)


def many_case(seed=44, n=1100):
    """One cluster of 1100 near-identical boxes: each class keeps one of them and votes with all 1100 (more candidates than the
    kernels stage in LDS)."""
    rng = np.random.default_rng(seed)
    H, W = 200, 300
    boxes = np.array([100.0, 60.0, 180.0, 140.0]) + rng.normal(0, 2.0, (n, 4))
    logits = rng.normal(0, 1.0, (n, K))
    return _case(boxes, _blob(rng, n), GI._softmax_rows(logits), H, W, 100)


def voting_cases():
    """tag -> case: the seeded voting cases of golden_inputs.py and the hand-built ones above."""
    out = {}
    for tag, (n, H, W, seed) in GI.VOTING_CASES.items():
        vc = GI.voting_case(n, H, W, seed)
        out[tag] = _case(vc["boxes"], vc["masks"], vc["scores"], H, W, 100)
    out["ties"] = ties_case()
    out["centre"] = centre_case()
    out["borders"] = borders_case()
    out["many"] = many_case()
    return out


def digest(*arrays):
    """sha256 over the arrays' dtypes, shapes and bytes."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def case_digest(case):
    return digest(case["boxes"], case["masks"], case["scores"],
                  np.array([case["H"], case["W"], case["max_per_image"]], np.int64))


def tester_digest(canned):
    return digest(*[v for out in canned for _, v in sorted(out.items())])
