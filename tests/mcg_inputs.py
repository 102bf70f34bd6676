"""Seeded synthetic MCG-raw images for the maskdb tests (tools/prepare_mcg_maskdb.py, db/mcg_maskdb.py, csrc/mcg_maskdb.hip), in
the shape of the published MCG candidates: `superpixels` a 1-based uint16 label map, `labels` an [n, 1] object array of [1, k]
uint16 rows.  Shared by the golden generator (tests/golden/make_golden_mcg.py), the CPU tests and the GPU tests; imports nothing
of the package under test.

    engineered_image(seed)   420 x 460, a jittered-grid label map with finely subdivided rectangles carved into it so that
                             proposals of exactly known extents exist (the widths / heights 87, 119, 153, 174 where the nearest
                             index rules differ, below / equal to the 21-pixel mask, one pixel wide / high, the whole image,
                             every border), plus a duplicate-id list, lists with ids that occur nowhere, and random unions
    random_image(...)        a jittered grid of any size with random unions of adjacent and of scattered superpixels
"""
import os

import numpy as np

ENG_H, ENG_W = 420, 460
TRAP_SIZES = (87, 119, 153, 174)
# (tag, x, y, w, h): rectangles carved into the engineered map; every TRAP size occurs as a width and as a height
ENG_RECTS = [("trap0", 5, 5, 87, 174), ("trap1", 100, 5, 119, 153), ("trap2", 230, 5, 153, 119), ("trap3", 5, 200, 174, 87),
             ("small", 200, 200, 13, 9), ("equal", 230, 200, 21, 21), ("thin_w", 270, 200, 1, 40), ("thin_h", 300, 200, 50, 1)]
GOLDEN_SEEDS = (0, 1)          # the two images of the reference golden
GOLDEN_TOP_K = 17              # its `--top_k` cut (the other run is -1)
NOWHERE_ID = 60000             # above every id of any map here


def jittered_grid(H, W, cell, rng):
    """[H, W] int32, ids 1..k all present: a grid of ~cell x cell superpixels whose edges wander by a few pixels."""
    dy = np.clip(np.cumsum(rng.integers(-1, 2, W)), -3, 3) + 3
    dx = np.clip(np.cumsum(rng.integers(-1, 2, H)), -3, 3) + 3
    yy, xx = np.mgrid[0:H, 0:W]
    gy, gx = (yy + dy[None, :]) // cell, (xx + dx[:, None]) // cell
    _, inv = np.unique(gy * (gx.max() + 1) + gx, return_inverse=True)
    return (inv.reshape(H, W) + 1).astype(np.int32)


def _stripes(n, rng):
    """Stripe index of each of n positions, stripes 1-3 wide."""
    widths = []
    while sum(widths) < n:
        widths.append(int(rng.integers(1, 4)))
    return np.repeat(np.arange(len(widths)), widths)[:n]


def engineered_image(seed=0):
    """-> {'name', 'superpixels' uint16 [420, 460], 'labels': list of int lists, 'tags': {tag: proposal index},
           'extents': {tag: (x1, y1, x2, y2)}} -- the extents the tagged proposals have by construction."""
    rng = np.random.default_rng(1000 + seed)
    sp = jittered_grid(ENG_H, ENG_W, 14, rng)
    next_id = int(sp.max()) + 5                    # ids max+1 .. max+4 occur nowhere
    gap_id = int(sp.max()) + 2
    labels, tags, extents = [], {}, {}

    def add(tag, ids, extent=None):
        tags[tag] = len(labels)
        labels.append([int(i) for i in ids])
        if extent is not None:
            extents[tag] = extent

    for tag, x, y, w, h in ENG_RECTS:
        cx, cy = _stripes(w, rng), _stripes(h, rng)
        ncx = int(cx.max()) + 1
        cells = next_id + cy[:, None] * ncx + cx[None, :]
        sp[y:y + h, x:x + w] = cells
        next_id = int(cells.max()) + 1
        checker = (cy[:, None] + cx[None, :]) % 2 == 0
        ids = set(np.unique(cells[checker]).tolist())
        ids.update(int(cells[a, b]) for a in (0, h - 1) for b in (0, w - 1))      # the four corners pin the extent
        add(tag, sorted(ids), (x, y, x + w - 1, y + h - 1))
    assert next_id <= 65535
    present = np.unique(sp)
    grid_ids = present[present < gap_id - 1]
    # the whole image: two thirds of the grid superpixels and the four corner superpixels; touches every border
    whole = set(int(i) for i in grid_ids if i % 3) | {int(sp[0, 0]), int(sp[0, -1]), int(sp[-1, 0]), int(sp[-1, -1])}
    add("whole", sorted(whole), (0, 0, ENG_W - 1, ENG_H - 1))
    add("left", [sp[ENG_H // 2, 0]])
    add("top", [sp[0, ENG_W // 2]])
    add("right", [sp[ENG_H // 3, ENG_W - 1]])
    add("bottom", [sp[ENG_H - 1, ENG_W // 3]])
    a, b, c = (int(sp[330, 60]), int(sp[330, 75]), int(sp[345, 60]))
    add("duplicates", [a, b, a, b, c, a])
    add("nowhere_high", [a, NOWHERE_ID, c])                    # an id above every id of the map
    add("nowhere_gap", [b, gap_id, c])                         # an id inside the map's range that no pixel has
    for k in range(24):                                        # adjacent: the superpixels of a window of the map
        h, w = int(rng.integers(8, 200)), int(rng.integers(8, 220))
        y, x = int(rng.integers(0, ENG_H - h)), int(rng.integers(0, ENG_W - w))
        ids = np.unique(sp[y:y + h:3, x:x + w:3])
        add("adjacent%d" % k, rng.permutation(ids)[:400])
    for k in range(16):                                        # scattered
        add("scattered%d" % k, rng.choice(present, int(rng.integers(1, 30))))
    return {"name": "mcg_eng_%d" % seed, "superpixels": sp.astype(np.uint16), "labels": labels, "tags": tags, "extents": extents}


def random_image(H, W, cell, n_proposals, n_labels, seed, name=None):
    """A jittered grid with n_proposals unions of ~n_labels superpixels: even ones adjacent (a window of the map), odd ones
    scattered."""
    rng = np.random.default_rng(2000 + seed)
    sp = jittered_grid(H, W, cell, rng)
    k = int(sp.max())
    labels = []
    for i in range(n_proposals):
        if i % 2 == 0:
            side = int(np.ceil(np.sqrt(n_labels))) * cell
            h, w = min(H, int(rng.integers(cell, 2 * side))), min(W, int(rng.integers(cell, 2 * side)))
            y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            ids = rng.permutation(np.unique(sp[y:y + h:2, x:x + w:2]))[:n_labels]
        else:
            ids = rng.integers(1, k + 1, n_labels)
        labels.append([int(j) for j in ids])
    return {"name": name or "mcg_rand_%d" % seed, "superpixels": sp.astype(np.uint16), "labels": labels}


def to_csr(labels):
    """-> (label_ptr int32 [n + 1], label_ids int32)."""
    ptr = np.zeros(len(labels) + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in labels])
    ids = np.array([i for x in labels for i in x], np.int32)
    return ptr, ids


def write_mcg_raw(directory, image):
    """<directory>/<name>.mat in MCG's own shape; -> its path."""
    import scipy.io
    os.makedirs(directory, exist_ok=True)
    cell = np.empty((len(image["labels"]), 1), object)
    for i, x in enumerate(image["labels"]):
        cell[i, 0] = np.asarray(x, np.uint16).reshape(1, -1)
    path = os.path.join(directory, image["name"] + ".mat")
    scipy.io.savemat(path, {"superpixels": np.asarray(image["superpixels"], np.uint16), "labels": cell})
    return path
