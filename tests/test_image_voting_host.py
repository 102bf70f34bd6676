"""Image-space mask voting (cfg.TEST.USE_GPU_MASK_MERGE = False) without a GPU: the fixture's inputs, a numpy restatement of the
kernels' formulation (csrc/mv_image.hip + mv_select_kernel's tie rule) against the reference's outputs, and the public surface."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import golden_inputs as GI  # noqa: E402
import image_voting_inputs as IV  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "reference_image_voting.npz")
CASES = ["small", "full", "ties", "centre", "borders", "many"]
NMS_THRESH, IOU_THRESH, THRESH = 0.3, 0.5, 0.4


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def cases():
    return IV.voting_cases()


def test_fixture_inputs_match_regenerated_inputs(gold, cases):
    assert sorted(cases) == sorted(CASES)
    for tag in CASES:
        assert str(gold["%s_digest" % tag]) == IV.case_digest(cases[tag]), tag
    assert str(gold["tester_digest"]) == IV.tester_digest(GI.tester_net_outputs(GI.sds_case()))


# ---- the kernels' formulation in numpy ------------------------------------------------------------------------------------
def _tie_reversed(sc):
    """mv_select_kernel with tie_reverse: keep-list positions in cpu_mask_voting's order -- the NaN tail reversed first, then
    every run of equal scores of the descending prefix reversed."""
    N = len(sc)
    f = N - int(np.isnan(sc).sum())
    out = list(range(N - 1, f - 1, -1))
    s = 0
    while s < f:
        e = s
        while e < f and sc[e] == sc[s]:
            e += 1
        out.extend(range(e - 1, s - 1, -1))
        s = e
    return np.array(out, np.int64)


def rows_and_candidates(c):
    from oracle import native
    boxes, scores, mpi = c["boxes"], c["scores"], c["max_per_image"]
    kept, pool = [], []
    for k in range(1, IV.K):
        keep = np.array(native.gpu_nms(np.hstack((boxes, scores[:, k:k + 1])), NMS_THRESH), np.int64)  # stable order, full list
        keep = keep[_tie_reversed(scores[keep, k])][:mpi]
        kept.append(keep)
        pool.extend(scores[keep, k])
    thresh = np.sort(np.array(pool, np.float32))[::-1][min(len(pool), mpi) - 1]
    rows = []
    for k in range(1, IV.K):
        for b in kept[k - 1]:
            if scores[b, k] >= thresh:
                ov = native.bbox_overlaps(boxes.astype(np.float64), boxes[b:b + 1].astype(np.float64))[:, 0]
                cand = np.where(ov >= IOU_THRESH)[0]
                w = scores[cand, k]
                w = w / np.float32(sum(w.astype(np.float64)))
                rows.append((b, k, cand, w))
    return rows


def _taps(d, inv, n_src):
    """cv_tap: float64 source coordinate rounded to float32, floor, float32 fraction, clamped."""
    src = ((np.asarray(d, np.float64) + 0.5) * inv - 0.5).astype(np.float32)
    i0 = np.floor(src).astype(np.int64)
    a = (src - i0.astype(np.float32)).astype(np.float32)
    lo = i0 < 0
    a[lo], i0[lo] = 0.0, 0
    hi = i0 >= n_src - 1
    a[hi], i0[hi] = 0.0, n_src - 1
    return i0, np.minimum(i0 + 1, n_src - 1), a


def _inv(dst, src):
    return 1.0 / (float(dst) / float(src))


def _bilinear(get, ty, tx):
    """h0 * (1 - ay) + h1 * ay over h = v(x0) * (1 - ax) + v(x1) * ax, all float32."""
    (y0, y1, ay), (x0, x1, ax) = ty, tx
    one = np.float32(1.0)
    h0 = get(y0, x0) * (one - ax) + get(y0, x1) * ax
    h1 = get(y1, x0) * (one - ax) + get(y1, x1) * ax
    return h0 * (one - ay) + h1 * ay


class Canvas(object):
    """A_r(y, x) = sum over the candidates in order of [pixel in the rounded box] * [resized mask >= float32(thr)] * (double)w."""

    def __init__(self, c, cand, w):
        self.c = c
        self.S = c["masks"].shape[-1]
        rb = np.rint(c["boxes"][cand]).astype(np.int64)
        self.cands = [(rb[j], c["masks"][m, 0], np.float64(w[j])) for j, m in enumerate(cand)]

    def _bin(self, box, mk, dy, dx):
        S = self.S
        ty = _taps(dy, _inv(box[3] - box[1] + 1, S), S)
        tx = _taps(dx, _inv(box[2] - box[0] + 1, S), S)
        return _bilinear(lambda yy, xx: mk[yy, xx], ty, tx) >= np.float32(THRESH)

    def region(self, x0, y0, x1, y1):
        """The canvas on [y0, y1] x [x0, x1] (the bounds scan over the union), each candidate on its own box."""
        acc = np.zeros((y1 - y0 + 1, x1 - x0 + 1))
        for box, mk, wj in self.cands:
            ya, yb, xa, xb = max(box[1], y0), min(box[3], y1), max(box[0], x0), min(box[2], x1)
            if ya > yb or xa > xb:
                continue
            dy, dx = np.meshgrid(np.arange(ya, yb + 1) - box[1], np.arange(xa, xb + 1) - box[0], indexing="ij")
            acc[ya - y0:yb - y0 + 1, xa - x0:xb - x0 + 1] += self._bin(box, mk, dy, dx).astype(np.float64) * wj
        return acc

    def at(self, ys, xs):
        """The canvas at arbitrary pixels (the resampling taps)."""
        acc = np.zeros(ys.shape)
        for box, mk, wj in self.cands:
            inside = (xs >= box[0]) & (xs <= box[2]) & (ys >= box[1]) & (ys <= box[3])
            b = self._bin(box, mk, np.where(inside, ys - box[1], 0), np.where(inside, xs - box[0], 0))
            acc += np.where(inside, b.astype(np.float64) * wj, 0.0)
        return acc


def kernel_restatement(c):
    """-> (boxes [R,5] float64, masks [R,1,S,S] float32, counts [K-1]) as mv_image_bounds / mv_image_resample compute them."""
    H, W, S = c["H"], c["W"], c["masks"].shape[-1]
    out_b, out_m, counts = [], [], np.zeros(IV.K - 1, np.int64)
    for b, k, cand, w in rows_and_candidates(c):
        cv = Canvas(c, cand, w)
        rb = np.rint(c["boxes"][cand]).astype(np.int64)
        ux0, uy0 = max(rb[:, 0].min(), 0), max(rb[:, 1].min(), 0)
        ux1, uy1 = min(rb[:, 2].max(), W - 1), min(rb[:, 3].max(), H - 1)
        r, q = np.where(cv.region(ux0, uy0, ux1, uy1) >= THRESH)
        if len(r):
            bx0, by0, bx1, by1 = ux0 + q.min(), uy0 + r.min(), ux0 + q.max(), uy0 + r.max()
        else:
            bx0 = bx1 = W // 2
            by0 = by1 = H // 2
        ty = _taps(np.arange(S), _inv(S, by1 - by0 + 1), by1 - by0 + 1)
        tx = _taps(np.arange(S), _inv(S, bx1 - bx0 + 1), bx1 - bx0 + 1)
        yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")

        def get(iy, ix):
            return cv.at(by0 + iy[yy], bx0 + ix[xx]).astype(np.float32)

        (y0, y1, ay), (x0, x1, ax) = ty, tx
        one = np.float32(1.0)
        h0 = get(y0, x0) * (one - ax[xx]) + get(y0, x1) * ax[xx]
        h1 = get(y1, x0) * (one - ax[xx]) + get(y1, x1) * ax[xx]
        out_m.append((h0 * (one - ay[yy]) + h1 * ay[yy]).astype(np.float32))
        out_b.append([bx0, by0, bx1, by1, np.float64(c["scores"][b, k])])
        counts[k - 1] += 1
    return (np.array(out_b, np.float64).reshape(-1, 5), np.array(out_m, np.float32).reshape(-1, 1, S, S), counts)


@pytest.mark.parametrize("tag", CASES)
def test_kernel_formulation_reproduces_the_reference(gold, cases, tag):
    boxes, masks, counts = kernel_restatement(cases[tag])
    assert np.array_equal(counts, gold["%s_count" % tag])
    assert np.array_equal(boxes, gold["%s_box" % tag])
    assert np.array_equal(masks, gold["%s_mask" % tag])


def test_fixture_cases_reach_what_they_are_for(gold):
    # ties: rows beyond max_per_image (tied at the threshold), and class 4's tie group cut in reverse keep order
    assert gold["ties_count"].sum() == 6 > 4
    # centre: some result fell back to the Python-2 centre pixel of the odd-sized image
    c = IV.centre_case()
    assert any((b[:4] == [c["W"] // 2, c["H"] // 2, c["W"] // 2, c["H"] // 2]).all() for b in gold["centre_box"])
    # many: every result votes with more candidates than the kernels keep in LDS
    assert gold["many_count"].sum() > 0


# ---- public surface ------------------------------------------------------------------------------------------------------
def test_cpu_mask_voting_has_the_reference_signature():
    import mnc_amd
    mnc_amd.install_paths()
    from transform import mask_transform
    params = list(inspect.signature(mask_transform.cpu_mask_voting).parameters)
    assert params == ["masks", "boxes", "scores", "num_classes", "max_per_image", "im_width", "im_height"]
    from caffeWrapper import TesterWrapper
    assert TesterWrapper.cpu_mask_voting is mask_transform.cpu_mask_voting


def test_new_symbols_are_declared_and_exported():
    from mnc_amd import _lib, engine, native_net
    decls = _lib.parse_header()
    lib = _lib.load()
    for name in ("mnc_mask_voting_image", "mnc_vote_instances_ex", "mnc_net_set_voting"):
        assert name in decls and hasattr(lib, name), name
    assert decls["mnc_mask_voting_image"][2][:10] == ["boxes", "masks", "scores", "n", "num_classes", "mask_size", "max_per_image",
                                                       "nms_thresh", "iou_thresh", "binarize_thresh"]
    assert decls["mnc_vote_instances_ex"][2][:2] == ["ctx", "mode"]
    assert decls["mnc_net_set_voting"][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    assert engine.Net.VOTE_MODES == native_net.NativeNet.VOTING == {"mv": 0, "image": 1}
    assert "mode" in inspect.signature(engine.Net.vote_instances).parameters
    assert "voting" in inspect.signature(native_net.NativeNet.__init__).parameters
    assert "voting" in inspect.signature(native_net.ImageStream.__init__).parameters


def test_host_entry_checks_before_touching_a_device():
    """n == 0 is an empty result and a box that is empty once rounded is an error -- both decided before any HIP call."""
    from mnc_amd import _lib
    lib = _lib.load()
    counts = np.full(20, 7, np.int32)
    R = ctypes.c_int(5)
    rc = lib.mnc_mask_voting_image(None, None, None, 0, 21, 21, 100, ctypes.c_float(0.3), ctypes.c_float(0.5),
                                   ctypes.c_double(0.4), 50, 60, None, None, None, counts.ctypes.data, ctypes.addressof(R), 0)
    assert rc == 0 and R.value == 0 and not counts.any()
    boxes = np.array([[1, 1, 10, 10], [5.7, 3, 4.6, 9]], np.float32)       # x2 rounds below x1
    masks = np.zeros((2, 21, 21), np.float32)
    scores = np.full((2, 21), 0.05, np.float32)
    out = np.zeros((40, 441), np.float32)
    ob = np.zeros((40, 4), np.int32)
    osc = np.zeros(40, np.float32)
    rc = lib.mnc_mask_voting_image(boxes.ctypes.data, masks.ctypes.data, scores.ctypes.data, 2, 21, 21, 100, ctypes.c_float(0.3),
                                   ctypes.c_float(0.5), ctypes.c_double(0.4), 50, 60, out.ctypes.data, ob.ctypes.data,
                                   osc.ctypes.data, counts.ctypes.data, ctypes.addressof(R), 0)
    assert rc == 1 and b"empty once rounded" in lib.mnc_last_error()
