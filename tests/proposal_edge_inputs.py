"""Inputs that sit ON the decisions of the proposal layer, the stage bridge and the detect tail, and the plain statement of each.

mnc_proposal (csrc/proposal.hip) decides more per line than any other entry: two clip bounds per coordinate, a `>=` against the
float32 product min_size * im_scale, a top-K with a defined tie order built twice (one workgroup: radix select + bitonic sort; many
workgroups: sorted runs of kRun keys + rank merge), a power-of-two pad, a survivor gather with two code paths, and np_exp.h's
restated exp.  mnc_stage_bridge adds a first-maximum arg-max over strided rows, mnc_detect_tail a float32 division.  Seeded random
blobs never tie, never land on a bound and never fill a run exactly; the corpora here do:

  1. anchor counts N = H * W * A around kRun (2048), kSelThreads * kKeysPer (24 576) and kRun * kMaxRuns (65 536);
  2. K = min(pre_nms_topn, valid) around 0, 1, the powers of two and the valid count, on a map whose valid count V is chosen;
  3. score sets: all equal, three values with the cut inside the middle class, +-0.0 / denormals / +-inf / negatives, distinct;
  4. decoded sides on min_size * im_scale and its float32 neighbours, coordinates on 0 and im_w - 1 and beyond, dw / dh at the
     cut-offs of the exp;
  5. more than 4096 NMS survivors (the scan's second gather path), and none at all;
  6. stage-bridge rows whose maximum is tied, with strided operands; tail numerators whose quotient differs from the product
     with the reciprocal;
  7. float32 bit patterns for the exp: the whole space thinned, dense around the cut-offs, 0, 1, every quadrant flip and the range
     with denormal results.

The statements are numpy written from the reference lines they cite (lib/pylayer/proposal_layer.py:52-175,
lib/transform/bbox_transform.py:64-130, lib/pylayer/stage_bridge_layer.py:237-255, tools/demo.py:84-100), not calls into the oracle,
and take every argument of the C entry.  Where the reference leaves an order to numpy's unstable sort the header's order holds:
score descending BY VALUE (the two zeros tie), anchor index ascending.  Every statement takes the variations (`mutants`) that
tests/test_proposal_edges_host.py shows the corpora to tell apart; tests/test_gpu_proposal_edges.py runs the library on the same
inputs.  Every comparison is exact.  NaN is no part of any contract here and appears in no input (only in gaps nothing may read)."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FLT_MAX = np.finfo(F32).max

# the constants of csrc/proposal.hip and csrc/nms.hip that the corpora bracket
K_RUN = 2048                   # kRun: keys per sorted run of the multi-workgroup top-K
K_MAX_RUNS = 32                # kMaxRuns: above 65 536 anchors only the single-workgroup kernel runs
K_REG_KEYS = 1024 * 24         # kSelThreads * kKeysPer: keys the single-workgroup kernel holds in registers
K_SORT_CAP = 16384             # kSortCap: the largest pre_nms_topn
K_SURV_CAP = 4096              # kSurvCap: survivors the scan lists in LDS

XMAX = F32(88.72283935546875)              # np_exp.h: x >= XMAX -> +inf
XMIN = F32(-103.97208404541015625)         # np_exp.h: x <= XMIN -> 0


def below(x):
    return np.nextafter(F32(x), F32(-np.inf))


def above(x):
    return np.nextafter(F32(x), F32(np.inf))


# =====================================================================================================================
# The exp of the statements: numpy's own float32 loop
# =====================================================================================================================
def numpy_uses_its_simd_exp():
    """tests/test_np_exp.py's probe: numpy's vector exp differs from the correctly rounded value on ~39 % of inputs."""
    x = np.linspace(-3, 3, 4001, dtype=np.float32)
    return float((np.exp(x) != np.exp(x.astype(np.float64)).astype(np.float32)).mean()) > 0.1


_EXP = []


def exp_reference():
    """-> (exp on float32 arrays, its name): np.exp where numpy runs its own vector loop, else the host build of
    csrc/np_exp.h through tests/np_exp_shim.cpp (bit-identical to that loop, tests/test_np_exp.py); (None, reason) without both."""
    if _EXP:
        return _EXP[0]
    if numpy_uses_its_simd_exp():
        _EXP.append((np.exp, "np.exp (numpy's float32 vector loop)"))
        return _EXP[0]
    cxx = shutil.which("g++")
    if cxx is None:
        _EXP.append((None, "numpy computes exp with libm and there is no g++ for np_exp_shim.cpp"))
        return _EXP[0]
    so = os.path.join(tempfile.mkdtemp(prefix="npexp"), "np_exp_shim.so")
    subprocess.check_call([cxx, "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "np_exp_shim.cpp"),
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.np_exp_f32_array.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]

    def shim_exp(x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        lib.np_exp_f32_array(x.ctypes.data, out.ctypes.data, x.size)
        return out
    _EXP.append((shim_exp, "the host build of csrc/np_exp.h (tests/np_exp_shim.cpp)"))
    return _EXP[0]


def exp_rounded(x):
    """The mutant: the correctly rounded float32 exp."""
    return np.exp(np.asarray(x, np.float64)).astype(F32)


# =====================================================================================================================
# Statements
# =====================================================================================================================
def decode_statement(boxes, deltas, exp, mutants=()):
    """bbox_transform_inv, bbox_transform.py:64-99, in the dtype of the deltas.  mutant: "exp_rounded"."""
    if boxes.shape[0] == 0:
        return np.zeros((0, deltas.shape[1]), dtype=deltas.dtype)
    if "exp_rounded" in mutants:
        exp = exp_rounded
    boxes = boxes.astype(deltas.dtype, copy=False)
    with np.errstate(all="ignore"):
        widths = boxes[:, 2] - boxes[:, 0] + 1.0
        heights = boxes[:, 3] - boxes[:, 1] + 1.0
        ctr_x = boxes[:, 0] + 0.5 * widths
        ctr_y = boxes[:, 1] + 0.5 * heights
        dx, dy, dw, dh = deltas[:, 0::4], deltas[:, 1::4], deltas[:, 2::4], deltas[:, 3::4]
        pcx = dx * widths[:, None] + ctr_x[:, None]
        pcy = dy * heights[:, None] + ctr_y[:, None]
        pw = exp(dw) * widths[:, None]
        ph = exp(dh) * heights[:, None]
        out = np.zeros(deltas.shape, dtype=deltas.dtype)
        out[:, 0::4] = pcx - 0.5 * pw
        out[:, 1::4] = pcy - 0.5 * ph
        out[:, 2::4] = pcx + 0.5 * pw
        out[:, 3::4] = pcy + 0.5 * ph
    assert out.dtype == deltas.dtype
    return out


def clip_statement(boxes, im_h, im_w, mutants=()):
    """clip_boxes, bbox_transform.py:102-120: each coordinate max(min(v, bound - 1), 0), the bound in the caller's type (a
    float32 blob entry for the two layers, an integer for the tail).  mutants: "clip_to_size" (bound, not bound - 1),
    "clip_skips_y2"."""
    off = 0 if "clip_to_size" in mutants else 1
    xb, yb = im_w - off, im_h - off
    out = np.zeros(boxes.shape, dtype=boxes.dtype)
    out[:, 0::4] = np.maximum(np.minimum(boxes[:, 0::4], xb), 0)
    out[:, 1::4] = np.maximum(np.minimum(boxes[:, 1::4], yb), 0)
    out[:, 2::4] = np.maximum(np.minimum(boxes[:, 2::4], xb), 0)
    out[:, 3::4] = boxes[:, 3::4] if "clip_skips_y2" in mutants else np.maximum(np.minimum(boxes[:, 3::4], yb), 0)
    return out


def candidate_order(scores, mutants=()):
    """proposal_layer.py:139 with the header's tie order: score descending by value, anchor index ascending (a stable sort of
    the negated scores: -(+0.0) and -(-0.0) compare equal).  mutants: "ties_by_index_descending", "zeros_by_sign" (every +0.0 in
    front of every -0.0, what an order by bit pattern gives)."""
    s = np.asarray(scores, F32).ravel()
    idx = np.arange(len(s))
    if "ties_by_index_descending" in mutants:
        return np.lexsort((-idx, -s))
    if "zeros_by_sign" in mutants:
        return np.lexsort((idx, np.signbit(s) & (s == 0), -s))
    return np.argsort(-s, kind="stable")


def proposal_statement(c, exp, mutants=(), nms=None):
    """ProposalLayer.forward, proposal_layer.py:52-175 (TEST phase), on a case of this module -> {"boxes", "scores": the sorted
    pre-NMS candidates, "rois" [R, 5], "valid": boxes that pass the size filter, "cut": whether pre_nms_topn cut any off}.
    The NMS step is oracle.native.nms_sorted on the candidates in their order (gpu_nms.pyx sorts them once more, a no-op up to
    ties).  mutants: decode_statement's and clip_statement's, "size_gt" (> for >=), "size_f64" (min_size * im_scale formed and
    compared in float64), candidate_order's, "cut_plus" / "cut_minus" (the cut at pre_nms_topn +- 1)."""
    if nms is None:
        from oracle import native
        nms = native.nms_sorted
    A, H, W = c["A"], c["H"], c["W"]
    im_info = np.asarray(c["im_info"], F32)
    scores = c["prob"][:, A:, :, :]                                                   # :75
    shift_x, shift_y = np.meshgrid(np.arange(0, W) * c["feat_stride"], np.arange(0, H) * c["feat_stride"])
    shifts = np.vstack((shift_x.ravel(), shift_y.ravel(), shift_x.ravel(), shift_y.ravel())).transpose()
    cells = shifts.shape[0]
    anchors = (c["anchors"].reshape((1, A, 4)) + shifts.reshape((1, cells, 4)).transpose((1, 0, 2))).reshape((cells * A, 4))
    deltas = c["deltas"].transpose((0, 2, 3, 1)).reshape((-1, 4))
    scores = scores.transpose((0, 2, 3, 1)).reshape((-1, 1))
    proposals = decode_statement(anchors, deltas, exp, mutants)                          # :121
    proposals = clip_statement(proposals, im_info[0], im_info[1], mutants)               # :124
    ws = proposals[:, 2] - proposals[:, 0] + 1                                           # :132, bbox_transform.py:123-130
    hs = proposals[:, 3] - proposals[:, 1] + 1
    if "size_f64" in mutants:
        thr = np.float64(F32(c["min_size"])) * np.float64(im_info[2])
        ws, hs = ws.astype(np.float64), hs.astype(np.float64)
    else:
        thr = F32(c["min_size"]) * im_info[2]
        assert thr.dtype == F32 and ws.dtype == F32
    keep = np.where(((ws > thr) & (hs > thr)) if "size_gt" in mutants else ((ws >= thr) & (hs >= thr)))[0]
    proposals, scores = proposals[keep, :], scores[keep]
    order = candidate_order(scores, mutants)                                             # :139
    topn = c["pre_nms_topn"]
    if topn > 0:
        topn += ("cut_plus" in mutants) - ("cut_minus" in mutants)
        cut = len(order) > topn
        order = order[:max(topn, 0)]                                                     # :141-142
    else:
        cut = False
    proposals, scores = proposals[order, :], scores[order]
    kept = nms(np.hstack((proposals, scores)), c["nms_thresh"]) if len(order) else np.zeros(0, np.int64)   # :149
    if c["post_nms_topn"] > 0:
        kept = kept[:c["post_nms_topn"]]
    rois = np.hstack((np.zeros((len(kept), 1), F32), proposals[kept, :].astype(F32, copy=False)))        # :159-160
    return {"boxes": proposals, "scores": scores.ravel(), "rois": rois.astype(F32, copy=False), "valid": len(keep), "cut": cut,
            "valid_index": keep}


def stage_bridge_statement(rois, bbox_pred, probs, im_h, im_w, exp, mutants=()):
    """StageBridgeLayer.forward_test, stage_bridge_layer.py:237-255: every class box decoded, the box of argmax(probs) -- numpy's
    argmax, the FIRST maximum, background included -- clipped; built in float64 from float32 values, stored as float32.
    rois [R, 5], bbox_pred [R, 4K], probs [R, K]; im_h, im_w float32.  mutants: decode's and clip's, "argmax_last",
    "argmax_without_background"."""
    R, K = probs.shape
    all_rois = decode_statement(rois[:, 1:5], bbox_pred, exp, mutants)
    if "argmax_last" in mutants:
        score_max = K - 1 - probs[:, ::-1].argmax(axis=1)
    elif "argmax_without_background" in mutants and K > 1:
        score_max = 1 + probs[:, 1:].argmax(axis=1)
    else:
        score_max = probs.argmax(axis=1)
    out = np.zeros((R, 5))
    if R:
        out[:, 1:5] = all_rois[np.arange(R)[:, None], 4 * score_max[:, None] + np.arange(4)[None, :]]
    out[:, 1:5] = clip_statement(out[:, 1:5], F32(im_h), F32(im_w), mutants)
    return out.astype(F32, copy=False)


def detect_tail_statement(rois1, rois2, scale, im_h, im_w, mutants=()):
    """im_detect's tail, tools/demo.py:92-98: rois[:, 1:5] / scale -- a float32 array over a scalar, a float32 division under the
    numpy the reference ran on -- clipped to the image's integer shape, the stages stacked.  mutant: "reciprocal"."""
    s = F32(scale)
    out = []
    for r in (rois1, rois2):
        r = np.asarray(r, F32).reshape(-1, 5)
        b = r[:, 1:5] * (F32(1) / s) if "reciprocal" in mutants else r[:, 1:5] / s
        assert b.dtype == F32
        out.append(clip_statement(b, F32(int(im_h)), F32(int(im_w)), mutants))
    return np.concatenate(out, axis=0)


# =====================================================================================================================
# Cases of mnc_proposal
# =====================================================================================================================
def make_case(name, scores, deltas, A, H, W, anchors, feat_stride, im_info, pre_nms_topn, post_nms_topn=300, nms_thresh=0.7,
              min_size=16.0):
    """scores [N], deltas [N, 4] in anchor order (h, w, a) -> the blobs of the layer: cls_prob [1, 2A, H, W] with the background
    half NaN (never read), bbox_pred [1, 4A, H, W]."""
    N = A * H * W
    scores, deltas = np.asarray(scores, F32).reshape(H, W, A), np.asarray(deltas, F32).reshape(H, W, A * 4)
    prob = np.full((1, 2 * A, H, W), np.nan, F32)
    prob[0, A:] = scores.transpose(2, 0, 1)
    bbox = np.ascontiguousarray(deltas.transpose(2, 0, 1)[None])
    return {"name": name, "prob": prob, "deltas": bbox, "A": A, "H": H, "W": W, "N": N,
            "anchors": np.ascontiguousarray(anchors, F32).reshape(A, 4), "feat_stride": int(feat_stride),
            "im_info": np.asarray(im_info, F32), "pre_nms_topn": int(pre_nms_topn), "post_nms_topn": int(post_nms_topn),
            "nms_thresh": float(nms_thresh), "min_size": float(min_size)}


SCORE_KINDS = ("distinct", "equal", "three", "special")
SPECIAL_SCORES = np.array([0.0, 0.0, 0.0, 1e-40, -1e-40, 1e-45, -1.5, -0.25, 0.75, np.inf, -np.inf], F32)


def score_set(kind, n, valid, K, seed):
    """[n] float32.  "distinct": the control.  "equal": the keys differ in their index half alone, so the low four radix passes
    select.  "three": 0.75 / 0.5 / 0.25 laid out so that the K-th of the valid anchors (index array `valid`) lies inside the 0.5
    class and, where anything is cut, so does the K+1-th.  "special": negatives, denormals, +-inf and zeros whose sign alternates
    from one zero to the next in index order."""
    rng = np.random.default_rng(seed)
    if kind == "distinct":
        return rng.permutation(np.linspace(0.001, 0.999, n)).astype(F32)
    if kind == "equal":
        return np.full(n, 0.5, F32)
    if kind == "three":
        s = rng.choice(np.array([0.25, 0.5, 0.75], F32), n)
        V = len(valid)
        if V >= 3:
            k = min(max(K, 1), V)
            top, mid_end = k // 2, min(V, k + max(1, (V - k + 1) // 2))
            perm = rng.permutation(valid)
            s[perm[:top]], s[perm[top:mid_end]], s[perm[mid_end:]] = 0.75, 0.5, 0.25
        return s
    assert kind == "special"
    s = rng.choice(SPECIAL_SCORES, n)
    zeros = np.flatnonzero(s == 0)
    s[zeros[1::2]] = -0.0
    return s


# ---- 1. anchor counts ----------------------------------------------------------------------------------------------------
ANCHOR_COUNTS = (
    (1, "one key: K = 1, no compare-exchange at all"),
    (63, "one short of a wave"),
    (64, "one wave"),
    (65, "a wave and one key"),
    (135, "the 3 x 5 x 9 map of the engine's smallest image"),
    (2047, "kRun - 1: one sentinel pads the only run"),
    (2048, "kRun: one full run, no sentinel"),
    (2049, "kRun + 1: a second run holding one key"),
    (4096, "2 kRun: two full runs"),
    (24575, "kSelThreads * kKeysPer - 1: one register slot holds the sentinel"),
    (24576, "kSelThreads * kKeysPer: every key in a register, none re-read"),
    (24577, "kSelThreads * kKeysPer + 1: one key re-read from global memory in each of the three loops"),
    (65535, "kRun * kMaxRuns - 1: 32 runs, the last one padded"),
    (65536, "kRun * kMaxRuns: the largest map of the multi-workgroup top-K"),
    (65537, "kRun * kMaxRuns + 1: the single-workgroup kernel whatever the setting"),
)
COUNT_STRIDE, COUNT_SIDE = 4, 24


def has_wide_path(N):
    return (N + K_RUN - 1) // K_RUN <= K_MAX_RUNS


def count_case(N, kind="distinct", pre_nms_topn=6000, post_nms_topn=300, seed=None):
    """A = 1, a 1 x N map at stride 4 of one 24 x 24 anchor (coordinates below 2^19); a seeded fifth of the anchors has dw = -1 and
    shrinks to 24 / e + 1, under min_size = 16 whatever exp is used, every other delta is 0 (exp(0) == 1: the box is the anchor
    with one more column and row, bbox_transform_inv's x2 = x1 + width).  Neighbours overlap at IoU 525 / 725 > 0.7, so the NMS
    works."""
    rng = np.random.default_rng(N if seed is None else seed)
    deltas = np.zeros((N, 4), F32)
    small = rng.random(N) < 0.2
    deltas[small, 2] = -1.0
    valid = np.flatnonzero(~small)
    K = min(pre_nms_topn if pre_nms_topn > 0 else N, len(valid))
    scores = score_set(kind, N, valid, K, N + 7)
    c = make_case("N=%d %s topn=%d" % (N, kind, pre_nms_topn), scores, deltas, 1, 1, N, [[0, 0, COUNT_SIDE - 1, COUNT_SIDE - 1]],
                  COUNT_STRIDE, (COUNT_SIDE, COUNT_STRIDE * N + COUNT_SIDE, 1.0), pre_nms_topn, post_nms_topn)
    c["expect_valid"] = len(valid)
    return c


def count_cases():
    """Every N of ANCHOR_COUNTS with distinct scores; the tied score sets at three of the sizes with the cut at 1, 2^10 + 1 and
    6000; pre_nms_topn at the documented limit 16384 with more valid anchors than that."""
    out = [count_case(N) for N, _ in ANCHOR_COUNTS]
    for N in (2049, 24577, 65537):
        for kind in SCORE_KINDS[1:]:
            for topn in (1, 1025, 6000):
                out.append(count_case(N, kind, topn))
    out.append(count_case(24577, "distinct", K_SORT_CAP))
    out.append(count_case(24577, "equal", K_SORT_CAP))
    return out


def refused_cases():
    """pre_nms_topn above kSortCap after the clamp to N: MNC_ERR_INVALID, nothing launched."""
    return [count_case(24577, "distinct", K_SORT_CAP + 1), count_case(24577, "distinct", 0), count_case(24577, "distinct", -1)]


# ---- 2. K = min(pre_nms_topn, valid) -----------------------------------------------------------------------------------------
K_MAP_W = 2100                                               # N = 4200
K_MAP_N = 2 * K_MAP_W
K_V = 1500
K_TOPNS = (-1, 0, 1, 2, 63, 64, 65, 1023, 1024, 1025, K_V - 1, K_V, K_V + 1, K_MAP_N, K_MAP_N + 1)
K_V_SWEEPS = tuple((topn, V) for topn in (64, 1024) for V in (0, 1, topn - 1, topn, topn + 1))


def k_valid(V):
    """Anchor indices that pass the filter of k_case(V): anchor 0 of the first V columns."""
    return 2 * np.arange(V)


def k_case(V, pre_nms_topn, kind="distinct", post_nms_topn=300):
    """One 1 x 2100 map at stride 16 with A = 2 integer anchors and zero deltas (exp(0) == 1; the decoded box is x1 .. x1 + width):
    a 15 x 15 anchor, whose box is exactly min_size = 16 wide, and a 14 x 14 one, always under it.  The image is 16 V pixels wide:
    the clip leaves the 16 x 16 box of column V - 1 whole and cuts that of column V to one pixel, so exactly V anchors, the even
    indices below 2 V, pass the filter (V = 0: 8 pixels)."""
    N = K_MAP_N
    valid = k_valid(V)
    K = min(pre_nms_topn if pre_nms_topn > 0 else N, V)
    scores = score_set(kind, N, valid, K, 1000 * V + (pre_nms_topn % 997))
    c = make_case("V=%d topn=%d %s" % (V, pre_nms_topn, kind), scores, np.zeros((N, 4), F32), 2, 1, K_MAP_W,
                  [[0, 0, 14, 14], [0, 0, 13, 13]], 16, (64, 16 * V if V else 8, 1.0), pre_nms_topn, post_nms_topn)
    c["expect_valid"], c["expect_K"] = V, K
    return c


def k_cases():
    out = []
    for kind in SCORE_KINDS:
        out += [k_case(K_V, topn, kind) for topn in K_TOPNS]
        out += [k_case(V, topn, kind) for topn, V in K_V_SWEEPS]
    return out


# ---- 4. the decode's rules ----------------------------------------------------------------------------------------------------
MIN_SIZE_ODD = 12.3                                           # no power of two; float32(12.3) * 1.6f rounds DOWN in float32
DECODE_SCALES = (F32(1), above(1), F32(1.6))


def _decode_case(name, anchors, deltas, im_h, im_w, scale, min_size):
    """H = W = 1: every anchor is one case, in score order."""
    A = len(anchors)
    assert A <= 16
    scores = 1.0 - np.arange(A) / 32.0
    return make_case(name, scores, np.asarray(deltas, F32).reshape(A, 4), A, 1, 1, anchors, 16, (im_h, im_w, scale), 6000, 300, 0.7,
                     min_size)


def threshold_case(scale):
    """Anchors (0, 0, t - 2, 63) with zero deltas decode to (0, 0, t - 1, 64), a width of exactly t (every step is exact: see the host test), for t
    the float32 below, on and above float32(min_size) * float32(im_scale); the same on the height; and both sides on it."""
    thr = F32(MIN_SIZE_ODD) * F32(scale)
    ts = (below(thr), thr, above(thr))
    two = F32(2)
    anchors = [[0, 0, t - two, 63] for t in ts] + [[0, 0, 63, t - two] for t in ts] + [[0, 0, thr - two, thr - two]]
    c = _decode_case("side on min_size * %r" % float(scale), anchors, np.zeros((7, 4), F32), 128, 128, scale, MIN_SIZE_ODD)
    c["sides"] = [(t, F32(65)) for t in ts] + [(F32(65), t) for t in ts] + [(thr, thr)]
    c["thr"] = thr
    return c


CLIP_H, CLIP_W = 100, 200
POINT_ANCHOR = [-0.5, -0.5, -0.5, -0.5]                       # width 1, centre 0: with exp(dw) == 0 the box is the point (dx, dy)
UNDERFLOW = -200.0                                            # exp(-200) == 0 in every exp


def clip_cases():
    """min_size = 1 so that nothing is filtered.  Points (dx, dy) through the unit anchor with exp underflowing to 0: the
    coordinate is any float32 we choose -- on the bound, one float32 step either side of it, on 0, one step either side, far out
    and infinite; then whole integer boxes on and over each edge."""
    out = []
    for axis, bound in ((0, CLIP_W - 1), (1, CLIP_H - 1)):
        vals = [bound, above(bound), below(bound), bound + 1, 0.0, 1e-45, -1e-45, -1.0, 1e30, -1e30, np.inf, -np.inf]
        deltas = np.zeros((len(vals), 4), F32)
        deltas[:, 2:] = UNDERFLOW
        deltas[:, 1 - axis] = 50
        deltas[:, axis] = vals
        c = _decode_case("points along %s" % "xy"[axis], [POINT_ANCHOR] * len(vals), deltas, CLIP_H, CLIP_W, 1.0, 1.0)
        c["points"] = deltas[:, :2].copy()
        out.append(c)
    W, H = CLIP_W, CLIP_H
    boxes = [[W - 16, 0, W - 1, 15], [W - 15, 0, W, 15], [0, H - 16, 15, H - 1], [0, H - 15, 15, H], [-1, 0, 14, 15], [0, -1, 15, 14],
             [-300, -300, -250, -250], [400, 300, 450, 350], [-300, 20, 500, 40], [20, -300, 40, 500], [0, 0, W - 1, H - 1]]
    anchors = np.array(boxes, F32) - np.array([0, 0, 1, 1], F32)          # zero deltas decode (x1, y1, x2, y2) to (x1, y1, x2 + 1, y2 + 1)
    c = _decode_case("integer boxes on the edges", anchors, np.zeros((len(boxes), 4), F32), H, W, 1.0, 1.0)
    c["decoded"] = np.array(boxes, F32)
    out.append(c)
    return out


EXP_EDGES = (below(XMAX), XMAX, above(XMAX), below(XMIN), XMIN, above(XMIN))


def exp_edge_case():
    """dw and dh at the cut-offs of the exp and their neighbours, on the unit anchor (x2 = 0.5 * exp, finite up to the cut-off)
    and on a 4 x 4 anchor centred on 0 (x2 = 2 * exp, exact for the denormal results above the lower cut-off); dw and dh take the
    edges in opposite order.  The image is as large as float32 goes, so only infinity is clipped."""
    anchors = [POINT_ANCHOR] * 6 + [[-2, -2, 1, 1]] * 6
    deltas = np.zeros((12, 4), F32)
    deltas[:, 2] = EXP_EDGES * 2
    deltas[:, 3] = (EXP_EDGES * 2)[::-1]
    return _decode_case("dw, dh at the exp cut-offs", anchors, deltas, FLT_MAX, FLT_MAX, 1.0, 1.0)


def decode_cases():
    return [threshold_case(s) for s in DECODE_SCALES] + clip_cases() + [exp_edge_case()]


# ---- 5. the scan's gather paths ----------------------------------------------------------------------------------------------------
SCAN_H, SCAN_W = 50, 100                                     # 5000 disjoint 16 x 16 boxes (15 x 15 anchors): all survive the NMS


def scan_case(post_nms_topn, min_size=16.0):
    """post_nms_topn = 4097 (and anything above): min(max_keep, candidates) > kSurvCap, the scan gathers through `keep`; 4096: through
    its LDS list.  min_size = 17 filters every box."""
    N = SCAN_H * SCAN_W
    scores = score_set("distinct", N, None, 0, 5)
    c = make_case("scan post=%d min=%g" % (post_nms_topn, min_size), scores, np.zeros((N, 4), F32), 1, SCAN_H, SCAN_W,
                  [[0, 0, 14, 14]], 16, (16 * SCAN_H, 16 * SCAN_W, 1.0), 6000, post_nms_topn, 0.7, min_size)
    c["expect_valid"] = N if min_size <= 16 else 0
    return c


SCAN_POSTS = (K_SURV_CAP, K_SURV_CAP + 1, 6000)


# ---- sequence on one context ----------------------------------------------------------------------------------------------------
SEQUENCE = (65537, 135, 2049)


# =====================================================================================================================
# Stage bridge
# =====================================================================================================================
BRIDGE_KS = (1, 2, 21, 64)
BRIDGE_RS = (0, 1, 63, 64, 65, 300)
BRIDGE_H, BRIDGE_W = 600, 1000


def bridge_case(R, K, seed=0):
    """rois [R, 5] inside and over a 600 x 1000 image, deltas N(0, 0.3) [R, 4K], probabilities [R, K]: row r has its maximum tied
    at positions (0, k) for r % 4 == 0, at (k, K - 1) for r % 4 == 1, all entries equal for r % 4 == 2 and a seeded softmax
    otherwise.  Both operands are column slices of wider arrays (ld = 4K + 3 and K + 5) whose other columns are NaN."""
    rng = np.random.default_rng(1000 * K + R + seed)
    x1, y1 = rng.uniform(-40, BRIDGE_W - 64, R), rng.uniform(-40, BRIDGE_H - 64, R)
    rois = np.zeros((R, 5), F32)
    rois[:, 1:] = np.stack([x1, y1, x1 + rng.uniform(8, 500, R), y1 + rng.uniform(8, 400, R)], 1)
    ld_bbox, ld_probs = 4 * K + 3, K + 5
    wide_bbox, wide_probs = np.full((R, ld_bbox), np.nan, F32), np.full((R, ld_probs), np.nan, F32)
    wide_bbox[:, :4 * K] = rng.normal(0, 0.3, (R, 4 * K))
    e = np.exp(rng.normal(0, 2.0, (R, K)))
    p = (e / e.sum(axis=1, keepdims=True)).astype(F32)
    for r in range(R if K > 1 else 0):
        if r % 4 == 0:
            p[r] = 0.25 / K
            p[r, [0, int(rng.integers(1, K))]] = 0.5
        elif r % 4 == 1:
            p[r] = 0.25 / K
            p[r, [int(rng.integers(0, K - 1)), K - 1]] = 0.5
        elif r % 4 == 2:
            p[r] = F32(1.0) / F32(K)
    wide_probs[:, :K] = p
    return {"name": "R=%d K=%d" % (R, K), "rois": rois, "bbox": wide_bbox, "probs": wide_probs, "ld_bbox": ld_bbox, "ld_probs": ld_probs,
            "R": R, "K": K, "im_h": F32(BRIDGE_H), "im_w": F32(BRIDGE_W)}


def bridge_from_decode(c):
    """A decode case on the roi side: rois = its anchors, K = 2 with both classes carrying its deltas and tied probabilities."""
    A = c["A"]
    rois = np.zeros((A, 5), F32)
    rois[:, 1:] = c["anchors"]
    d = c["deltas"].reshape(A, 4)
    wide_bbox, wide_probs = np.full((A, 11), np.nan, F32), np.full((A, 7), np.nan, F32)
    wide_bbox[:, :4], wide_bbox[:, 4:8] = d, d
    wide_probs[:, :2] = 0.5
    return {"name": "decode: " + c["name"], "rois": rois, "bbox": wide_bbox, "probs": wide_probs, "ld_bbox": 11, "ld_probs": 7, "R": A,
            "K": 2, "im_h": c["im_info"][0], "im_w": c["im_info"][1]}


def bridge_cases():
    return [bridge_case(R, K) for K in BRIDGE_KS for R in BRIDGE_RS] + [bridge_from_decode(c) for c in decode_cases()]


def bridge_statement_of(c, exp, mutants=()):
    K = c["K"]
    return stage_bridge_statement(c["rois"], c["bbox"][:, :4 * K], c["probs"][:, :K], c["im_h"], c["im_w"], exp, mutants)


# =====================================================================================================================
# Detect tail
# =====================================================================================================================
TAIL_H, TAIL_W = 375, 500
TAIL_SCALES = (("1", F32(1)), ("1.6f", F32(1.6)), ("0.8f", F32(0.8)), ("600/375", F32(600.0 / 375.0)), ("1/3", F32(1.0 / 3.0)))


def search_tail_numerators(scale, count=8):
    """The first `count` of x = float32(0.37 k), k = 22, 23, ... (full mantissas between 8 and a few hundred) with
    x / s != x * (1 / s) in float32.  Short mantissas do not serve: 1 / 1.6f rounds to 0.625 and multiples of 1/8 then give the same
    float32 both ways.  This is how TAIL_NUMERATORS was made; the tests read the table and do not search."""
    s = F32(scale)
    x = (np.arange(22, 4096) * 0.37).astype(F32)
    return tuple(float(v) for v in x[(x / s) != (x * (F32(1) / s))][:count])


# {name: search_tail_numerators(scale)}.  A division by 1 is a multiplication by 1; float32(600 / 375) is 1.6f over again (the
# scale of a 375-row image), and 0.8f = 1.6f / 2 differs from it by a power of two, hence the three equal rows.
_TAIL_16 = (8.510000228881836, 12.579999923706055, 15.90999984741211, 17.020000457763672, 24.049999237060547, 25.15999984741211,
            31.81999969482422, 34.040000915527344)
TAIL_NUMERATORS = {
    "1": (),
    "1.6f": _TAIL_16,
    "0.8f": _TAIL_16,
    "600/375": _TAIL_16,
    "1/3": (8.140000343322754, 9.619999885559082, 11.100000381469727, 12.210000038146973, 13.6899995803833, 14.800000190734863,
            15.170000076293945, 16.280000686645508),
}


def tail_rows(name):
    """rois [n, 5] for one scale: the table's numerators; coordinates whose quotient lands on W - 1 / H - 1 exactly, the float32
    steps around them, a pixel beyond, far beyond; 0 and negatives."""
    s = dict(TAIL_SCALES)[name]
    vals = list(TAIL_NUMERATORS[name])
    for bound in (TAIL_W - 1, TAIL_H - 1):
        on = F32(bound) * s
        near = on.view(np.uint32) + np.arange(-8, 9, dtype=np.int64)    # a float32 whose quotient IS the bound, where one exists
        near = near.astype(np.uint32).view(F32)
        on = near[near / s == bound][0] if (near / s == bound).any() else on
        vals += [on, below(on), above(on), below(below(on)), above(above(on)), F32(bound + 1) * s, F32(4 * bound)]
    vals += [0.0, -0.0, -1.0, -1e-3, -700.0, 1e-45, 3.5]
    vals = np.array(vals, F32)
    n = len(vals)
    rois = np.zeros((n, 5), F32)
    for k in range(4):                                        # every value in every column
        rois[:, 1 + k] = np.roll(vals, 5 * k)
    return rois


TAIL_COUNTS = ((0, 7), (7, 0), (1, 1), (300, 300), (0, 0))


def tail_case(name, R1, R2):
    rows = tail_rows(name)
    pick = lambda R, off: rows[(np.arange(R) + off) % len(rows)]
    return pick(R1, 0), pick(R2, 11)


# =====================================================================================================================
# The exp sweep: float32 bit patterns
# =====================================================================================================================
LOG2E = 1.442695040888963407359924681001892137
SWEEP_CHUNK = 1 << 21


def exp_sweep_patterns():
    """uint32 bit patterns, sorted, NaN removed (NaN is outside every contract here): every 1024th of the whole space; every one
    within 4096 of XMAX, XMIN, +0, -0 and 1; within 64 of each half-integer of x * log2(e) between the quotients -151 and 129,
    where `quadrant` flips; every 4th of [-103.98, -87.3], where ldexpf returns denormals."""
    parts = [np.arange(0, 1 << 32, 1024, dtype=np.int64)]
    for c in (XMAX, XMIN, F32(0.0), F32(-0.0), F32(1)):
        b = int(np.array(c, F32).view(np.uint32))
        parts.append(np.arange(max(b - 4096, b & 0x80000000), b + 4097, dtype=np.int64))
    halves = ((np.arange(-151, 129) + 0.5) / LOG2E).astype(F32).view(np.uint32).astype(np.int64)
    parts.append((halves[:, None] + np.arange(-64, 65)[None, :]).ravel())
    lo, hi = (int(np.array(v, F32).view(np.uint32)) for v in (-87.3, -103.98))
    parts.append(np.arange(lo, hi + 1, 4, dtype=np.int64))
    bits = np.unique(np.concatenate(parts)).astype(np.uint32)
    return bits[(bits & np.uint32(0x7FFFFFFF)) <= np.uint32(0x7F800000)]


SWEEP_ROIS = ((0.0, 0.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0))    # x2 == exp(d2) while 2 * exp is finite; x2 == 0.5 * exp


def sweep_rows(x, roi):
    """mnc_stage_bridge operands with K = 1 for the float32 values x: roi (0, roi), d = (-0.5, -0.5, x, x), probability 1."""
    n = len(x)
    rois = np.zeros((n, 5), F32)
    rois[:, 1:] = roi
    d = np.empty((n, 4), F32)
    d[:, :2] = -0.5
    d[:, 2], d[:, 3] = x, x
    return rois, d, np.ones((n, 1), F32)
