"""Shared corpus of tests/test_losses_host.py and tests/test_gpu_losses.py: inputs of the three loss layers and of the activation
backward passes (mnc_amd/losses.py), their statements' results computed once, and the constants of the tolerances.

The shapes are the smallest at which each path of csrc/loss.hip can go wrong: not a multiple of 64, more than one outer index,
exactly one wave, one position; rows shorter than, equal to and longer than a wave, more than two chunks, the limit C = 4096, and
the head's 300 rows (more than one workgroup)."""
import functools

import numpy as np

from mnc_amd import losses as L

# The ulp bound of the device's logf.  No table of ulp bounds ships with ROCm 7.2 (its share/doc/hip holds the runtime API
# reference only).  hipcc's logf is ROCm-Device-Libs' __ocml_log_f32, which targets the OpenCL C specification's accuracy table
# (OpenCL 3.0 C, 7.4 "Relative error as ULPs": log <= 3 ulp in single precision); the constant is that published bound, not a
# measurement of the kernel.
LOGF_ULP = 3.0
FINAL_OP_ULP = 1.0          # the rounding of the operations behind the logarithm (the sigmoid term's subtraction and multiply)

IGNORE = -1

SOFTMAX_POS_SHAPES = ((1, 2, 135), (2, 2, 65), (1, 2, 64), (1, 3, 1))                 # (outer, C, inner), inner > 1 but for the last
SOFTMAX_ROW_SHAPES = ((5, 1), (5, 2), (7, 21), (3, 63), (3, 64), (3, 65), (2, 130), (1, 4096), (300, 21))   # (rows, C)
SOFTMAX_SHAPES = SOFTMAX_POS_SHAPES + tuple((r, c, 1) for r, c in SOFTMAX_ROW_SHAPES)
# (score kind, label kind): every label kind on normal scores, the two special score kinds on mixed labels
SOFTMAX_KINDS = (("normal", "mixed"), ("normal", "all_ignored"), ("normal", "none_ignored"), ("normal", "no_ignore_minus1"),
                 ("normal", "bad"), ("equal", "mixed"), ("pm80", "mixed"))
SOFTMAX_KEYS = ["%dx%dx%d-%s-%s" % (s + k) for s in SOFTMAX_SHAPES for k in SOFTMAX_KINDS]
BAD_LABELS = (np.nan, 0.5, 3.0e9, -2.0, -3.0e9, np.inf)             # plus C itself: invalid under any ignore_label


@functools.lru_cache(maxsize=None)
def softmax_case(key):
    """-> dict(score [outer,C,inner], label [outer,inner] as given to the device, has_ignore, normalize, loss_weight, status = the
    status word expected, ref_label = the labels with every invalid one replaced by IGNORE: what the statements are given)."""
    shape, skind, lkind = key.split("-")
    outer, C, inner = (int(v) for v in shape.split("x"))
    rng = np.random.default_rng(outer * 100003 + C * 101 + inner + 17 * len(skind) + len(lkind))
    npos = outer * inner
    if skind == "normal":
        score = rng.standard_normal((outer, C, inner)) * 3.0
    elif skind == "equal":
        score = np.repeat(rng.standard_normal((outer, 1, inner)) * 3.0, C, axis=1)
    else:
        score = np.where(rng.random((outer, C, inner)) < 0.5, 80.0, -80.0)
    label = rng.integers(0, C, npos).astype(np.float32)
    ref = None
    has_ignore, normalize, weight = 1, True, 1.0
    if lkind in ("mixed", "bad"):
        label[rng.random(npos) < 0.3] = IGNORE
        if npos > 1:
            label[0], label[-1] = IGNORE, C - 1
    elif lkind == "all_ignored":
        label[:] = IGNORE
    elif lkind == "none_ignored":
        normalize, weight = False, 0.5
    elif lkind == "no_ignore_minus1":
        has_ignore, weight = 0, 2.0
        label[::3] = IGNORE                                           # not an ignore label here: invalid
        ref = label.copy()
    if lkind == "bad":
        bad = BAD_LABELS + (float(C),)
        ref = label.copy()
        for j, p in enumerate(range(0, npos, 2)):
            label[p], ref[p] = bad[j % len(bad)], IGNORE
    status = int(lkind in ("bad", "no_ignore_minus1"))           # position 0 holds an invalid label in both
    case = {"score": score.astype(np.float32), "label": label.reshape(outer, inner), "has_ignore": has_ignore, "normalize": normalize,
            "loss_weight": weight, "status": status, "ref_label": (label if ref is None else ref).reshape(outer, inner)}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def softmax_ref(key):
    """(float32 statement, float64 form) on ref_label with ignore_label = IGNORE; computed once, never changed."""
    c = softmax_case(key)
    out = tuple(f(c["score"], c["ref_label"], IGNORE, c["normalize"], c["loss_weight"]) for f in (L.softmax_loss_numpy, L.softmax_loss_f64))
    for r in out:
        for a in (r.terms, r.grad, r.prob):
            a.setflags(write=False)
    return out


def softmax_log_argument(key):
    """The float32 argument of the statement's logarithm at every position, and the valid mask: max(p_label, FLT_MIN)."""
    c, (r32, _) = softmax_case(key), softmax_ref(key)
    outer, C, inner = c["score"].shape
    valid, _, _, idx = L.classify_labels(c["ref_label"], C, IGNORE)
    p_label = np.take_along_axis(r32.prob.reshape(outer, C, inner), idx[:, None, :], 1)[:, 0, :]
    return np.maximum(p_label, L.FLT_MIN), valid


def softmax_term_reference(key):
    """-> float64 [outer, inner]: minus the float64 log of the statement's own float32 argument; 0 where not valid."""
    arg, valid = softmax_log_argument(key)
    return np.where(valid, -np.log(arg.astype(np.float64)), 0.0)


def ulp_error(got, ref64):
    """|got - ref64| in ulps of ref64 rounded to float32, elementwise (0 where both are zero)."""
    ref64 = np.asarray(ref64, np.float64)
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(ref64.astype(np.float32))).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - ref64) / ulp


# ---- SmoothL1
SMOOTH_KEYS = ("rpn", "head", "dyadic", "edges")


@functools.lru_cache(maxsize=None)
def smooth_case(key):
    """-> dict(pred, target, w_in, w_out, sigma, loss_weight)."""
    rng = np.random.default_rng(len(key) + 40)
    f = np.float32
    if key in ("rpn", "head"):
        shape, sigma, weight = ((1, 36, 3, 5), 3.0, 1.0) if key == "rpn" else ((7, 84), 1.0, 2.0)
        pred, target = rng.standard_normal(shape) * 0.7, rng.standard_normal(shape) * 0.7
        w_in = rng.choice([0.0, 1.0], shape)
        w_out = rng.choice([0.0, 1.0 / 64, 0.3], shape)
    elif key == "dyadic":                                             # nothing rounds: multiples of 1/8, sigma 2, weights 0, 0.5, 1
        shape, sigma, weight = (4, 24), 2.0, 1.0
        pred, target = rng.integers(-16, 17, shape) / 8.0, rng.integers(-16, 17, shape) / 8.0
        w_in, w_out = rng.choice([0.0, 0.5, 1.0], shape), rng.choice([0.0, 0.5, 1.0], shape)
    else:                                                             # d on and around the threshold of sigma 3, and the zero weights
        sigma, weight = 3.0, 1.0
        thr = f(1) / (f(3) * f(3))
        d = np.array([0.0, thr, -thr, np.nextafter(thr, f(0)), np.nextafter(thr, f(1)), -np.nextafter(thr, f(0)),
                      -np.nextafter(thr, f(1)), -0.0, 0.05, 0.05, 2.0, 2.0, 0.05, 2.0, -2.0, 1.0], f).reshape(2, 8)
        pred, target = d, np.zeros((2, 8))
        w_in, w_out = np.ones((2, 8)), np.ones((2, 8))
        w_in[1, 0], w_in[1, 2] = 0.0, 0.0                             # inside weight 0, outside weight non-zero
        w_out[1, 1], w_out[1, 3] = 0.0, 0.0                           # and the reverse
        w_out[1, 4:] = 0.75
    case = {"pred": f(pred), "target": f(target), "w_in": f(w_in), "w_out": f(w_out), "sigma": sigma, "loss_weight": weight}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def smooth_args(c):
    return c["pred"], c["target"], c["w_in"], c["w_out"], c["sigma"], c["loss_weight"]


@functools.lru_cache(maxsize=None)
def smooth_ref(key):
    out = tuple(f(*smooth_args(smooth_case(key))) for f in (L.smooth_l1_loss_numpy, L.smooth_l1_loss_f64))
    for r in out:
        r.terms.setflags(write=False)
        r.grad.setflags(write=False)
    return out


# ---- SigmoidCrossEntropy
SIGMOID_KEYS = ("mask", "no_weight", "tiny")
SIGMOID_SPECIALS = (0.0, 100.0, -100.0, 88.8, -0.0, -88.8)


@functools.lru_cache(maxsize=None)
def sigmoid_case(key):
    """-> dict(x [N, D], t, w or None, loss_weight)."""
    rng = np.random.default_rng(77)
    if key == "tiny":
        x, t, w, weight = np.array([[0.3, -1.2, 4.0]]), np.array([[1.0, 0.0, 1.0]]), np.array([[1.0, 0.5, 0.0]]), 1.0
    else:
        x = rng.standard_normal((6, 441)) * 3.0
        x[:, :6] = SIGMOID_SPECIALS                                   # in every row: under weight 1 and under weight 0
        t = (rng.random((6, 1, 21, 21)) < 0.4).astype(np.float32)
        w = np.repeat(np.array([1, 1, 1, 1, 0, 0], np.float32), 441).reshape(6, 1, 21, 21) if key == "mask" else None
        weight = 1.0 if key == "mask" else 3.0
    case = {"x": np.float32(x), "t": np.float32(t), "w": None if w is None else np.float32(w), "loss_weight": weight}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def sigmoid_args(c):
    return c["x"], c["t"], c["w"], c["loss_weight"]


@functools.lru_cache(maxsize=None)
def sigmoid_ref(key):
    out = tuple(f(*sigmoid_args(sigmoid_case(key))) for f in (L.sigmoid_ce_loss_numpy, L.sigmoid_ce_loss_f64))
    for r in out:
        r.terms.setflags(write=False)
        r.grad.setflags(write=False)
    return out


def sigmoid_term_reference(key):
    """-> float64, x's shape: the statement's term with the float64 log of its own float32 argument 1 + exp(x - 2 x pos); the
    float32 operands x * (t - pos) and w are the statement's, the subtraction and the product are exact."""
    c = sigmoid_case(key)
    x = c["x"]
    t = c["t"].reshape(x.shape)
    w = np.ones(x.shape, np.float32) if c["w"] is None else c["w"].reshape(x.shape)
    pos = (x >= 0).astype(np.float32)
    arg = np.float32(1) + np.exp(x - np.float32(2) * x * pos)
    return -((x * (t - pos)).astype(np.float64) - np.log(arg.astype(np.float64))) * w.astype(np.float64)


# ---- ReLU / Sigmoid backward
ELTWISE_COUNTS = (1, 63, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def eltwise_case(count):
    """-> (y, dy): y holds -0.0, 0.0 and 1.0 (as far as count goes) among values on both sides of zero."""
    rng = np.random.default_rng(count)
    y = rng.uniform(-1.0, 1.5, count).astype(np.float32)
    y[:3] = np.array([-0.0, 0.0, 1.0], np.float32)[:count]
    dy = rng.standard_normal(count).astype(np.float32)
    y.setflags(write=False)
    dy.setflags(write=False)
    return y, dy


def loss_bound(f64, per_term_ulps=0.0):
    """The most any float32 evaluation of the loss may differ from the float64 form f64: (n_terms + 32) * 2^-24 * sum|term|, plus
    per_term_ulps float32 ulps of every term (the allowance of the logarithm), all over the normaliser."""
    ulps = float(np.spacing(np.abs(np.asarray(f64.terms, np.float32))).astype(np.float64).sum()) if per_term_ulps else 0.0
    return ((f64.n_terms + 32.0) * 2.0 ** -24 * f64.abs_sum + per_term_ulps * ulps) / max(float(f64.normalizer), 1.0)
