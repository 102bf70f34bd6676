"""The loss layers that end the five stages of models/VGG16/mnc_5stage/train.prototxt, and the two activation backward passes
behind them (include/mnc_hip.h n25, csrc/loss.hip): the value of every loss and its gradient with respect to the prediction.

    softmax_loss_numpy(score, label, ignore_label=None, normalize=True, loss_weight=1.0)   the float32 statement -> LossResult
    softmax_loss_f64(...)                                     the float64 form (adds abs_sum, n_terms)
    softmax_loss(..., device_id=None)                         the same through mnc_softmax_loss (the GPU)
    smooth_l1_loss_numpy(pred, target, w_in, w_out, sigma=1.0, loss_weight=1.0) / _f64 / smooth_l1_loss
    sigmoid_ce_loss_numpy(x, t, w=None, loss_weight=1.0) / _f64 / sigmoid_ce_loss
    eltwise_backward_numpy(y, dy, op) / eltwise_backward      op "relu" (1) or "sigmoid" (2); y is the layer's OUTPUT
    softmax_plan(plan)                                        mnc_softmax_loss_plan: 0 by shape, 1 positions, 2 rows

A LossResult has loss (the unweighted loss, Caffe's top), terms, grad (already times loss_weight / normaliser), count,
normalizer, and prob for the softmax (None otherwise); the float64 forms add abs_sum, the float64 sum of |term|, and n_terms,
the number of terms, for the worst-case bound of any float32 evaluation of the loss:
|float32 loss - float64 loss| <= (n_terms + 32) * 2^-24 * abs_sum / normaliser.

Arrays are Caffe's blobs: score [outer, C, ...] with one label per position ([1, 2, 9H, W] with [1, 1, 9H, W]; [R, 21] with [R] or
[R, 1]), the softmax over axis 1; SmoothL1's four bottoms of one shape; x [R, 441] against t [R, 1, 21, 21] and an optional weight
of the same count.  N = shape[0].  There is no fallback: without the library or a GPU the device functions raise; what the library
refuses as MNC_ERR_INVALID, and a status bit in the result, is a ValueError.

The rules are public BVLC Caffe's and py-faster-rcnn's; caffe-mnc's own layer sources are not available.  What those sources
leave open is marked CHOICE.  All inputs are float32; the float32 statements evaluate operation by operation in the
order written, exp is numpy's float32 exp (csrc/np_exp.h restates it for the device): the device's prob, SmoothL1 terms and every
gradient are the statement's bits.  The terms of the softmax and of the sigmoid loss go through log, where the device's logf is
not numpy's: those agree within a few ulps.

    SoftmaxWithLoss   score [outer, C, inner], label [outer, inner].  m = max_c score; e_c = exp(score_c - m); s = the sum of e_c
                      in ASCENDING c, starting from +0.0; p_c = e_c / s.  li = (int)label.  A position is ignored when li ==
                      ignore_label (CHOICE: decided on the cast, as Caffe's static_cast has it: -1.5 is ignored under -1);
                      otherwise a label that is non-integral, outside [0, C), NaN or outside int's range is INVALID (CHOICE;
                      Caffe only DCHECKs): it is never used as an index; the statements raise, the device counts the position as ignored
                      and sets bit 0 of the status (the wrapper raises).  term = -log(max(p_li, FLT_MIN)) at valid positions, 0
                      elsewhere; count = the valid positions; the normaliser is max(count, 1) when normalize (CHOICE: the guard
                      of later BVLC get_normalizer; the 2015 fork divides by a zero count), else outer; loss = sum of the terms /
                      normaliser; scale = float32(loss_weight) / float32(normaliser); dscore_c = (p_c - [c == li]) * scale at
                      valid positions and +0.0 in all C channels elsewhere.  (Caffe's gradient ignores the FLT_MIN clamp; so
                      does this one.)  1 <= C <= 4096, outer * inner < 2^31.
    SmoothL1Loss      s2 = sigma * sigma in float32, thr = 1 / s2, d = (pred - target) * w_in,
                      term = (|d| < thr ? 0.5 * s2 * d * d : |d| - 0.5 / s2) * w_out, left to right, the comparison strict (|d| == thr
                      is linear); loss = sum of the terms / N; dpred = ((|d| < thr ? s2 * d : (0 < d) - (d < 0)) * w_in * w_out) *
                      (float32(loss_weight) / float32(N)).  The gradient with respect to target is the negation.
    SigmoidCrossEntropyLoss   pos = [x >= 0]; term = -(x * (t - pos) - log(1 + exp(x - 2 * x * pos))) * w; loss = sum / N;
                      dx = ((1 / (1 + exp(-x))) - t) * w * (float32(loss_weight) / float32(N)).  CHOICE: w multiplies every term
                      and every gradient element and the normaliser stays N (the reference fills mask_weight with ones for the
                      foreground rows and zeros for the rest, lib/pylayer/proposal_target_layer.py:209-211: either reading of the
                      weight gives the same numbers on its data).  exp(-x) may overflow to inf: dx = -t * w * scale is the rule.
    ReLU backward     dx = y > 0 ? dy : +0.0.        Sigmoid backward   dx = (dy * y) * (1 - y).  Both bit for bit."""
import numpy as np

from . import _lib
from .backward import Session

FLT_MIN = np.float32(np.finfo(np.float32).tiny)
OPS = {"relu": 1, "sigmoid": 2, 1: 1, 2: 2}


class LossResult(object):
    """loss, terms, grad, count, normalizer, prob (softmax only); abs_sum and n_terms in the float64 forms."""

    def __init__(self, loss, terms, grad, count, normalizer, prob=None, abs_sum=None, n_terms=None):
        self.loss, self.terms, self.grad, self.count, self.normalizer, self.prob = loss, terms, grad, count, normalizer, prob
        self.abs_sum, self.n_terms = abs_sum, n_terms


# ---- arguments ----

def _softmax_args(score, label):
    score = np.asarray(score, np.float32)
    label = np.asarray(label, np.float32)
    if score.ndim < 2:
        raise ValueError("softmax_loss: score %s has no class axis" % (score.shape,))
    outer, C = score.shape[:2]
    inner = int(np.prod(score.shape[2:], dtype=np.int64))
    if label.size != outer * inner:
        raise ValueError("softmax_loss: score %s and label %s do not fit" % (score.shape, label.shape))
    if not 1 <= C <= 4096 or outer * inner >= 2 ** 31:
        raise ValueError("softmax_loss: C = %d is not in [1, 4096], or 2^31 positions or more" % C)
    return np.ascontiguousarray(score.reshape(outer, C, inner)), np.ascontiguousarray(label.reshape(outer, inner)), score.shape


def classify_labels(label, C, ignore_label=None):
    """label float32 -> (valid bool, ignored bool, invalid bool, index int64 with 0 where not valid): the rule of the module text."""
    label = np.asarray(label, np.float32)
    castable = (label >= np.float32(-2.0 ** 31)) & (label < np.float32(2.0 ** 31))
    li = np.trunc(np.where(castable, label, np.float32(0))).astype(np.int64)           # C's (int): towards zero
    ignored = castable & (li == int(ignore_label)) if ignore_label is not None else np.zeros(label.shape, bool)
    valid = castable & ~ignored & (li.astype(np.float32) == label) & (li >= 0) & (li < C)
    return valid, ignored, ~valid & ~ignored, np.where(valid, li, 0)


def _labels(label, C, ignore_label):
    valid, _, invalid, idx = classify_labels(label, C, ignore_label)
    if invalid.any():
        raise ValueError("softmax_loss: label %r at position %d is neither ignore_label nor a class in [0, %d)"
                         % (float(label.ravel()[np.flatnonzero(invalid)[0]]), int(np.flatnonzero(invalid)[0]), C))
    return valid, idx


def _same_count(name, first, *others):
    first = np.asarray(first, np.float32)
    out = [first]
    for o in others:
        o = np.asarray(o, np.float32)
        if o.size != first.size:
            raise ValueError("%s: %s and %s do not fit" % (name, first.shape, o.shape))
        out.append(o.reshape(first.shape))
    if first.ndim < 1 or first.size >= 2 ** 31:
        raise ValueError("%s: a scalar bottom, or 2^31 elements or more" % name)
    return out


def _smooth_args(pred, target, w_in, w_out):
    pred = np.asarray(pred, np.float32)
    for o in (target, w_in, w_out):
        if np.shape(o) != pred.shape:
            raise ValueError("smooth_l1_loss: the four bottoms %s, %s, %s, %s are not of one shape"
                             % (pred.shape, np.shape(target), np.shape(w_in), np.shape(w_out)))
    return _same_count("smooth_l1_loss", pred, target, w_in, w_out)


# ---- the statements ----

def softmax_loss_numpy(score, label, ignore_label=None, normalize=True, loss_weight=1.0):
    """The float32 statement -- the specification csrc/loss.hip is tested against."""
    x, lab, shape = _softmax_args(score, label)
    outer, C, inner = x.shape
    valid, idx = _labels(lab, C, ignore_label)
    if x.size == 0:
        z = np.zeros(shape, np.float32)
        return LossResult(np.float32(0), np.zeros((outer, inner), np.float32), z, 0, np.float32(1 if normalize else outer), z.copy())
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = np.zeros((outer, inner), np.float32)
    for c in range(C):
        s = s + e[:, c, :]
    p = e / s[:, None, :]
    p_label = np.take_along_axis(p, idx[:, None, :], 1)[:, 0, :]
    terms = np.where(valid, -np.log(np.maximum(p_label, FLT_MIN)), np.float32(0)).astype(np.float32)
    count = int(valid.sum())
    normalizer = np.float32(max(count, 1) if normalize else outer)
    loss = terms.sum(dtype=np.float32) / normalizer
    scale = np.float32(loss_weight) / normalizer
    onehot = (np.arange(C)[None, :, None] == idx[:, None, :]).astype(np.float32)
    grad = np.where(valid[:, None, :], (p - onehot) * scale, np.float32(0)).astype(np.float32)
    return LossResult(loss, terms, grad.reshape(shape), count, normalizer, p.reshape(shape))


def softmax_loss_f64(score, label, ignore_label=None, normalize=True, loss_weight=1.0):
    """The float64 form on the same float32 inputs (the FLT_MIN clamp included); abs_sum and n_terms over the valid positions."""
    x, lab, shape = _softmax_args(score, label)
    outer, C, inner = x.shape
    valid, idx = _labels(lab, C, ignore_label)
    x = x.astype(np.float64)
    if x.size == 0:
        z = np.zeros(shape)
        return LossResult(0.0, np.zeros((outer, inner)), z, 0, float(1 if normalize else outer), z.copy(), 0.0, 0)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    p_label = np.take_along_axis(p, idx[:, None, :], 1)[:, 0, :]
    terms = np.where(valid, -np.log(np.maximum(p_label, float(FLT_MIN))), 0.0)
    count = int(valid.sum())
    normalizer = float(max(count, 1) if normalize else outer)
    onehot = (np.arange(C)[None, :, None] == idx[:, None, :]).astype(np.float64)
    grad = np.where(valid[:, None, :], (p - onehot) * (float(np.float32(loss_weight)) / normalizer), 0.0)
    return LossResult(terms.sum() / normalizer, terms, grad.reshape(shape), count, normalizer, p.reshape(shape),
                      float(np.abs(terms).sum()), count)


def smooth_l1_loss_numpy(pred, target, w_in, w_out, sigma=1.0, loss_weight=1.0):
    """The float32 statement."""
    pred, target, w_in, w_out = _smooth_args(pred, target, w_in, w_out)
    N = pred.shape[0]
    if pred.size == 0:
        return LossResult(np.float32(0), np.zeros(pred.shape, np.float32), np.zeros(pred.shape, np.float32), 0, np.float32(N))
    s2 = np.float32(sigma) * np.float32(sigma)
    thr = np.float32(1) / s2
    d = (pred - target) * w_in
    a = np.abs(d)
    quad = a < thr
    terms = np.where(quad, np.float32(0.5) * s2 * d * d, a - np.float32(0.5) / s2) * w_out
    sign = (np.float32(0) < d).astype(np.float32) - (d < np.float32(0)).astype(np.float32)
    grad = np.where(quad, s2 * d, sign) * w_in * w_out * (np.float32(loss_weight) / np.float32(N))
    return LossResult(terms.sum(dtype=np.float32) / np.float32(N), terms, grad, pred.size, np.float32(N))


def smooth_l1_loss_f64(pred, target, w_in, w_out, sigma=1.0, loss_weight=1.0):
    """The float64 form on the same float32 inputs and the float32 sigma."""
    pred, target, w_in, w_out = (a.astype(np.float64) for a in _smooth_args(pred, target, w_in, w_out))
    N = pred.shape[0]
    if pred.size == 0:
        return LossResult(0.0, np.zeros(pred.shape), np.zeros(pred.shape), 0, float(N), None, 0.0, 0)
    s2 = float(np.float32(sigma)) ** 2
    d = (pred - target) * w_in
    a = np.abs(d)
    quad = a < 1.0 / s2
    terms = np.where(quad, 0.5 * s2 * d * d, a - 0.5 / s2) * w_out
    grad = np.where(quad, s2 * d, np.sign(d)) * w_in * w_out * (float(np.float32(loss_weight)) / N)
    return LossResult(terms.sum() / N, terms, grad, pred.size, float(N), None, float(np.abs(terms).sum()), pred.size)


def _sigmoid_args(x, t, w):
    if w is None:
        x, t = _same_count("sigmoid_ce_loss", x, t)
        return x, t, None
    return _same_count("sigmoid_ce_loss", x, t, w)


def sigmoid_ce_loss_numpy(x, t, w=None, loss_weight=1.0):
    """The float32 statement; w None = no weight bottom."""
    x, t, w = _sigmoid_args(x, t, w)
    N = x.shape[0]
    if x.size == 0:
        return LossResult(np.float32(0), np.zeros(x.shape, np.float32), np.zeros(x.shape, np.float32), 0, np.float32(N))
    one = np.float32(1)
    wv = np.ones(x.shape, np.float32) if w is None else w
    pos = (x >= 0).astype(np.float32)
    with np.errstate(over="ignore"):
        terms = -(x * (t - pos) - np.log(one + np.exp(x - np.float32(2) * x * pos))) * wv
        grad = ((one / (one + np.exp(-x))) - t) * wv * (np.float32(loss_weight) / np.float32(N))
    return LossResult(terms.sum(dtype=np.float32) / np.float32(N), terms, grad, x.size, np.float32(N))


def sigmoid_ce_loss_f64(x, t, w=None, loss_weight=1.0):
    """The float64 form on the same float32 inputs (log1p for the logarithm: the form's own accuracy is not the subject)."""
    x, t, w = _sigmoid_args(x, t, w)
    x, t = x.astype(np.float64), t.astype(np.float64)
    N = x.shape[0]
    if x.size == 0:
        return LossResult(0.0, np.zeros(x.shape), np.zeros(x.shape), 0, float(N), None, 0.0, 0)
    wv = np.ones(x.shape) if w is None else w.astype(np.float64)
    pos = (x >= 0).astype(np.float64)
    terms = -(x * (t - pos) - np.log1p(np.exp(x - 2 * x * pos))) * wv
    with np.errstate(over="ignore"):
        grad = (1.0 / (1.0 + np.exp(-x)) - t) * wv * (float(np.float32(loss_weight)) / N)
    return LossResult(terms.sum() / N, terms, grad, x.size, float(N), None, float(np.abs(terms).sum()), x.size)


def _eltwise_args(y, dy, op):
    if op not in OPS:
        raise ValueError("eltwise_backward: op is 'relu' (1) or 'sigmoid' (2)")
    y, dy = np.asarray(y, np.float32), np.asarray(dy, np.float32)
    if y.shape != dy.shape:
        raise ValueError("eltwise_backward: y %s and dy %s do not fit" % (y.shape, dy.shape))
    return y, dy, OPS[op]


def eltwise_backward_numpy(y, dy, op):
    """y = the layer's output, dy = the gradient of its top -> the gradient of its bottom, float32."""
    y, dy, op = _eltwise_args(y, dy, op)
    if op == 1:
        return np.where(y > 0, dy, np.float32(0))
    return (dy * y) * (np.float32(1) - y)


# ---- the device ----

def softmax_plan(plan):
    """mnc_softmax_loss_plan: 0 = the layout by shape (the default), 1 = one lane per position, 2 = one wave per position."""
    try:
        _lib.call("mnc_softmax_loss_plan", int(plan))
    except _lib.MncError as e:
        raise ValueError(str(e))


def _result(s, d_result, who):
    raw = s.get(d_result, (4,))
    count, status = (int(v) for v in raw[2:].view(np.int32))
    if status:
        raise ValueError("%s: status %d: a label is neither ignore_label nor a class" % (who, status))
    return raw[0], raw[1], count


def softmax_loss(score, label, ignore_label=None, normalize=True, loss_weight=1.0, device_id=None):
    """softmax_loss_numpy on the GPU (mnc_softmax_loss): prob and grad the same bytes, terms within logf's ulps."""
    x, lab, shape = _softmax_args(score, label)
    outer, C, inner = x.shape
    with Session(device_id) as s:
        d_x, d_lab = s.put(x), s.put(lab)
        d_prob, d_terms, d_grad, d_res = s.empty(x.nbytes), s.empty(lab.nbytes), s.empty(x.nbytes), s.empty(16)
        s.call("mnc_softmax_loss", d_x, d_lab, outer, C, inner, int(ignore_label is not None), int(ignore_label or 0), int(bool(normalize)),
               float(loss_weight), d_prob, d_terms, d_grad, d_res)
        loss, normalizer, count = _result(s, d_res, "softmax_loss")
        prob, terms, grad = s.get(d_prob, shape), s.get(d_terms, (outer, inner)), s.get(d_grad, shape)
    return LossResult(loss, terms, grad, count, normalizer, prob)


def smooth_l1_loss(pred, target, w_in, w_out, sigma=1.0, loss_weight=1.0, device_id=None):
    """smooth_l1_loss_numpy on the GPU (mnc_smooth_l1_loss): terms and grad the same bytes."""
    pred, target, w_in, w_out = _smooth_args(pred, target, w_in, w_out)
    with Session(device_id) as s:
        d_in = [s.put(a) for a in (pred, target, w_in, w_out)]
        d_terms, d_grad, d_res = s.empty(pred.nbytes), s.empty(pred.nbytes), s.empty(16)
        s.call("mnc_smooth_l1_loss", d_in[0], d_in[1], d_in[2], d_in[3], pred.shape[0], pred.size, float(sigma), float(loss_weight),
               d_terms, d_grad, d_res)
        loss, normalizer, count = _result(s, d_res, "smooth_l1_loss")
        terms, grad = s.get(d_terms, pred.shape), s.get(d_grad, pred.shape)
    return LossResult(loss, terms, grad, count, normalizer)


def sigmoid_ce_loss(x, t, w=None, loss_weight=1.0, device_id=None):
    """sigmoid_ce_loss_numpy on the GPU (mnc_sigmoid_ce_loss): grad the same bytes, terms within logf's ulps."""
    x, t, w = _sigmoid_args(x, t, w)
    with Session(device_id) as s:
        d_x, d_t = s.put(x), s.put(t)
        d_w = s.put(w) if w is not None else None
        d_terms, d_grad, d_res = s.empty(x.nbytes), s.empty(x.nbytes), s.empty(16)
        s.call("mnc_sigmoid_ce_loss", d_x, d_t, d_w, x.shape[0], x.size, float(loss_weight), d_terms, d_grad, d_res)
        loss, normalizer, count = _result(s, d_res, "sigmoid_ce_loss")
        terms, grad = s.get(d_terms, x.shape), s.get(d_grad, x.shape)
    return LossResult(loss, terms, grad, count, normalizer)


def eltwise_backward(y, dy, op, device_id=None):
    """eltwise_backward_numpy on the GPU (mnc_eltwise_backward): the same bytes."""
    y, dy, op = _eltwise_args(y, dy, op)
    with Session(device_id) as s:
        d_y, d_dy = s.put(y), s.put(dy)
        d_dx = s.empty(y.nbytes)
        s.call("mnc_eltwise_backward", d_y, d_dy, d_dx, y.size, op)
        dx = s.get(d_dx, y.shape)
    return dx
