"""csrc/loss.hip on the GPU against the statements of mnc_amd/losses.py: every gradient, the probabilities, the SmoothL1 terms and
both activation backward passes bit for bit, in every forced layout; the terms behind a logarithm within the ulp allowance of
tests/loss_inputs.py; the scalar loss within the worst-case float32 bound of the float64 form; count, normaliser and status; the
same bytes on every run; null outputs untouched; invalid labels; zero sizes; the refusals; loss and activation backward composed."""
import functools

import numpy as np
import pytest

import loss_inputs as LI
from gpu_util import Dev
from mnc_amd import _lib
from mnc_amd import losses as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    _lib.call("mnc_softmax_loss_plan", 0)
    d.close()


def _unpack(raw):
    """The 16 bytes of d_result -> (loss float32, normaliser float32, count, status)."""
    i = raw.view(np.int32)
    return raw[0], raw[1], int(i[2]), int(i[3])


@functools.lru_cache(maxsize=None)
def log_allowance():
    """Ulps a term behind a logarithm may be off the float64 log of the statement's float32 argument: the larger of what numpy's
    own float32 log shows on the corpus and the published bound of the device's logf, plus the roundings after the logarithm."""
    shown = max(float(LI.ulp_error(LI.softmax_ref(k)[0].terms, LI.softmax_term_reference(k)).max()) for k in LI.SOFTMAX_KEYS)
    shown = max([shown] + [float(LI.ulp_error(LI.sigmoid_ref(k)[0].terms, LI.sigmoid_term_reference(k)).max()) for k in LI.SIGMOID_KEYS])
    print("numpy's float32 log on the corpus: %.3f ulp; logf: %.1f ulp" % (shown, LI.LOGF_ULP))
    return max(shown, LI.LOGF_ULP) + LI.FINAL_OP_ULP


# ---- SoftmaxWithLoss

def run_softmax(dev, c, want=("prob", "terms", "grad"), fill=np.nan):
    """mnc_softmax_loss on buffers pre-filled with `fill` -> dict of what comes back (outputs not wanted are passed as NULL)."""
    score, label = c["score"], c["label"]
    outer, C, inner = score.shape
    mark = dev.mark()
    d = {"prob": dev.empty(score.shape, fill=fill), "terms": dev.empty(label.shape, fill=fill), "grad": dev.empty(score.shape, fill=fill)}
    d_res = dev.empty((4,), fill=fill)
    dev.call("mnc_softmax_loss", dev.put(score), dev.put(label), outer, C, inner, c["has_ignore"], LI.IGNORE, int(c["normalize"]),
             float(c["loss_weight"]), *[d[k] if k in want else None for k in ("prob", "terms", "grad")], d_res)
    out = {"prob": dev.get(d["prob"], score.shape), "terms": dev.get(d["terms"], label.shape), "grad": dev.get(d["grad"], score.shape),
           "res": dev.get(d_res, (4,))}
    dev.free_since(mark)
    return out


@pytest.mark.parametrize("plan", (0, 1, 2))
@pytest.mark.parametrize("key", LI.SOFTMAX_KEYS)
def test_softmax_loss_against_the_statements(dev, key, plan):
    c, (r32, r64) = LI.softmax_case(key), LI.softmax_ref(key)
    outer, C, inner = c["score"].shape
    _lib.call("mnc_softmax_loss_plan", plan)
    try:
        got = run_softmax(dev, c)
        again = run_softmax(dev, c, fill=3.0)
    finally:
        _lib.call("mnc_softmax_loss_plan", 0)
    loss, normalizer, count, status = _unpack(got["res"])
    assert status == c["status"] and count == r32.count and normalizer == r32.normalizer
    assert not np.isnan(got["prob"]).any() and not np.isnan(got["grad"]).any() and not np.isnan(got["terms"]).any()
    assert np.array_equal(got["prob"], r32.prob.reshape(outer, C, inner))
    assert got["grad"].tobytes() == r32.grad.reshape(outer, C, inner).tobytes()        # invalid labels: the statement's with ignore_label in their place
    off = ~L.classify_labels(c["label"], C, LI.IGNORE if c["has_ignore"] else None)[0]
    assert (np.moveaxis(got["grad"], 1, 2)[off].view(np.uint32) == 0).all()           # +0.0 in all C channels of an ignored or invalid position
    assert (got["terms"][off] == 0).all()
    ulps = LI.ulp_error(got["terms"], LI.softmax_term_reference(key))
    print("terms: %.3f ulp of %.1f allowed" % (ulps.max(), log_allowance()))
    assert ulps.max() <= log_allowance()
    err, lim = abs(float(loss) - r64.loss), LI.loss_bound(r64, log_allowance())
    print("loss %.9g, float64 %.17g: error %.3g, bound %.3g" % (loss, r64.loss, err, lim))
    assert err <= lim
    for k in ("prob", "terms", "grad", "res"):
        assert again[k].tobytes() == got[k].tobytes(), k


def test_softmax_loss_null_outputs_stay_untouched(dev):
    c = LI.softmax_case("7x21x1-normal-mixed")
    for plan in (1, 2):
        _lib.call("mnc_softmax_loss_plan", plan)
        try:
            full = run_softmax(dev, c)                 # (per layout: the loss is summed in the layout's order)
            for want in ((), ("prob",), ("terms",), ("grad",), ("prob", "grad")):
                got = run_softmax(dev, c, want=want)
                assert got["res"].tobytes() == full["res"].tobytes()
                for k in ("prob", "terms", "grad"):
                    assert got[k].tobytes() == full[k].tobytes() if k in want else np.isnan(got[k]).all(), (plan, want, k)
        finally:
            _lib.call("mnc_softmax_loss_plan", 0)


# ---- SmoothL1Loss

def run_smooth(dev, c, want=("terms", "grad"), fill=np.nan):
    pred = c["pred"]
    mark = dev.mark()
    d_terms, d_grad, d_res = dev.empty(pred.shape, fill=fill), dev.empty(pred.shape, fill=fill), dev.empty((4,), fill=fill)
    dev.call("mnc_smooth_l1_loss", dev.put(pred), dev.put(c["target"]), dev.put(c["w_in"]), dev.put(c["w_out"]), pred.shape[0], pred.size,
             float(c["sigma"]), float(c["loss_weight"]), d_terms if "terms" in want else None, d_grad if "grad" in want else None, d_res)
    out = {"terms": dev.get(d_terms, pred.shape), "grad": dev.get(d_grad, pred.shape), "res": dev.get(d_res, (4,))}
    dev.free_since(mark)
    return out


@pytest.mark.parametrize("key", LI.SMOOTH_KEYS)
def test_smooth_l1_loss_against_the_statements(dev, key):
    c, (r32, r64) = LI.smooth_case(key), LI.smooth_ref(key)
    got = run_smooth(dev, c)
    loss, normalizer, count, status = _unpack(got["res"])
    assert status == 0 and count == c["pred"].size and normalizer == c["pred"].shape[0]
    assert got["terms"].tobytes() == r32.terms.tobytes() and got["grad"].tobytes() == r32.grad.tobytes()
    err, lim = abs(float(loss) - r64.loss), LI.loss_bound(r64)
    print("loss %.9g, float64 %.17g: error %.3g, bound %.3g" % (loss, r64.loss, err, lim))
    assert err <= lim
    if key == "dyadic":
        assert float(loss) == r64.loss                                                 # nothing rounds, in any order
    again = run_smooth(dev, c, fill=3.0)
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    for want in ((), ("terms",), ("grad",)):
        part = run_smooth(dev, c, want=want)
        assert part["res"].tobytes() == got["res"].tobytes()
        for k in ("terms", "grad"):
            assert part[k].tobytes() == got[k].tobytes() if k in want else np.isnan(part[k]).all(), (want, k)


# ---- SigmoidCrossEntropyLoss

def run_sigmoid(dev, c, want=("terms", "grad"), fill=np.nan):
    x = c["x"]
    mark = dev.mark()
    d_terms, d_grad, d_res = dev.empty(x.shape, fill=fill), dev.empty(x.shape, fill=fill), dev.empty((4,), fill=fill)
    dev.call("mnc_sigmoid_ce_loss", dev.put(x), dev.put(c["t"]), dev.put(c["w"]) if c["w"] is not None else None, x.shape[0], x.size,
             float(c["loss_weight"]), d_terms if "terms" in want else None, d_grad if "grad" in want else None, d_res)
    out = {"terms": dev.get(d_terms, x.shape), "grad": dev.get(d_grad, x.shape), "res": dev.get(d_res, (4,))}
    dev.free_since(mark)
    return out


@pytest.mark.parametrize("key", LI.SIGMOID_KEYS)
def test_sigmoid_ce_loss_against_the_statements(dev, key):
    c, (r32, r64) = LI.sigmoid_case(key), LI.sigmoid_ref(key)
    got = run_sigmoid(dev, c)
    loss, normalizer, count, status = _unpack(got["res"])
    assert status == 0 and count == c["x"].size and normalizer == c["x"].shape[0]
    assert got["grad"].tobytes() == r32.grad.tobytes()
    assert not np.isnan(got["terms"]).any()
    ulps = LI.ulp_error(got["terms"], LI.sigmoid_term_reference(key))
    print("terms: %.3f ulp of %.1f allowed" % (ulps.max(), log_allowance()))
    assert ulps.max() <= log_allowance()
    err, lim = abs(float(loss) - r64.loss), LI.loss_bound(r64, log_allowance())
    print("loss %.9g, float64 %.17g: error %.3g, bound %.3g" % (loss, r64.loss, err, lim))
    assert err <= lim
    again = run_sigmoid(dev, c, fill=3.0)
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    for want in ((), ("terms",), ("grad",)):
        part = run_sigmoid(dev, c, want=want)
        assert part["res"].tobytes() == got["res"].tobytes()
        for k in ("terms", "grad"):
            assert part[k].tobytes() == got[k].tobytes() if k in want else np.isnan(part[k]).all(), (want, k)


# ---- ReLU / Sigmoid backward

@pytest.mark.parametrize("op", (1, 2))
@pytest.mark.parametrize("count", LI.ELTWISE_COUNTS)
def test_eltwise_backward(dev, count, op):
    y, dy = LI.eltwise_case(count)
    mark = dev.mark()
    d_dx = dev.empty((count + 3,), fill=np.nan)
    dev.call("mnc_eltwise_backward", dev.put(y), dev.put(dy), d_dx, count, op)
    dx = dev.get(d_dx, (count + 3,))
    dev.free_since(mark)
    assert dx[:count].tobytes() == L.eltwise_backward_numpy(y, dy, op).tobytes() and np.isnan(dx[count:]).all()


def test_sigmoid_loss_composes_with_the_sigmoid_backward(dev):
    """The loss layer on the logits x against the same loss stated on y = sigmoid(x) and carried back through
    mnc_eltwise_backward(op = 2): L = -sum w (t log y + (1 - t) log(1 - y)) / N, dL/dy = -w (t / y - (1 - t) / (1 - y)) / N in
    float64 from the float64 y; dy and y go to the device as float32.  Per element both routes are (y - t) * w / N with a handful
    of roundings each: two addends, so |difference| <= (2 + 32) * 2^-24 * (y + t) * w / N, the n24 form -- plus what this route,
    unlike the loss layer's own, owes to handing y over in float32: dy * y * (1 - y) moves by |dy| * |1 - 2 y| per unit of y, and
    the float32 y is up to half a spacing off (with t = 0 and y near 1, dy = w / (N (1 - y)) is large and 1 - y cancels).
    |x| <= 6 keeps that term small."""
    rng = np.random.default_rng(441)
    x = np.clip(rng.standard_normal((6, 441)) * 2.0, -6.0, 6.0).astype(np.float32)
    t = (rng.random((6, 1, 21, 21)) < 0.4).astype(np.float32)
    w = np.repeat(np.array([1, 1, 1, 1, 0, 0], np.float32), 441).reshape(6, 1, 21, 21)
    got = run_sigmoid(dev, {"x": x, "t": t, "w": w, "loss_weight": 1.0})
    x64, t64, w64 = x.astype(np.float64), t.reshape(6, 441).astype(np.float64), w.reshape(6, 441).astype(np.float64)
    y64 = 1.0 / (1.0 + np.exp(-x64))
    terms64 = -w64 * (t64 * np.log(y64) + (1 - t64) * np.log1p(-y64))
    loss64 = terms64.sum() / 6
    f64 = L.LossResult(loss64, terms64, None, x.size, 6.0, None, float(np.abs(terms64).sum()), x.size)
    assert abs(float(got["res"][0]) - loss64) <= LI.loss_bound(f64, log_allowance())
    dy = -w64 * (t64 / y64 - (1 - t64) / (1 - y64)) / 6
    mark = dev.mark()
    d_dx = dev.empty(x.shape, fill=np.nan)
    dev.call("mnc_eltwise_backward", dev.put(y64.astype(np.float32)), dev.put(dy.astype(np.float32)), d_dx, x.size, 2)
    dx = dev.get(d_dx, x.shape)
    dev.free_since(mark)
    half_spacing = np.spacing(y64.astype(np.float32)).astype(np.float64) / 2
    lim = 34 * 2.0 ** -24 * (y64 + t64) * w64 / 6 + np.abs(dy) * np.abs(1 - 2 * y64) * half_spacing
    assert (np.abs(dx.astype(np.float64) - got["grad"].astype(np.float64)) <= lim).all()
    assert (dx[4:] == 0).all() and dx[:4].any()


# ---- zero sizes, refusals, the host-array functions

def test_zero_size_calls_return_a_zero_loss(dev):
    mark = dev.mark()
    d_a = dev.empty((64,), fill=7.0)
    for name, args in (("mnc_softmax_loss", [d_a, d_a, 0, 21, 1, 1, -1, 1, 1.0, d_a, d_a, d_a]),
                       ("mnc_softmax_loss", [d_a, d_a, 4, 2, 0, 1, -1, 1, 1.0, d_a, d_a, d_a]),
                       ("mnc_softmax_loss", [None, None, 0, 21, 1, 0, 0, 0, 1.0, None, None, None]),
                       ("mnc_smooth_l1_loss", [d_a, d_a, d_a, d_a, 0, 0, 3.0, 1.0, d_a, d_a]),
                       ("mnc_smooth_l1_loss", [d_a, d_a, d_a, d_a, 4, 0, 3.0, 1.0, d_a, d_a]),
                       ("mnc_sigmoid_ce_loss", [d_a, d_a, None, 0, 0, 1.0, d_a, d_a]),
                       ("mnc_sigmoid_ce_loss", [None, None, None, 0, 16, 1.0, None, None])):
        d_res = dev.empty((4,), fill=np.nan)
        dev.call(name, *(args + [d_res]))
        assert dev.get(d_res, (4,)).tobytes() == bytes(16), name
    dev.call("mnc_eltwise_backward", None, None, None, 0, 1)
    assert (dev.get(d_a, (64,)) == 7.0).all()
    dev.free_since(mark)


def _refused(dev, name, *args):
    with pytest.raises(_lib.MncError) as e:
        dev.call(name, *args)
    assert e.value.code == 1, (name, e.value)


def test_refusals_leave_the_outputs_alone(dev):
    """Limits and null pointers: MNC_ERR_INVALID (1) before any launch."""
    mark = dev.mark()
    d_in, d_a, d_res = dev.empty((64,), fill=0.0), dev.empty((64,), fill=7.0), dev.empty((4,), fill=7.0)
    soft = lambda **k: [k.get("score", d_in), k.get("label", d_in), k.get("outer", 2), k.get("C", 3), k.get("inner", 4), 1, -1, 1, 1.0, d_a, d_a,
                        d_a, k.get("res", d_res)]
    for a in (soft(C=0), soft(C=4097), soft(outer=-1), soft(inner=-1), soft(outer=65536, inner=32768), soft(score=None), soft(label=None),
              soft(res=None)):
        _refused(dev, "mnc_softmax_loss", *a)
    sm = lambda **k: [k.get("pred", d_in), d_in, k.get("w_in", d_in), d_in, k.get("N", 2), k.get("count", 16), 3.0, 1.0, d_a, d_a, k.get("res", d_res)]
    for a in (sm(N=-1), sm(count=-1), sm(count=2 ** 31), sm(pred=None), sm(w_in=None), sm(res=None)):
        _refused(dev, "mnc_smooth_l1_loss", *a)
    sg = lambda **k: [k.get("x", d_in), k.get("t", d_in), None, k.get("N", 2), k.get("count", 16), 1.0, d_a, d_a, k.get("res", d_res)]
    for a in (sg(N=-1), sg(count=-1), sg(count=2 ** 31), sg(x=None), sg(t=None), sg(res=None)):
        _refused(dev, "mnc_sigmoid_ce_loss", *a)
    for a in ([d_in, d_in, d_a, 16, 0], [d_in, d_in, d_a, 16, 3], [None, d_in, d_a, 16, 1], [d_in, None, d_a, 16, 1], [d_in, d_in, None, 16, 2]):
        _refused(dev, "mnc_eltwise_backward", *a)
    with pytest.raises(_lib.MncError) as e:
        _lib.call("mnc_softmax_loss_plan", 3)
    assert e.value.code == 1
    assert (dev.get(d_a, (64,)) == 7.0).all() and (dev.get(d_res, (4,)) == 7.0).all()
    dev.free_since(mark)


def test_host_array_functions(dev):
    """mnc_amd.losses' device functions: Caffe's shapes in, the statements' results out, ValueError for a status bit and for what the
    library refuses."""
    c, (r32, r64) = LI.softmax_case("1x2x135-normal-mixed"), LI.softmax_ref("1x2x135-normal-mixed")
    got = L.softmax_loss(c["score"].reshape(1, 2, 27, 5), c["label"].reshape(1, 1, 27, 5), LI.IGNORE, device_id=0)
    assert got.grad.shape == (1, 2, 27, 5) and got.grad.tobytes() == r32.grad.tobytes() and got.prob.tobytes() == r32.prob.tobytes()
    assert got.count == r32.count and got.normalizer == r32.normalizer and abs(float(got.loss) - r64.loss) <= LI.loss_bound(r64, log_allowance())
    c, (r32, _) = LI.softmax_case("7x21x1-normal-none_ignored"), LI.softmax_ref("7x21x1-normal-none_ignored")
    for label in (c["label"].reshape(7), c["label"].reshape(7, 1)):
        got = L.softmax_loss(c["score"].reshape(7, 21), label, None, c["normalize"], c["loss_weight"], device_id=0)
        assert got.grad.tobytes() == r32.grad.tobytes() and got.normalizer == 7
    with pytest.raises(ValueError):                                                   # a status bit
        L.softmax_loss(c["score"].reshape(7, 21), np.full(7, 21.0, np.float32), LI.IGNORE, device_id=0)
    with pytest.raises(ValueError):                                                   # the statement's own shape check
        L.softmax_loss(np.zeros((2, 4097), np.float32), np.zeros(2, np.float32), device_id=0)
    c, (r32, _) = LI.smooth_case("rpn"), LI.smooth_ref("rpn")
    got = L.smooth_l1_loss(*LI.smooth_args(c), device_id=0)
    assert got.terms.tobytes() == r32.terms.tobytes() and got.grad.tobytes() == r32.grad.tobytes() and got.count == c["pred"].size
    c, (r32, r64) = LI.sigmoid_case("mask"), LI.sigmoid_ref("mask")
    got = L.sigmoid_ce_loss(*LI.sigmoid_args(c), device_id=0)
    assert got.grad.tobytes() == r32.grad.tobytes() and abs(float(got.loss) - r64.loss) <= LI.loss_bound(r64, log_allowance())
    y, dy = LI.eltwise_case(65)
    for op in ("relu", "sigmoid"):
        assert L.eltwise_backward(y, dy, op, device_id=0).tobytes() == L.eltwise_backward_numpy(y, dy, op).tobytes()
    e = L.softmax_loss(np.zeros((0, 21), np.float32), np.zeros(0, np.float32), LI.IGNORE, device_id=0)
    assert float(e.loss) == 0 and e.count == 0
    with pytest.raises(ValueError):
        L.softmax_plan(5)
