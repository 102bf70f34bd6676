"""CPU: the statements of mnc_amd/losses.py.  The float64 forms are torch's (loss and autograd) and the derivatives of their own
losses (central differences); the float32 statements stay within the rounding bound of the float64 forms; the exact cases are
exact; the threshold elements take the branch the rule names; what does not fit raises."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_inputs as LI
from mnc_amd import losses as L

CLAMP = -np.log(float(L.FLT_MIN))          # the largest term the FLT_MIN clamp lets through


@pytest.fixture(autouse=True)
def _autograd_on():
    """Other modules of the suite switch autograd off for the process; these tests need it."""
    with torch.enable_grad():
        yield


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize("key", LI.SOFTMAX_KEYS)
def test_softmax_f64_is_torch_cross_entropy(key):
    """F.cross_entropy(ignore_index, reduction='mean'); an all-ignored case: 'sum' over 1.  The form's one departure from torch is
    Caffe's FLT_MIN clamp of the VALUE (the +-80 rows): there the per-position terms are torch's clamped at -log(FLT_MIN); the
    gradient ignores the clamp in Caffe as in torch."""
    c, (_, r64) = LI.softmax_case(key), LI.softmax_ref(key)
    outer, C, inner = c["score"].shape
    x = _t(c["score"], True)
    target = torch.tensor(c["ref_label"].astype(np.int64))
    per = F.cross_entropy(x, target, ignore_index=LI.IGNORE, reduction="none")
    assert np.abs(np.minimum(per.detach().numpy(), CLAMP) - r64.terms).max(initial=0) <= 1e-12
    if r64.count == 0:
        loss = F.cross_entropy(x, target, ignore_index=LI.IGNORE, reduction="sum") / 1.0
    elif c["normalize"]:
        loss = F.cross_entropy(x, target, ignore_index=LI.IGNORE, reduction="mean")
    else:
        loss = F.cross_entropy(x, target, ignore_index=LI.IGNORE, reduction="sum") / outer
    (loss * float(np.float32(c["loss_weight"]))).backward()
    assert np.abs(x.grad.numpy() - r64.grad).max() <= 1e-12
    if not (r64.terms >= CLAMP * (1 - 1e-12)).any():
        assert abs(float(loss.detach()) - r64.loss) <= 1e-12
    assert r64.normalizer == (max(r64.count, 1) if c["normalize"] else outer) and r64.n_terms == r64.count


@pytest.mark.parametrize("key", LI.SMOOTH_KEYS)
def test_smooth_l1_f64_is_torch_smooth_l1(key):
    c, (_, r64) = LI.smooth_case(key), LI.smooth_ref(key)
    pred, target, w_in, w_out = _t(c["pred"], True), _t(c["target"]), _t(c["w_in"]), _t(c["w_out"])
    N = c["pred"].shape[0]
    per = F.smooth_l1_loss(pred * w_in, target * w_in, beta=1.0 / float(np.float32(c["sigma"])) ** 2, reduction="none") * w_out
    loss = per.sum() / N
    (loss * c["loss_weight"]).backward()
    assert abs(float(loss.detach()) - r64.loss) <= 1e-12
    assert np.abs(per.detach().numpy() - r64.terms).max() <= 1e-12
    assert np.abs(pred.grad.numpy() - r64.grad).max() <= 1e-12


@pytest.mark.parametrize("key", LI.SIGMOID_KEYS)
def test_sigmoid_ce_f64_is_torch_bce_with_logits(key):
    c, (_, r64) = LI.sigmoid_case(key), LI.sigmoid_ref(key)
    x = _t(c["x"], True)
    t = _t(c["t"].reshape(c["x"].shape))
    w = _t(np.ones(c["x"].shape) if c["w"] is None else c["w"].reshape(c["x"].shape))
    per = F.binary_cross_entropy_with_logits(x, t, reduction="none") * w
    loss = per.sum() / c["x"].shape[0]
    (loss * c["loss_weight"]).backward()
    assert abs(float(loss.detach()) - r64.loss) <= 1e-12
    assert np.abs(per.detach().numpy() - r64.terms).max() <= 1e-12
    assert np.abs(x.grad.numpy() - r64.grad).max() <= 1e-12


def _central(f, x, h=1e-6):
    """Central differences of the scalar f at the float32 array x, in float64, element by element."""
    x = np.array(x, np.float64, order="C")                              # (a contiguous copy: flat below is a view of it)
    g = np.zeros(x.shape)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        up = f(x)
        flat[i] = keep - h
        gf[i] = (up - f(x)) / (2 * h)
        flat[i] = keep
    return g


def _fd_tol(f0, h=1e-6):
    """What central differences with step h may be off by: the rounding of the two float64 sums of size f0 (a few units of
    2^-53 * f0 each, over 2 h) plus the truncation h^2 / 6 times a third derivative, which is below 1 for these losses."""
    return 8 * 2.0 ** -53 * abs(f0) / h + h * h


def test_f64_gradients_are_central_differences():
    """Each float64 gradient against central differences of its float64 loss, at points away from the kinks (the SmoothL1
    threshold; the FLT_MIN clamp, which the gradient ignores by rule).  The forms cast their inputs to float32 first, so the
    differences are taken through a float64 restatement of each loss, which the form's loss has to equal at the point itself."""
    c = LI.softmax_case("7x21x1-normal-mixed")
    r64 = LI.softmax_ref("7x21x1-normal-mixed")[1]
    valid, _, _, idx = L.classify_labels(c["ref_label"], 21, LI.IGNORE)

    def softmax_loss64(x):
        z = x - x.max(axis=1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
        per = -np.take_along_axis(logp, idx[:, None, :], 1)[:, 0, :]
        return np.where(valid, per, 0.0).sum() / max(int(valid.sum()), 1)

    x0 = c["score"].astype(np.float64)
    assert abs(softmax_loss64(x0) - r64.loss) <= 1e-12
    assert np.abs(_central(softmax_loss64, x0) * c["loss_weight"] - r64.grad).max() <= _fd_tol(r64.abs_sum / r64.normalizer)

    c = LI.smooth_case("head")
    r64 = LI.smooth_ref("head")[1]
    tg, wi, wo = (c[k].astype(np.float64) for k in ("target", "w_in", "w_out"))
    s2 = float(np.float32(c["sigma"])) ** 2

    def smooth_loss64(p):
        d = (p - tg) * wi
        a = np.abs(d)
        return (np.where(a < 1.0 / s2, 0.5 * s2 * d * d, a - 0.5 / s2) * wo).sum() / p.shape[0]

    p0 = c["pred"].astype(np.float64)
    assert abs(smooth_loss64(p0) - r64.loss) <= 1e-12
    far = np.abs(np.abs((p0 - tg) * wi) - 1.0 / s2) > 1e-4               # (no element of the corpus sits within h of the kink)
    assert far.all()
    assert np.abs(_central(smooth_loss64, p0) * c["loss_weight"] - r64.grad).max() <= c["loss_weight"] * _fd_tol(r64.abs_sum / r64.normalizer)

    c = LI.sigmoid_case("tiny")
    r64 = LI.sigmoid_ref("tiny")[1]
    t, w = c["t"].astype(np.float64), c["w"].astype(np.float64)

    def sigmoid_loss64(x):
        pos = (x >= 0).astype(np.float64)
        return (-(x * (t - pos) - np.log1p(np.exp(x - 2 * x * pos))) * w).sum() / x.shape[0]

    x0 = c["x"].astype(np.float64)
    assert abs(sigmoid_loss64(x0) - r64.loss) <= 1e-12
    assert np.abs(_central(sigmoid_loss64, x0) * c["loss_weight"] - r64.grad).max() <= _fd_tol(r64.abs_sum / r64.normalizer)
    c = LI.sigmoid_case("mask")                                          # the large case: a sample of elements, specials included
    r64 = LI.sigmoid_ref("mask")[1]
    t, w = c["t"].reshape(6, 441).astype(np.float64)[:, :12], c["w"].reshape(6, 441).astype(np.float64)[:, :12]
    x0 = c["x"].astype(np.float64)[:, :12]
    keep = np.abs(x0) > 1e-3                                             # (x = +-0 sits on the kink of pos; the loss is smooth there, its formula is not)
    g = _central(sigmoid_loss64, x0)
    assert np.abs(g * c["loss_weight"] - r64.grad[:, :12])[keep].max() <= _fd_tol(sigmoid_loss64(x0))


@pytest.mark.parametrize("key", LI.SOFTMAX_KEYS)
def test_softmax_f32_statement_within_the_bound(key):
    r32, r64 = LI.softmax_ref(key)
    assert r32.loss.dtype == np.float32 and r32.grad.dtype == np.float32 and r32.prob.dtype == np.float32 and r32.terms.dtype == np.float32
    err, lim = abs(float(r32.loss) - r64.loss), LI.loss_bound(r64)
    print("float32 statement: error %.3g, bound %.3g (%.1f %%)" % (err, lim, 100 * err / lim if lim else 0.0))
    assert err <= lim
    assert r32.count == r64.count and float(r32.normalizer) == r64.normalizer
    C = r32.prob.shape[1]
    assert np.abs(r32.prob - r64.prob).max(initial=0) <= (C + 8) * 2.0 ** -24     # C roundings in s, a few in exp and the division; p <= 1
    assert np.abs(r32.grad - r64.grad).max(initial=0) <= (C + 9) * 2.0 ** -24 * float(np.float32(LI.softmax_case(key)["loss_weight"])) / r64.normalizer
    ignored = ~L.classify_labels(LI.softmax_case(key)["ref_label"], C, LI.IGNORE)[0]
    g = np.moveaxis(r32.grad.reshape(r32.grad.shape[0], C, -1), 1, 2)[ignored]
    assert (g.view(np.uint32) == 0).all()                               # +0.0 in all C channels: the bit pattern


def test_softmax_terms_numpy_log_error():
    """The error numpy's own float32 log shows against the float64 log of the same float32 argument, over the corpus: the figure
    the GPU test's allowance is the larger of, next to LOGF_ULP."""
    worst = max(float(LI.ulp_error(LI.softmax_ref(k)[0].terms, LI.softmax_term_reference(k)).max()) for k in LI.SOFTMAX_KEYS)
    print("numpy float32 log on the softmax corpus: %.3f ulp" % worst)
    assert worst <= 4.0                                                   # numpy documents its float32 log as within 4 ulp


@pytest.mark.parametrize("key", LI.SMOOTH_KEYS)
def test_smooth_l1_f32_statement_within_the_bound(key):
    r32, r64 = LI.smooth_ref(key)
    assert r32.terms.dtype == np.float32 and r32.grad.dtype == np.float32 and r32.loss.dtype == np.float32
    err, lim = abs(float(r32.loss) - r64.loss), LI.loss_bound(r64)
    print("float32 statement: error %.3g, bound %.3g (%.1f %%)" % (err, lim, 100 * err / lim if lim else 0.0))
    assert err <= lim
    assert np.abs(r32.terms - r64.terms).max() <= 8 * 2.0 ** -24 * np.abs(r64.terms).max()
    assert r32.count == r32.terms.size and float(r32.normalizer) == r32.terms.shape[0]


def test_smooth_l1_dyadic_case_is_exact():
    r32, r64 = LI.smooth_ref("dyadic")
    assert float(r32.loss) == r64.loss and r64.loss > 0
    assert np.array_equal(r32.terms.astype(np.float64), r64.terms) and np.array_equal(r32.grad.astype(np.float64), r64.grad)


def test_smooth_l1_threshold_elements_take_the_named_branch():
    c, (r32, _) = LI.smooth_case("edges"), LI.smooth_ref("edges")
    f = np.float32
    s2 = f(9)
    thr, lin = f(1) / s2, f(0.5) / s2
    d = c["pred"][0]
    assert d[1] == thr and d[2] == -thr and d[3] < thr < d[4]
    scale = f(1) / f(2)                                                   # loss_weight 1, N = 2
    # d == 0 and -0.0: quadratic, zero; |d| == thr: LINEAR (the comparison is strict); one ulp below: quadratic; one above: linear
    want_terms = [f(0), thr - lin, thr - lin, f(0.5) * s2 * d[3] * d[3], d[4] - lin, f(0.5) * s2 * d[5] * d[5], -d[6] - lin, f(0)]
    want_grad = [f(0) * scale, f(1) * scale, f(-1) * scale, s2 * d[3] * scale, f(1) * scale, s2 * d[5] * scale, f(-1) * scale, s2 * f(-0.0) * scale]
    assert np.array_equal(r32.terms[0], np.array(want_terms, f))
    assert r32.grad[0].tobytes() == np.array(want_grad, f).tobytes()
    # inside weight 0, outside weight non-zero: d = 0, no loss, no gradient; outside weight 0: neither
    assert (r32.terms[1, :4] == 0).all() and (r32.grad[1, :4] == 0).all()
    assert (r32.terms[1, 4:] != 0).all() and (r32.grad[1, 4:] != 0).all()


def test_softmax_equal_scores_are_exact():
    """Rows of equal scores with C = 2: e = 1, 1; s = 2; p = 0.5 in any arithmetic, so dscore = +-0.5 * scale exactly."""
    for key in ("1x2x135-equal-mixed", "2x2x65-equal-mixed", "5x2x1-equal-mixed"):
        c, (r32, r64) = LI.softmax_case(key), LI.softmax_ref(key)
        outer, C, inner = c["score"].shape
        valid, _, _, idx = L.classify_labels(c["ref_label"], C, LI.IGNORE)
        scale = np.float32(c["loss_weight"]) / r32.normalizer
        want = np.where(np.arange(2)[None, :, None] == idx[:, None, :], np.float32(-0.5), np.float32(0.5)) * scale
        want = np.where(valid[:, None, :], want, np.float32(0)).astype(np.float32)
        assert (r32.prob == 0.5).all()
        assert r32.grad.reshape(outer, C, inner).tobytes() == want.tobytes()
        assert (r64.prob == 0.5).all()                                   # and in float64: +-0.5 times its own scale
        assert (np.abs(r64.grad.reshape(outer, C, inner)) == np.where(valid[:, None, :], 0.5 * float(np.float32(c["loss_weight"])) / r64.normalizer, 0.0)).all()


def test_softmax_pm80_rows_clamp():
    r32, r64 = LI.softmax_ref("7x21x1-pm80-mixed")
    assert np.isfinite(r32.terms).all() and np.isfinite(r32.prob).all()
    assert (r32.terms == np.float32(CLAMP)).any() and (r64.terms == CLAMP).any()       # a losing class under the FLT_MIN clamp


@pytest.mark.parametrize("key", LI.SIGMOID_KEYS)
def test_sigmoid_ce_f32_statement_within_the_bound(key):
    c, (r32, r64) = LI.sigmoid_case(key), LI.sigmoid_ref(key)
    assert r32.terms.dtype == np.float32 and r32.grad.dtype == np.float32
    assert np.isfinite(r32.terms).all() and np.isfinite(r32.grad).all()
    err, lim = abs(float(r32.loss) - r64.loss), LI.loss_bound(r64)
    print("float32 statement: error %.3g, bound %.3g (%.1f %%)" % (err, lim, 100 * err / lim if lim else 0.0))
    assert err <= lim
    scale = c["loss_weight"] / c["x"].shape[0]
    assert np.abs(r32.grad - r64.grad).max() <= 8 * 2.0 ** -24 * scale
    if key != "tiny":
        x, t = c["x"], c["t"].reshape(c["x"].shape)
        w = np.ones(x.shape, np.float32) if c["w"] is None else c["w"].reshape(x.shape)
        over = x == -100                                                  # exp(-x) = inf: dx = -t * w * scale, the rule
        assert over.any() and np.array_equal(r32.grad[over], (-t * w * np.float32(scale))[over])
        if key == "mask":
            assert (r32.terms[4:] == 0).all() and (r32.grad[4:] == 0).all() and (r32.terms[:4, 1:4] != 0).any()


@pytest.mark.parametrize("count", LI.ELTWISE_COUNTS)
def test_eltwise_backward_statement(count):
    y, dy = LI.eltwise_case(count)
    relu = L.eltwise_backward_numpy(y, dy, "relu")
    assert relu.dtype == np.float32 and np.array_equal(relu[y > 0], dy[y > 0])
    assert (relu[~(y > 0)].view(np.uint32) == 0).all()                   # +0.0, also under y = -0.0
    sig = L.eltwise_backward_numpy(y, dy, "sigmoid")
    yt, dyt = _t(y), _t(dy)
    assert np.abs(sig - (dyt * yt * (1 - yt)).numpy()).max() <= 4 * 2.0 ** -24 * np.abs(dy).max() * 1.5
    assert sig.dtype == np.float32 and (sig[y == 1.0] == 0).all()
    assert np.array_equal(L.eltwise_backward_numpy(y, dy, 2), sig)


def test_invalid_labels_raise():
    score = np.zeros((4, 3), np.float32)
    for f in (L.softmax_loss_numpy, L.softmax_loss_f64):
        for bad in (3.0, 0.5, -2.0, np.nan, 3e9, np.inf):
            with pytest.raises(ValueError):
                f(score, np.array([0, 1, bad, 2], np.float32), LI.IGNORE)
        with pytest.raises(ValueError):                                   # no ignore label: -1 is not a class
            f(score, np.array([0, 1, -1, 2], np.float32), None)
        r = f(score, np.array([0, 1, -1, -1.5], np.float32), LI.IGNORE)   # (int)-1.5 is -1: ignored, as Caffe's cast has it
        assert r.count == 2
    valid, ignored, invalid, idx = L.classify_labels(np.array([0, 2, -1, 3, 1.5, np.nan, -1.5], np.float32), 3, -1)
    assert valid.tolist() == [True, True, False, False, False, False, False]
    assert ignored.tolist() == [False, False, True, False, False, False, True]
    assert invalid.tolist() == [False, False, False, True, True, True, False] and idx.tolist() == [0, 2, 0, 0, 0, 0, 0]


def test_shapes_that_do_not_fit_raise():
    z = np.zeros
    with pytest.raises(ValueError):
        L.softmax_loss_numpy(z((4, 3)), z(5))
    with pytest.raises(ValueError):
        L.softmax_loss_numpy(z((1, 2, 6, 5)), z((1, 1, 6, 4)))
    with pytest.raises(ValueError):
        L.softmax_loss_f64(z((2, 4097)), z(2))
    with pytest.raises(ValueError):
        L.softmax_loss_numpy(z(4), z(4))
    with pytest.raises(ValueError):
        L.smooth_l1_loss_numpy(z((2, 4)), z((2, 4)), z((2, 4)), z((2, 3)))
    with pytest.raises(ValueError):
        L.smooth_l1_loss_f64(z((2, 4)), z((4, 2)), z((2, 4)), z((2, 4)))
    with pytest.raises(ValueError):
        L.sigmoid_ce_loss_numpy(z((2, 441)), z((2, 1, 21, 20)))
    with pytest.raises(ValueError):
        L.sigmoid_ce_loss_f64(z((2, 441)), z((2, 1, 21, 21)), z((2, 440)))
    with pytest.raises(ValueError):
        L.eltwise_backward_numpy(z(4), z(5), "relu")
    with pytest.raises(ValueError):
        L.eltwise_backward_numpy(z(4), z(4), "tanh")
    # Caffe's shapes fit
    assert L.softmax_loss_numpy(z((1, 2, 18, 5)), z((1, 1, 18, 5))).terms.shape == (1, 90)
    assert L.softmax_loss_numpy(z((6, 21)), z((6, 1))).grad.shape == (6, 21) and L.softmax_loss_numpy(z((6, 21)), z(6)).count == 6
    assert L.sigmoid_ce_loss_numpy(z((2, 441)), z((2, 1, 21, 21)), z((2, 1, 21, 21))).grad.shape == (2, 441)
    e = L.softmax_loss_numpy(z((0, 21)), z(0))
    assert float(e.loss) == 0 and e.count == 0 and L.smooth_l1_loss_numpy(z((0, 4)), z((0, 4)), z((0, 4)), z((0, 4))).loss == 0
