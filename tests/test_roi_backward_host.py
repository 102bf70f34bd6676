"""The statements of mnc_amd/backward.py on the CPU: the float64 forms against torch autograd and central finite differences of a
float64 restatement of oracle/SPEC.md sections 1-3 written here, the float32 statements against the float64 forms within the
worst-case rounding bound, and adjointness to the oracle's forward layers, exactly, on a corpus without rounding."""
import numpy as np
import pytest
import torch

import roi_backward_inputs as RB
from mnc_amd import backward as B
from oracle import native

F64 = torch.float64


# ---- the restatement: SPEC.md 1-3 in differentiable float64, floor detached ----

def _positions32(rois, P, scale, lo, hi):
    """The forward's float32 sample positions of one axis, in its operation order."""
    f = np.float32
    a, b = rois[:, lo].astype(f) * f(scale), rois[:, hi].astype(f) * f(scale)
    step = np.maximum(b - a + f(1), f(1)) / f(P)
    return a[:, None] + np.arange(P, dtype=f)[None, :] * step[:, None]


def warp_torch(feat, rois, PH, PW, scale, at32=None):
    """feat [C,H,W], rois [R,5] float64 tensors -> [R,C,PH,PW].  at32 = (sx32, sy32): evaluate at those positions (the cells are
    theirs, the positions are moved onto them by a detached shift, so the derivatives are the restatement's)."""
    C, H, W = feat.shape
    s = float(np.float32(scale))

    def axis(lo, hi, P, pos):
        a, b = rois[:, lo] * s, rois[:, hi] * s
        step = torch.clamp(b - a + 1, min=1) / P
        p = a[:, None] + torch.arange(P, dtype=F64)[None, :] * step[:, None]
        if pos is not None:
            pos = torch.as_tensor(pos.astype(np.float64))
            p = p + (pos - p).detach()
            cell = torch.floor(pos)
        else:
            cell = torch.floor(p).detach()
        return cell.long(), p - cell

    x0, ax = axis(1, 3, PW, None if at32 is None else at32[0])
    y0, ay = axis(2, 4, PH, None if at32 is None else at32[1])

    def tap(dy, dx):
        yy, xx = (y0 + dy)[:, :, None], (x0 + dx)[:, None, :]
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = feat[:, yy.clamp(0, H - 1).expand(-1, -1, PW), xx.clamp(0, W - 1).expand(-1, PH, -1)]        # [C,R,PH,PW]
        return v * ok[None]

    ax, ay = ax[None, :, None, :], ay[None, :, :, None]
    out = (1 - ax) * (1 - ay) * tap(0, 0) + ax * (1 - ay) * tap(0, 1) + (1 - ax) * ay * tap(1, 0) + ax * ay * tap(1, 1)
    return out.permute(1, 0, 2, 3)


def warp_autograd(case, at32):
    feat = torch.tensor(case["feat"].astype(np.float64), requires_grad=True)
    rois = torch.tensor(case["rois"].astype(np.float64), requires_grad=True)
    pos = None
    if at32:
        pos = (_positions32(case["rois"], case["PW"], case["scale"], 1, 3), _positions32(case["rois"], case["PH"], case["scale"], 2, 4))
    with torch.enable_grad():                   # (another module of the suite may have switched autograd off for the process)
        out = warp_torch(feat, rois, case["PH"], case["PW"], case["scale"], pos)
        (out * torch.tensor(case["dtop"].astype(np.float64))).sum().backward()
    return feat.grad.numpy(), rois.grad.numpy()


def resize_torch(m, OH, OW):
    """SPEC.md 2 on [R,1,IH,IW] float64 (the source positions are float32 constants, as in the forward)."""
    R, _, IH, IW = m.shape
    rows = []
    for h in range(OH):
        iy = np.float32(h) * (np.float32(IH) / np.float32(OH))
        sy = int(np.floor(iy))
        fy = float(iy - np.float32(sy))
        row = []
        for w in range(OW):
            ix = np.float32(w) * (np.float32(IW) / np.float32(OW))
            sx = int(np.floor(ix))
            fx = float(ix - np.float32(sx))
            if sx == IW - 1 or sy == IH - 1:
                row.append(m[:, 0, sy, sx])
            else:
                row.append((1 - fx) * (1 - fy) * m[:, 0, sy, sx] + fx * (1 - fy) * m[:, 0, sy, sx + 1] +
                           (1 - fx) * fy * m[:, 0, sy + 1, sx] + fx * fy * m[:, 0, sy + 1, sx + 1])
        rows.append(torch.stack(row, -1))
    return torch.stack(rows, -2)[:, None]


def _rel(got, want):
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1.0) if want.size else 0.0


AUTOGRAD_CASES = [(C, PH, PW) for C, PH, PW in RB.WARP_CASES if C <= 64]


@pytest.mark.parametrize("geometry", ["float64", "float32"])
@pytest.mark.parametrize("C,PH,PW", AUTOGRAD_CASES)
def test_f64_statement_is_the_autograd_of_the_spec(C, PH, PW, geometry):
    """geometry="float64" against the restatement as it stands; geometry="float32" (the form the kernels are held to) against
    the restatement recomputed at the float32 positions: dfeat to 1e-12, drois to 1e-9 of the largest entry."""
    case = RB.warp_case(C, PH, PW)
    dfeat, drois, dabs, terms = B.roi_warp_backward_f64(*RB.args(case), geometry=geometry)
    want_f, want_r = warp_autograd(case, at32=geometry == "float32")
    assert np.abs(want_r).max() > 1.0 and np.abs(want_f).max() > 1.0
    print("dfeat rel %.3g  drois rel %.3g" % (_rel(dfeat, want_f), _rel(drois, want_r)))
    assert _rel(dfeat, want_f) <= 1e-12
    assert _rel(drois, want_r) <= 1e-9
    assert (drois[:, 0] == 0).all() and (dabs >= np.abs(drois)).all() and (terms[:, 1:] == 4 * C * PH * PW).all()
    if geometry == "float64":
        # the two geometries differ by the float32 rounding of the sample positions and by nothing else
        d32 = B.roi_warp_backward_f64(*RB.args(case))[0]
        assert 0 < np.abs(d32 - dfeat).max() <= 1e-5 * np.abs(dfeat).max()


def test_subgradient_of_the_width_clamp():
    """Malformed box (x2 < x1): the whole of Gx goes to x1, x2 gets exactly 0; the tied clamp (width exactly 1) is free, as torch's
    clamp(min=1) has it; a box wholly outside the map has no gradient at all."""
    case = RB.warp_case(8, 7, 7)
    for fn in (B.roi_warp_backward_numpy, lambda *a: B.roi_warp_backward_f64(*a)[:2]):
        _, drois = fn(*RB.args(case))
        assert drois[3, 3] == 0 and drois[3, 1] != 0 and drois[3, 4] != 0
        assert drois[2, 3] != 0 and drois[2, 4] != 0
        assert (drois[5] == 0).all()


@pytest.mark.parametrize("PH,PW", RB.GRIDS)
def test_central_finite_differences(PH, PW):
    """drois against central differences of the float64 forward restatement, on the RoIs that are smooth within the step: every
    sample farther than the step from an integer, no size within the step of the clamp.  Between kinks the forward is a
    polynomial of degree two in the box, so central differences are exact up to rounding."""
    case = RB.warp_case(8, PH, PW)
    h = 1e-3                                                   # image pixels
    step = 2 * h * RB.SCALE                                    # how far a sample can move, feature-map cells (both edges move it)
    rois = case["rois"].astype(np.float64)
    s = float(np.float32(RB.SCALE))
    smooth = []
    for r, (_, x1, y1, x2, y2) in enumerate(rois):
        ok = True
        for lo, hi, P in ((x1, x2, PW), (y1, y2, PH)):
            ext = hi * s - lo * s + 1
            pos = lo * s + np.arange(P) * (max(ext, 1.0) / P)
            ok = ok and abs(ext - 1) > step and np.abs(pos - np.round(pos)).min() > step
        if ok:
            smooth.append(r)
    print("smooth RoIs:", smooth)
    assert 2 * len(smooth) >= len(rois)
    feat, G = torch.tensor(case["feat"].astype(np.float64)), torch.tensor(case["dtop"].astype(np.float64))
    loss = lambda rr: float((warp_torch(feat, torch.tensor(rr), PH, PW, RB.SCALE) * G).sum())
    drois = B.roi_warp_backward_f64(*RB.args(case), geometry="float64")[1]
    fd = np.zeros_like(drois)
    for r in smooth:
        for k in range(1, 5):
            up, dn = rois.copy(), rois.copy()
            up[r, k] += h
            dn[r, k] -= h
            fd[r, k] = (loss(up) - loss(dn)) / (2 * h)
    assert np.abs(fd[smooth]).max() > 1e-2
    print("finite differences: max abs diff %.3g of %.3g" % (np.abs(fd[smooth] - drois[smooth]).max(), np.abs(drois[smooth]).max()))
    assert np.abs(fd[smooth] - drois[smooth]).max() <= 1e-7 * np.abs(drois[smooth]).max()


@pytest.mark.parametrize("key", ["%d-%dx%d" % c for c in RB.WARP_CASES] + ["head", "dyadic", "empty"])
def test_f32_statement_within_the_rounding_bound_of_the_f64_form(key):
    """(terms + 32) * 2^-24 * abs: the worst case of ANY float32 summation of `terms` addends, 32 for the roundings inside one."""
    case = {"head": RB.head_case, "dyadic": RB.dyadic_case, "empty": RB.empty_case}.get(key, lambda: None)()
    if case is None:
        C, g = key.split("-")
        case = RB.warp_case(int(C), *(int(v) for v in g.split("x")))
    (dfeat32, drois32), (dfeat64, drois64, dabs, terms) = RB.warp_ref(key, case)
    assert dfeat32.dtype == np.float32 and drois32.dtype == np.float32 and dfeat32.shape == case["feat"].shape
    assert (np.abs(drois32 - drois64) <= RB.bound(terms, dabs)).all(), np.abs(drois32 - drois64).max()
    Hh, Ww = case["feat"].shape[1:]
    counts = B.roi_warp_tap_counts(case["rois"], case["PH"], case["PW"], case["scale"], Hh, Ww)
    fabs = B.roi_warp_backward_f64(case["feat"], case["rois"], case["PH"], case["PW"], case["scale"], np.abs(case["dtop"]))[0]
    assert (np.abs(dfeat32 - dfeat64) <= RB.bound(counts[None], fabs)).all(), np.abs(dfeat32 - dfeat64).max()
    assert (dfeat32[:, counts == 0] == 0).all()
    if key == "dyadic":
        assert np.array_equal(dfeat32, dfeat64)                   # (not drois: tx = pw / 14 rounds)
    if key == "empty":
        assert drois32.shape == (0, 5) and not dfeat32.any()


def test_warp_adjoint_to_the_oracle_forward_exactly():
    """sum(roi_warp(F) * G) == sum(F * dfeat(G)) where nothing rounds -- and with a second F, so that it is the adjoint of the map."""
    case = RB.dyadic_case()
    F, G = case["feat"], case["dtop"]
    dfeat = B.roi_warp_backward_numpy(*RB.args(case))[0]
    for feat in (F, np.roll(F, 3, axis=2) * 2):
        out = native.roi_warp(feat, case["rois"], 14, 14, RB.SCALE)
        assert out.any() and float((out.astype(np.float64) * G).sum()) == float((feat.astype(np.float64) * dfeat).sum())


def test_mask_resize_backward():
    rng = np.random.default_rng(2)
    for IH, IW, OH, OW in RB.RESIZE_CASES:
        dout = RB.resize_case(IH, IW, OH, OW)
        din = B.mask_resize_backward_numpy(dout, IH, IW)
        m = torch.tensor(rng.standard_normal((dout.shape[0], 1, IH, IW)), requires_grad=True)
        with torch.enable_grad():
            out = resize_torch(m, OH, OW)
            (out * torch.tensor(dout.astype(np.float64))).sum().backward()
        assert float(np.abs(out.detach().numpy() - native.mask_resize(m.detach().numpy().astype(np.float32), OH, OW)).max()) < 1e-5
        want = m.grad.numpy()
        m2 = torch.tensor(np.zeros((dout.shape[0], 1, IH, IW)), requires_grad=True)
        with torch.enable_grad():
            (resize_torch(m2, OH, OW) * torch.tensor(np.abs(dout).astype(np.float64))).sum().backward()
        counts = B.mask_resize_tap_counts(IH, IW, OH, OW)
        assert din.dtype == np.float32 and counts.sum() >= OH * OW
        assert (np.abs(din - want) <= RB.bound(counts[None, None], m2.grad.numpy())).all(), (IH, IW, OH, OW)
    # adjoint to the oracle's forward, exactly: 21 -> 14 has fractions 0 and 0.5 only
    M = rng.integers(-4, 5, (3, 1, 21, 21)).astype(np.float32)
    G = rng.integers(-3, 4, (3, 1, 14, 14)).astype(np.float32)
    lhs = (native.mask_resize(M, 14, 14).astype(np.float64) * G).sum()
    assert lhs != 0 and float(lhs) == float((M.astype(np.float64) * B.mask_resize_backward_numpy(G, 21, 21)).sum())


def test_mask_resize_edge_rule_is_hit():
    """IH = OH: the ratio is 1, every output reads its own cell, and the last row and column take the nearest rule with weight 1 --
    the gradient is dout itself.  With IW = OW only, the last column is nearest in both directions: row floor(iy) gets all of it."""
    dout = RB.resize_case(14, 14, 14, 14)
    assert np.array_equal(B.mask_resize_backward_numpy(dout, 14, 14), dout)
    g = RB.resize_case(5, 7, 9, 7)
    want = np.zeros((g.shape[0], 5), np.float32)
    for h in range(9):
        want[:, int(np.floor(np.float32(h) * (np.float32(5) / np.float32(9))))] += g[:, 0, h, 6]
    assert np.array_equal(B.mask_resize_backward_numpy(g, 5, 7)[:, 0, :, 6], want)


def test_maxpool_gradient_goes_to_the_first_maximum():
    for shape in RB.POOL_CASES:
        x, dout = RB.pool_case(*shape)
        din = B.maxpool2_backward_numpy(x, dout)
        assert din.shape == x.shape and din.dtype == np.float32
        win = np.stack([din[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)])
        xin = np.stack([x[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)])
        assert np.array_equal(win.sum(0), dout) and ((win != 0).sum(0) <= 1).all()
        first = np.argmax(xin, axis=0)                            # numpy's argmax takes the first of equal maxima
        assert np.array_equal(np.take_along_axis(win, first[None], 0)[0], dout)
        assert native.maxpool2(x).shape == dout.shape and np.array_equal(np.take_along_axis(xin, first[None], 0)[0], native.maxpool2(x))
    x, dout = RB.pool_case(*RB.POOL_CASES[0])
    din = B.maxpool2_backward_numpy(x, dout)
    assert din[0, 0, 0, 0] == dout[0, 0, 0, 0] and not din[0, 0, 0, 1] and not din[0, 0, 1, 0] and not din[0, 0, 1, 1]
    assert not np.signbit(din[din == 0]).any()                   # the losers get +0.0


def test_mask_pool_backward():
    for shape in RB.MASKPOOL_CASES:
        feat, mask, dtop = RB.maskpool_case(*shape)
        f = torch.tensor(feat.astype(np.float64), requires_grad=True)
        m = torch.tensor(mask.astype(np.float64), requires_grad=True)
        with torch.enable_grad():
            (f * m * torch.tensor(dtop.astype(np.float64))).sum().backward()
        dfeat64, dmask64, dabs, terms = B.mask_pool_backward_f64(feat, mask, dtop)
        assert _rel(dfeat64, f.grad.numpy()) <= 1e-12 and _rel(dmask64, m.grad.numpy()) <= 1e-12
        dfeat, dmask = B.mask_pool_backward_numpy(feat, mask, dtop)
        assert dfeat.dtype == np.float32 and dmask.shape == mask.shape and (terms == shape[1]).all()
        assert np.array_equal(dfeat, dtop * mask)
        assert (np.abs(dmask - dmask64) <= RB.bound(terms, dabs)).all()
    # adjoint in feat to the oracle's forward, exactly
    rng = np.random.default_rng(4)
    F = rng.integers(-4, 5, (2, 8, 3, 5)).astype(np.float32)
    M = (rng.integers(0, 5, (2, 1, 3, 5)) / 4.0).astype(np.float32)
    G = rng.integers(-3, 4, F.shape).astype(np.float32)
    lhs = (native.mask_pool(F, M).astype(np.float64) * G).sum()
    assert lhs != 0 and float(lhs) == float((F.astype(np.float64) * B.mask_pool_backward_numpy(F, M, G)[0]).sum())


def test_statements_refuse_what_does_not_fit():
    case = RB.warp_case(8, 7, 7)
    feat, rois, PH, PW, scale, dtop = RB.args(case)
    for fn in (B.roi_warp_backward_numpy, B.roi_warp_backward_f64):
        with pytest.raises(ValueError):
            fn(feat, rois, PH, PW + 1, scale, dtop)
        with pytest.raises(ValueError):
            fn(feat, rois[:3], PH, PW, scale, dtop)
        bad = rois.copy()
        bad[1, 2] = np.nan
        with pytest.raises(ValueError):
            fn(feat, bad, PH, PW, scale, dtop)
    x, dout = RB.pool_case(*RB.POOL_CASES[0])
    with pytest.raises(ValueError):
        B.maxpool2_backward_numpy(x[:, :, :5], dout)
    with pytest.raises(ValueError):
        B.mask_resize_backward_numpy(RB.resize_case(21, 21, 14, 14), 1, 21)
    f, m, d = RB.maskpool_case(*RB.MASKPOOL_CASES[0])
    with pytest.raises(ValueError):
        B.mask_pool_backward_numpy(f, m[:, :, :2], d)
