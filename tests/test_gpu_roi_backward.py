"""csrc/roi_backward.hip on the GPU against the statements of mnc_amd/backward.py: bit for bit where the rule fixes the summation
order (warp dfeat, max pool, mask resize, mask pool dfeat), within the worst-case float32 bound of the float64 form where the
order is the launch's (drois, dmask); the same bytes on every run; every output element written; exact adjointness to the
existing forward kernel; the refusals."""
import ctypes

import numpy as np
import pytest

import roi_backward_inputs as RB
from gpu_util import Dev, from_c8, to_c8
from mnc_amd import _lib
from mnc_amd import backward as B
from mnc_amd.native_net import LayerConventions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def rhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def rchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def run_warp(dev, case, want_dfeat=True, want_drois=True, fill=np.nan):
    """mnc_roi_warp_backward through Dev.call on buffers pre-filled with `fill` -> (dfeat [C,H,W], drois [R,5]) as they come back."""
    feat, rois, PH, PW, scale, dtop = RB.args(case)
    C, H, W = feat.shape
    R = len(rois)
    mark = dev.mark()
    d_feat, d_rois, d_dtop = dev.put(to_c8(feat)), dev.put(rois), dev.put(rhwc(dtop))
    d_dfeat, d_drois = dev.empty((C, H, W), fill=fill), dev.empty((max(R, 1), 5), fill=fill)
    dev.call("mnc_roi_warp_backward", d_feat, C, H, W, d_rois, R, PH, PW, scale, d_dtop, d_dfeat if want_dfeat else None,
             d_drois if want_drois else None)
    dfeat, drois = from_c8(dev.get(d_dfeat, (C // 8, H, W, 8)), C, H, W), dev.get(d_drois, (max(R, 1), 5))[:R]
    dev.free_since(mark)
    return dfeat, drois


def _case(key):
    if key in ("head", "dyadic", "empty"):
        return {"head": RB.head_case, "dyadic": RB.dyadic_case, "empty": RB.empty_case}[key]()
    C, g = key.split("-")
    return RB.warp_case(int(C), *(int(v) for v in g.split("x")))


WARP_KEYS = ["%d-%dx%d" % c for c in RB.WARP_CASES] + ["head", "dyadic", "empty"]


@pytest.mark.parametrize("key", WARP_KEYS)
def test_warp_backward_against_the_statements(dev, key):
    case = _case(key)
    (dfeat32, _), (_, drois64, dabs, terms) = RB.warp_ref(key, case)
    dfeat, drois = run_warp(dev, case)
    assert not np.isnan(dfeat).any() and not np.isnan(drois).any()                    # every element written over the NaN fill
    assert np.array_equal(dfeat, dfeat32)
    err, lim = np.abs(drois - drois64), RB.bound(terms, dabs)
    print("drois: max error %.3g, at most %.3g of the bound" % (err.max() if err.size else 0, (err[lim > 0] / lim[lim > 0]).max() if (lim > 0).any() else 0))
    assert (err <= lim).all()
    assert (drois[:, 0] == 0).all()
    again = run_warp(dev, case, fill=3.0)
    assert again[0].tobytes() == dfeat.tobytes() and again[1].tobytes() == drois.tobytes()


def test_warp_backward_null_halves(dev):
    case = RB.warp_case(64, 14, 14)
    dfeat, drois = run_warp(dev, case)
    only_f = run_warp(dev, case, want_drois=False, fill=5.0)
    assert only_f[0].tobytes() == dfeat.tobytes() and (only_f[1] == 5.0).all()
    only_r = run_warp(dev, case, want_dfeat=False, fill=5.0)
    assert only_r[1].tobytes() == drois.tobytes() and (only_r[0] == 5.0).all()


def test_warp_backward_is_the_adjoint_of_the_forward_kernel(dev):
    """mnc_roi_warp and mnc_roi_warp_backward on the corpus where nothing rounds: sum(warp(F) * G) == sum(F * dfeat(G)), exactly."""
    case = RB.dyadic_case()
    feat, rois, PH, PW, scale, G = RB.args(case)
    C, H, W = feat.shape
    R = len(rois)
    dfeat = run_warp(dev, case)[0]
    mark = dev.mark()
    for F in (feat, np.roll(feat, 3, axis=2) * 2):
        d_out = dev.empty((R, PH, PW, C), fill=np.nan)
        dev.call("mnc_roi_warp", dev.put(to_c8(F)), C, H, W, dev.put(rois), R, PH, PW, scale, 0, d_out)
        out = rchw(dev.get(d_out, (R, PH, PW, C)))
        assert out.any() and float((out.astype(np.float64) * G).sum()) == float((F.astype(np.float64) * dfeat).sum())
    dev.free_since(mark)


def run_pool(dev, x, dout, fill=np.nan):
    R, C, PH, PW = x.shape
    mark = dev.mark()
    d_din = dev.empty(x.shape, fill=fill)
    dev.call("mnc_maxpool2_rhwc_backward", dev.put(rhwc(x)), dev.put(rhwc(dout)), d_din, R, PH, PW, C)
    din = rchw(dev.get(d_din, (R, PH, PW, C)))
    dev.free_since(mark)
    return din


@pytest.mark.parametrize("shape", RB.POOL_CASES)
def test_maxpool_backward(dev, shape):
    x, dout = RB.pool_case(*shape)
    din = run_pool(dev, x, dout)
    assert not np.isnan(din).any()
    assert din.tobytes() == B.maxpool2_backward_numpy(x, dout).tobytes()               # +0.0 for the losers: the bytes
    assert run_pool(dev, x, dout, fill=3.0).tobytes() == din.tobytes()


def run_resize(dev, dout, IH, IW, fill=np.nan):
    R, _, OH, OW = dout.shape
    mark = dev.mark()
    d_din = dev.empty((R, 1, IH, IW), fill=fill)
    dev.call("mnc_mask_resize_backward", dev.put(dout), d_din, R, IH, IW, OH, OW)
    din = dev.get(d_din, (R, 1, IH, IW))
    dev.free_since(mark)
    return din


@pytest.mark.parametrize("sizes", RB.RESIZE_CASES)
def test_mask_resize_backward(dev, sizes):
    IH, IW, OH, OW = sizes
    dout = RB.resize_case(*sizes)
    din = run_resize(dev, dout, IH, IW)
    assert not np.isnan(din).any()
    assert np.array_equal(din, B.mask_resize_backward_numpy(dout, IH, IW))
    assert run_resize(dev, dout, IH, IW, fill=3.0).tobytes() == din.tobytes()


def run_maskpool(dev, feat, mask, dtop, want_dfeat=True, want_dmask=True, fill=np.nan):
    R, C, PH, PW = feat.shape
    mark = dev.mark()
    d_dfeat, d_dmask = dev.empty(feat.shape, fill=fill), dev.empty(mask.shape, fill=fill)
    dev.call("mnc_mask_pool_backward", dev.put(rhwc(feat)), dev.put(mask), dev.put(rhwc(dtop)), d_dfeat if want_dfeat else None,
             d_dmask if want_dmask else None, R, PH, PW, C)
    dfeat, dmask = rchw(dev.get(d_dfeat, (R, PH, PW, C))), dev.get(d_dmask, mask.shape)
    dev.free_since(mark)
    return dfeat, dmask


@pytest.mark.parametrize("shape", RB.MASKPOOL_CASES)
def test_mask_pool_backward(dev, shape):
    feat, mask, dtop = RB.maskpool_case(*shape)
    dfeat, dmask = run_maskpool(dev, feat, mask, dtop)
    assert not np.isnan(dfeat).any() and not np.isnan(dmask).any()
    assert np.array_equal(dfeat, B.mask_pool_backward_numpy(feat, mask, dtop)[0])
    _, dmask64, dabs, terms = B.mask_pool_backward_f64(feat, mask, dtop)
    assert (np.abs(dmask - dmask64) <= RB.bound(terms, dabs)).all()
    again = run_maskpool(dev, feat, mask, dtop, fill=3.0)
    assert again[0].tobytes() == dfeat.tobytes() and again[1].tobytes() == dmask.tobytes()
    only_f = run_maskpool(dev, feat, mask, dtop, want_dmask=False, fill=5.0)
    assert only_f[0].tobytes() == dfeat.tobytes() and (only_f[1] == 5.0).all()
    only_m = run_maskpool(dev, feat, mask, dtop, want_dfeat=False, fill=5.0)
    assert only_m[1].tobytes() == dmask.tobytes() and (only_m[0] == 5.0).all()


def test_host_array_functions(dev):
    """mnc_amd.backward's device functions: the oracle's layouts in and out, ValueError for MNC_ERR_INVALID."""
    case = RB.warp_case(8, 3, 5)
    (dfeat32, _), (_, drois64, dabs, terms) = RB.warp_ref("8-3x5", case)
    dfeat, drois = B.roi_warp_backward(*RB.args(case), device_id=0)
    assert np.array_equal(dfeat, dfeat32) and (np.abs(drois - drois64) <= RB.bound(terms, dabs)).all()
    e = RB.empty_case()
    dfeat, drois = B.roi_warp_backward(*RB.args(e), device_id=0)
    assert dfeat.shape == e["feat"].shape and not dfeat.any() and drois.shape == (0, 5)
    x, dout = RB.pool_case(*RB.POOL_CASES[0])
    assert np.array_equal(B.maxpool2_backward(x, dout, device_id=0), B.maxpool2_backward_numpy(x, dout))
    g = RB.resize_case(21, 21, 14, 14)
    assert np.array_equal(B.mask_resize_backward(g, 21, 21, device_id=0), B.mask_resize_backward_numpy(g, 21, 21))
    feat, mask, dtop = RB.maskpool_case(*RB.MASKPOOL_CASES[1])
    dfeat, dmask = B.mask_pool_backward(feat, mask, dtop, device_id=0)
    _, dmask64, mabs, mterms = B.mask_pool_backward_f64(feat, mask, dtop)
    assert np.array_equal(dfeat, dtop * mask) and (np.abs(dmask - dmask64) <= RB.bound(mterms, mabs)).all()
    with pytest.raises(ValueError):                                                  # C % 4: the library's own check
        B.maxpool2_backward(x[:, :3], dout[:, :3], device_id=0)
    with pytest.raises(ValueError):
        B.roi_warp_backward(case["feat"][:4], case["rois"], 3, 5, RB.SCALE, case["dtop"][:, :4], device_id=0)


def _refused(dev, code, name, *args):
    with pytest.raises(_lib.MncError) as e:
        dev.call(name, *args)
    assert e.value.code == code, (name, e.value)


def test_refusals_leave_the_outputs_alone(dev):
    """Bad sizes: MNC_ERR_INVALID (1); a convention other than the SPEC's: MNC_ERR_UNSUPPORTED (5); both before any launch."""
    case = RB.warp_case(8, 7, 7)
    feat, rois, PH, PW, scale, dtop = RB.args(case)
    C, H, W = feat.shape
    R = len(rois)
    mark = dev.mark()
    d_feat, d_rois, d_dtop = dev.put(to_c8(feat)), dev.put(rois), dev.put(rhwc(dtop))
    n = max(feat.size, dtop.size)
    d_a, d_b = dev.empty((n,), fill=7.0), dev.empty((n,), fill=7.0)
    warp = lambda **k: [k.get("feat", d_feat), k.get("C", C), k.get("H", H), W, k.get("rois", d_rois), k.get("R", R), k.get("PH", PH), PW,
                        scale, k.get("dtop", d_dtop), k.get("dfeat", d_a), k.get("drois", d_b)]
    invalid = [("mnc_roi_warp_backward", warp(C=12)), ("mnc_roi_warp_backward", warp(H=0)), ("mnc_roi_warp_backward", warp(R=-1)),
               ("mnc_roi_warp_backward", warp(PH=0)), ("mnc_roi_warp_backward", warp(PH=40000)),
               ("mnc_roi_warp_backward", warp(dfeat=None, drois=None)), ("mnc_roi_warp_backward", warp(dtop=None)),
               ("mnc_roi_warp_backward", warp(feat=None)), ("mnc_roi_warp_backward", warp(rois=None)),
               ("mnc_maxpool2_rhwc_backward", [d_dtop, d_dtop, d_a, R, 7, 6, C]), ("mnc_maxpool2_rhwc_backward", [d_dtop, d_dtop, d_a, R, 6, 6, 6]),
               ("mnc_maxpool2_rhwc_backward", [d_dtop, d_dtop, None, R, 6, 6, C]),
               ("mnc_mask_resize_backward", [d_dtop, d_a, R, 1, 7, 7, 7]), ("mnc_mask_resize_backward", [d_dtop, d_a, R, 7, 7, 0, 7]),
               ("mnc_mask_resize_backward", [None, d_a, R, 7, 7, 7, 7]),
               ("mnc_mask_pool_backward", [d_dtop, d_dtop, d_dtop, d_a, d_b, R, 7, 7, 6]),
               ("mnc_mask_pool_backward", [d_dtop, d_dtop, d_dtop, None, None, R, 7, 7, C]),
               ("mnc_mask_pool_backward", [None, d_dtop, d_dtop, d_a, d_b, R, 7, 7, C])]
    for name, a in invalid:
        _refused(dev, 1, name, *a)
    try:
        for field, name, a in (("warp_sample", "mnc_roi_warp_backward", warp()), ("warp_round_edges", "mnc_roi_warp_backward", warp()),
                               ("warp_no_plus_one", "mnc_roi_warp_backward", warp()), ("warp_oob", "mnc_roi_warp_backward", warp()),
                               ("resize_mode", "mnc_mask_resize_backward", [d_dtop, d_a, R, 7, 7, 7, 7]),
                               ("maskpool_binary", "mnc_mask_pool_backward", [d_dtop, d_dtop, d_dtop, d_a, d_b, R, 7, 7, C])):
            c = LayerConventions.make({field: 1})
            dev.call("mnc_ctx_set_layer_conventions", ctypes.addressof(c))
            _refused(dev, 5, name, *a)
    finally:
        dev.call("mnc_ctx_set_layer_conventions", None)
    assert (dev.get(d_a, (n,)) == 7.0).all() and (dev.get(d_b, (n,)) == 7.0).all()
    dev.free_since(mark)
