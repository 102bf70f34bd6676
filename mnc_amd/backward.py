"""Backward passes of the per-RoI layers that are MNC's own (include/mnc_hip.h n24, csrc/roi_backward.hip): ROIWarping with
respect to the feature map AND to the box, the MAX 2x2/2 pooling behind the 28x28 warp, MaskResize and MaskPooling -- the
derivatives of oracle/SPEC.md sections 1-3 under the SPEC's default conventions.

    roi_warp_backward_numpy(feat, rois, PH, PW, scale, dtop)  -> (dfeat [C,H,W], drois [R,5]): the float32 statement
    roi_warp_backward_f64(...)                                -> (dfeat, drois, drois_abs, drois_terms) in float64
    roi_warp_backward(..., device_id=None)                    the same through mnc_roi_warp_backward (the GPU)
    maxpool2_backward_numpy(x, dout) / maxpool2_backward(...)             x [R,C,PH,PW], dout [R,C,PH/2,PW/2] -> din [R,C,PH,PW]
    mask_resize_backward_numpy(dout, IH, IW) / mask_resize_backward(...)  dout [R,1,OH,OW] -> din [R,1,IH,IW]
    mask_pool_backward_numpy(feat, mask, dtop) / mask_pool_backward(...)  -> (dfeat [R,C,PH,PW], dmask [R,1,PH,PW])
    mask_pool_backward_f64(...)                               -> (dfeat, dmask, dmask_abs, dmask_terms) in float64
    roi_warp_tap_counts / mask_resize_tap_counts              the number of addends of every dfeat / din element
    kernel_times(fn)                                          the launches of fn() on the device's context and their device times

Arrays are in the oracle's layouts (feat [C,H,W], per-RoI tensors [R,C,PH,PW], rois [R,5] with the batch index first); the device
functions change layouts inside.  There is no fallback: without the library or a GPU the device functions raise; what the
library refuses as MNC_ERR_INVALID is a ValueError.

The rules.  floor is piecewise constant, so a sample's cell (x0, y0) is a constant and its position enters only through
ax = sx - x0, ay = sy - y0.  The float32 quantities x1s, y1s, bw, bh, sx, sy, x0, y0, ax, ay are the forward's own: the identical
expressions in the identical order as csrc/roi.hip and oracle/mnc_oracle.c.

    warp dfeat   dfeat[c, y, x] = sum of w * g over all (r, ph, pw, tap) whose tap lands on (y, x), g = dtop[r, c, ph, pw],
                 w00 = (1-ax)(1-ay), w01 = ax(1-ay), w10 = (1-ax)ay, w11 = ax ay formed as in the forward, then times g; taps
                 outside the map are dropped.  The ORDER is part of the rule: ascending r, then ph, then pw, within a sample
                 00, 01, 10, 11; float32 from +0.0, no contraction.  The kernel equals this statement bit for bit.
    warp drois   drois[r, 0] = 0.  Per sample dsx_c = (1-ay)(F01-F00) + ay(F11-F10), dsy_c = (1-ax)(F10-F00) + ax(F11-F01),
                 Gx = sum_c g dsx_c, Gy = sum_c g dsy_c; drois[r,1] += scale (1-tx) Gx, [r,3] += scale tx Gx, [r,2] += scale (1-ty) Gy,
                 [r,4] += scale ty Gy; tx = pw / PW when the width is free, else 0 (ty alike).  Free: the float32 value
                 x2s - x1s + 1 is >= 1 (the max(., 1) clamp inactive or tied: the sub-gradient torch's clamp(min=1) takes); a
                 clamped width sends all of Gx to x1.  The order of this sum is the implementation's (here numpy's, on the GPU
                 the launch geometry's): statement and kernel agree within the rounding bound below, not bit for bit.
    max pool     the gradient of an output goes to the FIRST maximum of its 2x2 window in the order (0,0), (0,1), (1,0), (1,1): a
                 later element wins only when strictly greater (the forward's order, Caffe's rule); the other three get +0.0.
    mask resize  din[r, iy, ix] = sum over (h, w), ascending h then w, of weight * dout[r, h, w], the weight SPEC section 2's: the
                 bilinear four, or 1 on the nearest cell when sx == IW - 1 or sy == IH - 1.  Bit for bit.
    mask pool    dfeat = dtop * mask (bit for bit); dmask[r, h, w] = sum_c dtop * feat, order the implementation's.

The float64 forms.  Their geometry is the float32 one promoted (geometry="float32", the default: the gradient AT the positions the
forward sampled) or float64 arithmetic on the same float32 inputs (geometry="float64": what float64 autograd of the SPEC gives).
drois_abs / dmask_abs is the float64 sum of the absolute values of the addends of each entry and *_terms their number, for the
worst-case bound of ANY float32 evaluation: |float32 result - float64 result| <= (terms + 32) * 2^-24 * abs.  So that the bound
also covers the cancellation inside a slope, an addend of drois is one product scale * t * g * weight * F (four per sample and
channel: the two differences of a slope written out), not the slope as a whole."""
import ctypes
import threading

import numpy as np

from . import _lib


# ---- geometry: the forward's own expressions ----

def _rois(rois):
    r = np.ascontiguousarray(np.asarray(rois, np.float32).reshape(-1, 5))
    if not np.isfinite(r[:, 1:]).all():
        raise ValueError("roi_warp_backward: a RoI coordinate is not finite")
    return r


def _axis(lo, hi, P, scale, dt):
    """One axis of all RoIs, in dtype dt, in the forward's operation order -> (cell int64 [R,P], fraction [R,P], free bool [R])."""
    a, b = lo.astype(dt) * dt(scale), hi.astype(dt) * dt(scale)
    ext = b - a + dt(1)
    size = np.maximum(ext, dt(1))
    step = size / dt(P)
    s = a[:, None] + np.arange(P, dtype=dt)[None, :] * step[:, None]
    c = np.floor(s)
    return c.astype(np.int64), s - c, ext >= dt(1)


def _geometry(rois, PH, PW, scale, geometry="float32"):
    if geometry not in ("float32", "float64"):
        raise ValueError("geometry is 'float32' or 'float64'")
    dt = np.float32 if geometry == "float32" else np.float64
    scale = np.float32(scale)
    x0, ax, fw = _axis(rois[:, 1], rois[:, 3], PW, scale, dt)
    y0, ay, fh = _axis(rois[:, 2], rois[:, 4], PH, scale, dt)
    return x0, ax, fw, y0, ay, fh


def _warp_args(feat, rois, PH, PW, dtop):
    feat = np.asarray(feat, np.float32)
    if feat.ndim == 4 and feat.shape[0] == 1:
        feat = feat[0]
    rois = _rois(rois)
    dtop = np.asarray(dtop, np.float32)
    PH, PW = int(PH), int(PW)
    if feat.ndim != 3 or PH < 1 or PW < 1 or dtop.shape != (rois.shape[0], feat.shape[0], PH, PW):
        raise ValueError("roi_warp_backward: feat %s, %d rois, %d x %d and dtop %s do not fit" % (feat.shape, rois.shape[0], PH, PW,
                                                                                                  dtop.shape))
    return feat, rois, PH, PW, dtop


def _taps(feat, y0, x0):
    """The four taps of every sample of one RoI, zero outside the map: feat [C,H,W], y0 [PH], x0 [PW] -> 4 x [C,PH,PW]."""
    C, H, W = feat.shape
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = y0 + dy, x0 + dx
            ok = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
            v = feat[:, np.clip(yy, 0, H - 1)[:, None], np.clip(xx, 0, W - 1)[None, :]]
            out.append(np.where(ok[None], v, feat.dtype.type(0)))
    return out


# ---- the statements ----

def roi_warp_backward_numpy(feat, rois, PH, PW, scale, dtop):
    """The float32 statement -- the specification csrc/roi_backward.hip is tested against.  -> (dfeat [C,H,W], drois [R,5])."""
    feat, rois, PH, PW, dtop = _warp_args(feat, rois, PH, PW, dtop)
    C, H, W = feat.shape
    R = rois.shape[0]
    f1 = np.float32(1)
    x0, ax, fw, y0, ay, fh = _geometry(rois, PH, PW, scale)
    g_all = np.ascontiguousarray(dtop.transpose(0, 2, 3, 1))
    acc = np.zeros((H, W, C), np.float32)
    for r in range(R):
        for ph in range(PH):
            yy, b = int(y0[r, ph]), ay[r, ph]
            if yy < -1 or yy >= H:
                continue
            for pw in range(PW):
                xx, a = int(x0[r, pw]), ax[r, pw]
                if xx < -1 or xx >= W:
                    continue
                g = g_all[r, ph, pw]
                w = ((f1 - a) * (f1 - b), a * (f1 - b), (f1 - a) * b, a * b)
                for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    if 0 <= yy + dy < H and 0 <= xx + dx < W:
                        acc[yy + dy, xx + dx] += w[k] * g
    dfeat = np.ascontiguousarray(acc.transpose(2, 0, 1))
    drois = np.zeros((R, 5), np.float32)
    s = np.float32(scale)
    for r in range(R):
        f00, f01, f10, f11 = _taps(feat, y0[r], x0[r])
        a, b = ax[r][None, None, :], ay[r][None, :, None]
        g = dtop[r]
        gx = (g * ((f1 - b) * (f01 - f00) + b * (f11 - f10))).sum(axis=0, dtype=np.float32)
        gy = (g * ((f1 - a) * (f10 - f00) + a * (f11 - f01))).sum(axis=0, dtype=np.float32)
        tx = (np.arange(PW, dtype=np.float32) / np.float32(PW) if fw[r] else np.zeros(PW, np.float32))[None, :]
        ty = (np.arange(PH, dtype=np.float32) / np.float32(PH) if fh[r] else np.zeros(PH, np.float32))[:, None]
        drois[r, 1] = s * ((f1 - tx) * gx).sum(dtype=np.float32)
        drois[r, 3] = s * (tx * gx).sum(dtype=np.float32)
        drois[r, 2] = s * ((f1 - ty) * gy).sum(dtype=np.float32)
        drois[r, 4] = s * (ty * gy).sum(dtype=np.float32)
    return dfeat, drois


def _scatter_taps(H, W, x0, ax, y0, ay, values):
    """sum of weight * values[r, ph, pw] over the taps inside the map, per cell: values [R,PH,PW,K] float64 (None: count the taps)
    -> [H*W, K] float64 (int64 [H*W] when counting)."""
    out = np.zeros(H * W, np.int64) if values is None else np.zeros((H * W, values.shape[-1]), np.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = (y0 + dy)[:, :, None], (x0 + dx)[:, None, :]
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            idx = (yy * W + xx)[ok]
            if values is None:
                np.add.at(out, idx, 1)
            else:
                w = (ay if dy else 1.0 - ay)[:, :, None] * (ax if dx else 1.0 - ax)[:, None, :]
                np.add.at(out, idx, (w[..., None] * values)[ok])
    return out


def roi_warp_tap_counts(rois, PH, PW, scale, H, W):
    """-> int64 [H, W]: the number of addends of dfeat[:, y, x] (the taps of all samples of all RoIs that land on the cell)."""
    x0, _, _, y0, _, _ = _geometry(_rois(rois), int(PH), int(PW), scale)
    return _scatter_taps(H, W, x0, None, y0, None, None).reshape(H, W)


def roi_warp_backward_f64(feat, rois, PH, PW, scale, dtop, geometry="float32"):
    """The float64 form -> (dfeat [C,H,W], drois [R,5], drois_abs [R,5], drois_terms int64 [R,5]); see the module text."""
    feat, rois, PH, PW, dtop = _warp_args(feat, rois, PH, PW, dtop)
    C, H, W = feat.shape
    R = rois.shape[0]
    x0, ax, fw, y0, ay, fh = _geometry(rois, PH, PW, scale, geometry)
    ax, ay = ax.astype(np.float64), ay.astype(np.float64)
    feat, dtop = feat.astype(np.float64), dtop.astype(np.float64)
    dfeat = _scatter_taps(H, W, x0, ax, y0, ay, dtop.transpose(0, 2, 3, 1)).reshape(H, W, C).transpose(2, 0, 1)
    drois, dabs = np.zeros((R, 5)), np.zeros((R, 5))
    terms = np.zeros((R, 5), np.int64)
    terms[:, 1:] = 4 * C * PH * PW
    s = float(np.float32(scale))
    for r in range(R):
        f00, f01, f10, f11 = _taps(feat, y0[r], x0[r])
        a, b = ax[r][None, None, :], ay[r][None, :, None]
        g = dtop[r]
        gx = (g * ((1 - b) * (f01 - f00) + b * (f11 - f10))).sum(axis=0)
        gy = (g * ((1 - a) * (f10 - f00) + a * (f11 - f01))).sum(axis=0)
        hx = (np.abs(g) * ((1 - b) * (np.abs(f01) + np.abs(f00)) + b * (np.abs(f11) + np.abs(f10)))).sum(axis=0)
        hy = (np.abs(g) * ((1 - a) * (np.abs(f10) + np.abs(f00)) + a * (np.abs(f11) + np.abs(f01)))).sum(axis=0)
        tx = (np.arange(PW) / float(PW) if fw[r] else np.zeros(PW))[None, :]
        ty = (np.arange(PH) / float(PH) if fh[r] else np.zeros(PH))[:, None]
        for out, vx, vy in ((drois, gx, gy), (dabs, hx, hy)):
            out[r, 1], out[r, 3] = s * ((1 - tx) * vx).sum(), s * (tx * vx).sum()
            out[r, 2], out[r, 4] = s * ((1 - ty) * vy).sum(), s * (ty * vy).sum()
    return np.ascontiguousarray(dfeat), drois, dabs, terms


def _pool_args(x, dout):
    x, dout = np.asarray(x, np.float32), np.asarray(dout, np.float32)
    if x.ndim != 4 or x.shape[2] % 2 or x.shape[3] % 2 or dout.shape != x.shape[:2] + (x.shape[2] // 2, x.shape[3] // 2):
        raise ValueError("maxpool2_backward: x %s (even PH, PW) and dout %s do not fit" % (x.shape, dout.shape))
    return x, dout


def maxpool2_backward_numpy(x, dout):
    """x [R,C,PH,PW] = the forward's input, dout [R,C,PH/2,PW/2] -> din [R,C,PH,PW]."""
    x, dout = _pool_args(x, dout)
    win = [x[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
    k, m = np.zeros(dout.shape, np.int8), win[0].copy()
    for i in (1, 2, 3):
        up = win[i] > m
        k[up], m[up] = i, win[i][up]
    din = np.zeros(x.shape, np.float32)
    for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        din[:, :, dy::2, dx::2] = np.where(k == i, dout, np.float32(0))
    return din


def _resize_args(dout, IH, IW):
    dout = np.asarray(dout, np.float32)
    IH, IW = int(IH), int(IW)
    if dout.ndim != 4 or dout.shape[1] != 1 or IH < 2 or IW < 2 or dout.shape[2] < 1 or dout.shape[3] < 1:
        raise ValueError("mask_resize_backward: dout %s ([R,1,OH,OW]) and input size %d x %d do not fit" % (dout.shape, IH, IW))
    return dout, IH, IW


def _resize_taps(IH, IW, OH, OW):
    """The forward's taps of every output cell in its order: (h, w, [(iy, ix, float32 weight or None for weight 1), ...])."""
    f1 = np.float32(1)
    rh, rw = np.float32(IH) / np.float32(OH), np.float32(IW) / np.float32(OW)
    for h in range(OH):
        iy = np.float32(h) * rh
        sy = int(np.floor(iy))
        fy = iy - np.float32(sy)
        for w in range(OW):
            ix = np.float32(w) * rw
            sx = int(np.floor(ix))
            fx = ix - np.float32(sx)
            if sx == IW - 1 or sy == IH - 1:
                yield h, w, [(sy, sx, None)]
            else:
                yield h, w, [(sy, sx, (f1 - fx) * (f1 - fy)), (sy, sx + 1, fx * (f1 - fy)), (sy + 1, sx, (f1 - fx) * fy),
                             (sy + 1, sx + 1, fx * fy)]


def mask_resize_backward_numpy(dout, IH, IW):
    """dout [R,1,OH,OW] -> din [R,1,IH,IW], float32 in the stated order."""
    dout, IH, IW = _resize_args(dout, IH, IW)
    din = np.zeros((dout.shape[0], 1, IH, IW), np.float32)
    for h, w, taps in _resize_taps(IH, IW, dout.shape[2], dout.shape[3]):
        for iy, ix, wgt in taps:
            din[:, 0, iy, ix] += dout[:, 0, h, w] if wgt is None else wgt * dout[:, 0, h, w]
    return din


def mask_resize_tap_counts(IH, IW, OH, OW):
    """-> int64 [IH, IW]: the number of addends of din[:, 0, iy, ix]."""
    n = np.zeros((IH, IW), np.int64)
    for _, _, taps in _resize_taps(IH, IW, OH, OW):
        for iy, ix, _ in taps:
            n[iy, ix] += 1
    return n


def _maskpool_args(feat, mask, dtop):
    feat, mask, dtop = np.asarray(feat, np.float32), np.asarray(mask, np.float32), np.asarray(dtop, np.float32)
    if feat.ndim != 4 or dtop.shape != feat.shape or mask.shape != (feat.shape[0], 1) + feat.shape[2:]:
        raise ValueError("mask_pool_backward: feat %s, mask %s and dtop %s do not fit" % (feat.shape, mask.shape, dtop.shape))
    return feat, mask, dtop


def mask_pool_backward_numpy(feat, mask, dtop):
    """feat, dtop [R,C,PH,PW], mask [R,1,PH,PW] -> (dfeat [R,C,PH,PW], dmask [R,1,PH,PW]) in float32."""
    feat, mask, dtop = _maskpool_args(feat, mask, dtop)
    return dtop * mask, (dtop * feat).sum(axis=1, keepdims=True, dtype=np.float32)


def mask_pool_backward_f64(feat, mask, dtop):
    """-> (dfeat, dmask, dmask_abs, dmask_terms int64) in float64; an addend of dmask is one product dtop * feat."""
    feat, mask, dtop = (a.astype(np.float64) for a in _maskpool_args(feat, mask, dtop))
    p = dtop * feat
    return (dtop * mask, p.sum(axis=1, keepdims=True), np.abs(p).sum(axis=1, keepdims=True),
            np.full(mask.shape, feat.shape[1], np.int64))


# ---- the device ----

_lock = threading.RLock()
_ctxs = {}                 # device -> engine context, made on first use and kept (contexts are not thread-safe: _lock)


def _device_id(device_id):
    if device_id is not None:
        return int(device_id)
    from mnc_config import cfg
    return int(cfg.get("GPU_ID", 0))


def _call(name, *args):
    try:
        _lib.call(name, *args)
    except _lib.MncError as e:
        if e.code == 1:
            raise ValueError(str(e))
        raise


class Session(object):
    """The device buffers of one call on the device's context, freed on the way out (tools/roi_backward_bench.py times the forward
    kernel through one, beside the backward ones)."""

    def __init__(self, device_id=None):
        self.device = _device_id(device_id)
        self.ptrs = []

    def __enter__(self):
        _lock.acquire()
        try:
            if self.device not in _ctxs:
                _lib.load()
                h = ctypes.c_void_p()
                _call("mnc_ctx_create", ctypes.addressof(h), self.device)
                _ctxs[self.device] = h.value
            self.h = _ctxs[self.device]
        except Exception:
            _lock.release()
            raise
        return self

    def __exit__(self, *exc):
        try:
            for p in self.ptrs:
                _lib.call("mnc_dev_free", self.h, p)
        finally:
            _lock.release()

    def empty(self, nbytes):
        p = ctypes.c_void_p()
        _call("mnc_dev_alloc", self.h, int(max(nbytes, 16)), ctypes.addressof(p))
        self.ptrs.append(p.value)
        return p.value

    def put(self, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        p = self.empty(arr.nbytes)
        if arr.nbytes:
            _call("mnc_h2d", self.h, p, _lib.ptr(arr), arr.nbytes)
        return p

    def get(self, p, shape):
        out = np.empty(shape, np.float32)
        if out.nbytes:
            _call("mnc_d2h", self.h, _lib.ptr(out), p, out.nbytes)
        return out

    def call(self, name, *args):
        _call(name, self.h, *args)


def _rhwc(a):
    return a.transpose(0, 2, 3, 1)


def _rchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def roi_warp_backward(feat, rois, PH, PW, scale, dtop, device_id=None):
    """roi_warp_backward_numpy on the GPU (mnc_roi_warp_backward): dfeat the same bytes, drois within the rounding bound.  The
    feature map goes up in the c8 layout, dtop as [R,PH,PW,C]; C must be a multiple of 8.  ValueError for what the library refuses."""
    feat, rois, PH, PW, dtop = _warp_args(feat, rois, PH, PW, dtop)
    C, H, W = feat.shape
    R = rois.shape[0]
    if C % 8:
        raise ValueError("roi_warp_backward: C = %d is not a multiple of 8" % C)
    with Session(device_id) as s:
        d_feat = s.put(feat.reshape(C // 8, 8, H, W).transpose(0, 2, 3, 1))
        d_rois, d_dtop = s.put(rois), s.put(_rhwc(dtop))
        d_dfeat, d_drois = s.empty(feat.nbytes), s.empty(rois.nbytes)
        s.call("mnc_roi_warp_backward", d_feat, C, H, W, d_rois, R, PH, PW, float(scale), d_dtop, d_dfeat, d_drois)
        dfeat = s.get(d_dfeat, (C // 8, H, W, 8))
        drois = s.get(d_drois, (R, 5))
    return np.ascontiguousarray(dfeat.transpose(0, 3, 1, 2).reshape(C, H, W)), drois


def maxpool2_backward(x, dout, device_id=None):
    """maxpool2_backward_numpy on the GPU (mnc_maxpool2_rhwc_backward): the same bytes.  C must be a multiple of 4."""
    x, dout = _pool_args(x, dout)
    R, C, PH, PW = x.shape
    with Session(device_id) as s:
        d_in, d_dout = s.put(_rhwc(x)), s.put(_rhwc(dout))
        d_din = s.empty(x.nbytes)
        s.call("mnc_maxpool2_rhwc_backward", d_in, d_dout, d_din, R, PH, PW, C)
        din = s.get(d_din, (R, PH, PW, C))
    return _rchw(din)


def mask_resize_backward(dout, IH, IW, device_id=None):
    """mask_resize_backward_numpy on the GPU (mnc_mask_resize_backward): the same bytes."""
    dout, IH, IW = _resize_args(dout, IH, IW)
    R, _, OH, OW = dout.shape
    with Session(device_id) as s:
        d_dout = s.put(dout)
        d_din = s.empty(R * IH * IW * 4)
        s.call("mnc_mask_resize_backward", d_dout, d_din, R, IH, IW, OH, OW)
        din = s.get(d_din, (R, 1, IH, IW))
    return din


def mask_pool_backward(feat, mask, dtop, device_id=None):
    """mask_pool_backward_numpy on the GPU (mnc_mask_pool_backward): dfeat the same bytes, dmask within the rounding bound.
    C must be a multiple of 4."""
    feat, mask, dtop = _maskpool_args(feat, mask, dtop)
    R, C, PH, PW = feat.shape
    with Session(device_id) as s:
        d_feat, d_mask, d_dtop = s.put(_rhwc(feat)), s.put(mask), s.put(_rhwc(dtop))
        d_dfeat, d_dmask = s.empty(feat.nbytes), s.empty(mask.nbytes)
        s.call("mnc_mask_pool_backward", d_feat, d_mask, d_dtop, d_dfeat, d_dmask, R, PH, PW, C)
        dfeat = s.get(d_dfeat, (R, PH, PW, C))
        dmask = s.get(d_dmask, (R, 1, PH, PW))
    return _rchw(dfeat), dmask


def kernel_times(fn, device_id=None):
    """fn() with the per-launch event profile of the device's context switched on (mnc_prof_enable) -> [(launch name,
    milliseconds), ...] of the launches fn() made on that context, in launch order: the kernels alone, without the copies."""
    with Session(device_id) as s:
        s.call("mnc_prof_reset")
        s.call("mnc_prof_enable", 1)
        try:
            fn()
        finally:
            s.call("mnc_prof_enable", 0)
        n = ctypes.c_int(0)
        s.call("mnc_prof_count", ctypes.addressof(n))
        out = []
        for i in range(n.value):
            name, ms = ctypes.create_string_buffer(64), ctypes.c_float(0)
            s.call("mnc_prof_get", i, ctypes.addressof(name), 64, ctypes.addressof(ms), None, None)
            out.append((name.value.decode(), float(ms.value)))
        s.call("mnc_prof_reset")
    return out
