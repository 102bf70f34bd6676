"""The visualisation tail on the GPU (include/mnc_hip.h n4, csrc/render.hip): label maps, VOC colours and the blend over the
photograph of device-resident instance records, through mnc_render_records.

    DeviceRenderer(ctx_handle)      owns the output buffers of one context; .render(...) enqueues one image's rendering on the
                                    context's stream and returns a RenderResult
    RenderResult                    .inst / .cls (int32 [H, W]), .inst_rgb / .cls_rgb / .overlay (uint8 [H, W, 3]) copied down on first
                                    access, .kept (instances painted)
    render_pred_dict(pred, ...)     the same for a host-side pred_dict of utils/vis_seg.py (the stored-results path)

There is no fallback: without the library or a GPU these raise."""
import ctypes

import numpy as np

from . import _lib
from .instances import HEAD_BYTES


class RenderResult(object):
    """One image's rendering in a DeviceRenderer's buffers, which the next render() reuses: arrays are copied on first access
    (one device-to-host copy each, synchronising the stream) and kept; a result that was never read refuses a later image's."""
    _FIELDS = {"inst": (0, np.int32, 1), "cls": (1, np.int32, 1), "inst_rgb": (2, np.uint8, 3), "cls_rgb": (3, np.uint8, 3),
               "overlay": (4, np.uint8, 3)}

    def __init__(self, renderer, H, W):
        self._r, self._gen, self.H, self.W = renderer, renderer.generation, int(H), int(W)
        self.renderer = renderer
        self._host = {}

    def _check(self):
        if self._r.generation != self._gen:
            raise RuntimeError("this rendering's device buffers have been reused by a later render() (read .inst / .cls / ... before "
                               "the next image if they must outlive it)")

    def __getattr__(self, name):
        if name.startswith("_"):                   # (an object whose __init__ has not run: no lookup through _host)
            raise AttributeError(name)
        if name == "kept":
            if "kept" not in self._host:
                self._check()
                k = np.zeros(1, np.int32)
                _lib.call("mnc_d2h", self._r.h, _lib.ptr(k), self._r.kept_ptr, 4)
                self._host["kept"] = int(k[0])
            return self._host["kept"]
        if name not in self._FIELDS:
            raise AttributeError(name)
        if name not in self._host:
            self._check()
            which, dtype, ch = self._FIELDS[name]
            out = np.zeros((self.H, self.W) if ch == 1 else (self.H, self.W, ch), dtype)
            _lib.call("mnc_d2h", self._r.h, _lib.ptr(out), self._r.out_ptr(which, self.H, self.W), out.nbytes)
            self._host[name] = out
        return self._host[name]

    def fetch(self, names=("inst", "cls", "inst_rgb", "cls_rgb", "overlay", "kept")):
        """Copy the named outputs now (so that they outlive the next render()); -> self."""
        for n in names:
            getattr(self, n)
        return self


class DeviceRenderer(object):
    def __init__(self, ctx_handle):
        self.h = ctx_handle
        self._ptr, self._cap = 0, 0
        self._img_ptr, self._img_cap = 0, 0
        self.generation = 0

    # [inst | cls | inst_rgb | cls_rgb | overlay | kept], allocated with mnc_dev_alloc directly: nothing captured holds these addresses
    def _offsets(self, H, W):
        px = H * W
        o = [0, px * 4, px * 8, px * 11, px * 14]
        kept = (px * 17 + 255) & ~255
        return o, kept, kept + 256

    def _alloc(self, nbytes):
        p = ctypes.c_void_p()
        _lib.call("mnc_dev_alloc", self.h, int(nbytes), ctypes.addressof(p))
        return p.value

    @property
    def image_ptr(self):
        """Device address of the photograph the last render(image=<array>) uploaded (0: none) -- pass it as image= to render the
        same photograph again without another upload."""
        return self._img_ptr

    def out_ptr(self, which, H, W):
        return self._ptr + self._offsets(H, W)[0][which]

    def render(self, records_ptr, counts_ptr, record_cap, num_classes, mask_size, H, W, vis_thresh=0.5, binarize_thresh=None,
               image=None, alpha=0.8):
        """Enqueue mnc_render_records for the records at (records_ptr, counts_ptr) on this context's stream.  image: uint8 BGR
        [H, W, 3] numpy array (uploaded here), a device address of one, or None (the overlay is then blended over black)."""
        if binarize_thresh is None:
            from mnc_config import cfg
            binarize_thresh = cfg.BINARIZE_THRESH
        H, W = int(H), int(W)
        offs, kept, total = self._offsets(H, W)
        if total > self._cap:
            if self._ptr:
                _lib.call("mnc_ctx_sync", self.h)
                _lib.call("mnc_dev_free", self.h, self._ptr)
                self._ptr, self._cap = 0, 0
            self._ptr, self._cap = self._alloc(total), total
        self.kept_ptr = self._ptr + kept
        d_img = None
        if isinstance(image, np.ndarray):
            if image.dtype != np.uint8 or image.shape != (H, W, 3):
                raise TypeError("render: image must be uint8 [%d, %d, 3] (got %s %r)" % (H, W, image.dtype, image.shape))
            image = np.ascontiguousarray(image)
            if image.nbytes > self._img_cap:
                if self._img_ptr:
                    _lib.call("mnc_ctx_sync", self.h)
                    _lib.call("mnc_dev_free", self.h, self._img_ptr)
                    self._img_ptr, self._img_cap = 0, 0
                self._img_ptr, self._img_cap = self._alloc(image.nbytes), image.nbytes
            _lib.call("mnc_h2d", self.h, self._img_ptr, _lib.ptr(image), image.nbytes)
            d_img = self._img_ptr
        elif image is not None:
            d_img = int(image)
        self.generation += 1
        p = self._ptr
        _lib.call("mnc_render_records", self.h, records_ptr, counts_ptr, int(record_cap), int(num_classes), int(mask_size),
                  float(vis_thresh), float(binarize_thresh), H, W, d_img, float(alpha), p + offs[0], p + offs[1], p + offs[2],
                  p + offs[3], p + offs[4], self.kept_ptr)
        return RenderResult(self, H, W)

    def release(self):
        for p in (self._ptr, self._img_ptr):
            if p and self.h:
                _lib.call("mnc_dev_free", self.h, p)
        self._ptr = self._img_ptr = 0
        self._cap = self._img_cap = 0


class _HostRenderer(object):
    """A context of its own for pred_dicts that live on the host (utils/vis_seg.py:vis_seg, tools/demo.py:_visualise)."""

    def __init__(self, device_id):
        from .engine import _Ctx
        self.ctx = _Ctx(device_id)
        self.renderer = DeviceRenderer(self.ctx.h)
        self._blk, self._blk_cap = 0, 0

    def block(self, nbytes):
        if nbytes > self._blk_cap:
            if self._blk:
                _lib.call("mnc_ctx_sync", self.ctx.h)
                _lib.call("mnc_dev_free", self.ctx.h, self._blk)
            self._blk, self._blk_cap = self.renderer._alloc(nbytes), nbytes
        return self._blk


_host_renderers = {}


def release_host_renderers():
    """Free the contexts and device buffers render_pred_dict keeps per device (they are re-created on the next call)."""
    for hr in _host_renderers.values():
        _lib.call("mnc_ctx_sync", hr.ctx.h)
        hr.renderer.release()
        if hr._blk:
            _lib.call("mnc_dev_free", hr.ctx.h, hr._blk)
        hr.ctx.close()
    _host_renderers.clear()


def render_pred_dict(img_width, img_height, pred_dict, image=None, alpha=0.8, binarize_thresh=None, device_id=None):
    """A pred_dict of utils/vis_seg.py ({'boxes': [[x1, y1, x2, y2, score]], 'masks': [S x S], 'cls_name': [class id]}, already
    cut at the visualisation threshold) -> RenderResult, through mnc_render_records: the instances become a record block with the
    boxes rounded on the host (np.round in the boxes' own precision, as _convert_pred_to_image does; the rounded values are exact
    in the record's float32) and are all kept."""
    from mnc_config import cfg
    if device_id is None:
        device_id = int(cfg.get("GPU_ID", 0))
    hr = _host_renderers.get(device_id)
    if hr is None:
        hr = _host_renderers[device_id] = _HostRenderer(device_id)
    n = len(pred_dict["boxes"])
    S = int(np.asarray(pred_dict["masks"][0]).shape[-1]) if n else int(cfg.MASK_SIZE)
    D = 6 + S * S
    rec = np.zeros((max(n, 1), D), np.float32)
    for i in range(n):
        box = np.round(pred_dict["boxes"][i])
        if not (np.abs(box[:4]) < 2 ** 24).all():
            raise ValueError("render_pred_dict: box %d out of range" % i)
        rec[i, :4] = box[:4]
        rec[i, 4] = 1.0
        rec[i, 5] = pred_dict["cls_name"][i]
        rec[i, 6:] = np.asarray(pred_dict["masks"][i], np.float32).reshape(-1)
    head = np.zeros(HEAD_BYTES // 4, np.int32)
    head[0] = n
    blk = hr.block(HEAD_BYTES + rec.nbytes)
    raw = np.concatenate((head.view(np.uint8), rec.reshape(-1).view(np.uint8)))
    _lib.call("mnc_h2d", hr.ctx.h, blk, _lib.ptr(raw), raw.nbytes)
    return hr.renderer.render(blk + HEAD_BYTES, blk, max(n, 1), 256, S, img_height, img_width, vis_thresh=0.0,
                              binarize_thresh=binarize_thresh, image=image, alpha=alpha)
