"""The picture under packed instance masks: per instance and channel the pixel count, the sums, the extremes with their positions
and the histogram of an image's values (include/mnc_hip.h n21, csrc/mask_pixels.hip) on mnc_amd.masks.PackedMasks -- what
scipy.ndimage keeps as sum, mean, variance, minimum_position, maximum_position, histogram and center_of_mass(input, labels, index),
and skimage.regionprops as intensity_mean, intensity_min, intensity_max and centroid_weighted.

    pixel_stats_numpy(pm, image)                         -> PixelStats: the CPU statement
    histogram_numpy(pm, image, bins=256, lo=0, shift=0)  -> MaskHistograms: the CPU statement
    pixel_stats / histogram                              the same through mnc_mask_pixel_stats / mnc_mask_histogram (the GPU);
                                                         PackedMasks.pixel_stats / .histogram are the methods
    quantise(a, frac_bits=16)                            a float map -> the int32 image np.rint(a * 2^frac_bits)

The rules.  Every number the device gives is an integer; the floats (mean, variance, weighted centroid, percentiles) are made on
the host from those integers by the methods of the result classes, so the numpy path and the device path share them.

    image      an integer array [H, W] or [H, W, C] (made C-contiguous), H and W in [1, 32768], H * W <= 2^26, C in [1, 32] ([H, W]
               is C = 1), of dtype uint8, uint16, int16 or int32.  An int32 image has every value in [-2^18, 2^18]: with at most
               2^26 pixels and coordinates below 2^15 every sum then fits 64 signed bits (sumsq < 2^62, sum x v < 2^59).  Float maps
               go through quantise() first; there is no floating point on the device.
    pixels     those of an instance are its set bits inside its bounds that also lie inside [0, W) x [0, H): PackedMasks.full(i, H,
               W).  Bounds may be negative, unclipped or wholly outside the image; padding bits are not trusted.
    stats      count int64 [n]; sum, sumsq, sum_xv, sum_yv int64 [n, C], x and y the pixel's image column and row; min, max int32
               [n, C]; argmin, argmax int32 [n, C, 2] as (x, y), on equal values the pixel that is lowest in (y, x) order
               (scipy.ndimage.minimum_position's choice).  An instance without a pixel has zeros and (-1, -1) positions.
    histogram  hist int64 [n, C, bins], count int64 [n].  A pixel of value v is counted in bin (v - lo) >> shift when that lies in
               [0, bins) and dropped otherwise, as np.histogram drops values outside its range.  bins in [1, 4096], shift in [0, 31],
               lo any int32, n * C * bins <= 2^24.

Refused with ValueError, by the statements and by the device functions alike (the library says MNC_ERR_INVALID): everything
mnc_mask_moments refuses about a set (n outside [0, 2048], |coordinate| >= 2^24, more than 2^26 pixels in one bound, a bound wider
or taller than 32768); an image outside the limits above; an int32 value outside the range -- found by a kernel on the device, with
nothing written: the host does not walk the image (a call that is answered on the host -- no instance, or none with a row inside
the image -- does not look at the values at all; the statements always do).  There is no fallback: without the library or a GPU the
device functions raise.  They read host arrays: a device-resident PackedMasks (engine results) is fetched to the host first."""
import collections
import math

import numpy as np

from . import _lib
from .masks import MAX_SIDE, _device_id, _set_args
from .shape import _check_set

MAX_PIXELS = 2 ** 26
MAX_CHANNELS = 32
MAX_VALUE = 2 ** 18
MAX_BINS = 4096
MAX_TABLE = 2 ** 24
DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.int16), np.dtype(np.int32))      # the library's dtype codes


def quantise(a, frac_bits=16):
    """A float map [H, W] or [H, W, C] -> the int32 image np.rint(a * 2^frac_bits), for the entries here (a mean of it is the
    map's mean times 2^frac_bits).  ValueError where a value is not finite or leaves [-2^18, 2^18] once scaled, or frac_bits is
    not in [0, 30]."""
    frac_bits = int(frac_bits)
    if not 0 <= frac_bits <= 30:
        raise ValueError("quantise: frac_bits=%d not in [0, 30]" % frac_bits)
    q = np.rint(np.asarray(a, np.float64) * float(2 ** frac_bits))
    if q.size and not (np.isfinite(q).all() and -MAX_VALUE <= q.min() and q.max() <= MAX_VALUE):
        raise ValueError("quantise: a value leaves [-2^18, 2^18] at %d fractional bits, or is not finite" % frac_bits)
    return np.ascontiguousarray(q.astype(np.int32))


def _check_image(who, image, values=True):
    """-> (the image as a C-contiguous array [H, W, C], the library's dtype code).  values: look at an int32 image's range."""
    image = np.asarray(image)
    if image.ndim not in (2, 3) or image.dtype not in DTYPES:
        raise ValueError("%s: image is not a uint8, uint16, int16 or int32 array [H, W] or [H, W, C] (shape %s, dtype %s)"
                         % (who, image.shape, image.dtype))
    H, W = image.shape[:2]
    C = image.shape[2] if image.ndim == 3 else 1
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("%s: image %d x %d not in [1, %d]" % (who, H, W, MAX_SIDE))
    if H * W > MAX_PIXELS:
        raise ValueError("%s: %d pixels (limit %d)" % (who, H * W, MAX_PIXELS))
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError("%s: C=%d not in [1, %d]" % (who, C, MAX_CHANNELS))
    if values and image.dtype == np.int32 and (int(image.min()) < -MAX_VALUE or int(image.max()) > MAX_VALUE):
        raise ValueError("%s: an int32 image value not in [%d, %d]" % (who, -MAX_VALUE, MAX_VALUE))
    return np.ascontiguousarray(image).reshape(H, W, C), DTYPES.index(image.dtype)


def _check_bins(who, n, C, bins, lo, shift):
    bins, lo, shift = int(bins), int(lo), int(shift)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError("%s: bins=%d not in [1, %d]" % (who, bins, MAX_BINS))
    if not 0 <= shift <= 31:
        raise ValueError("%s: shift=%d not in [0, 31]" % (who, shift))
    if not -2 ** 31 <= lo < 2 ** 31:
        raise ValueError("%s: lo=%d does not fit int32" % (who, lo))
    if n * C * bins > MAX_TABLE:
        raise ValueError("%s: n * C * bins = %d (limit %d)" % (who, n * C * bins, MAX_TABLE))
    return bins, lo, shift


class PixelStats(collections.namedtuple("PixelStats", "count sum sumsq sum_xv sum_yv min max argmin argmax")):
    """count int64 [n]; sum, sumsq, sum_xv, sum_yv int64 [n, C]; min, max int32 [n, C]; argmin, argmax int32 [n, C, 2] = (x, y)."""
    __slots__ = ()

    def _ratio(self, num, den):
        out = np.full(np.shape(num), np.nan)
        for idx in np.ndindex(*np.shape(num)):
            d = int(den[idx])
            if d:
                out[idx] = int(num[idx]) / d
        return out

    def mean(self):
        """float64 [n, C]: sum / count; NaN for an instance without a pixel."""
        return self._ratio(self.sum, np.broadcast_to(self.count[:, None], self.sum.shape))

    def var(self, ddof=0):
        """float64 [n, C]: (count sumsq - sum^2) / (count (count - ddof)), the numerator in Python integers (count * sumsq does not
        fit int64) before the one division; NaN where count - ddof < 1."""
        out = np.full(self.sum.shape, np.nan)
        ddof = int(ddof)
        for i, c in np.ndindex(*self.sum.shape):
            k = int(self.count[i])
            if k - ddof >= 1:
                s = int(self.sum[i, c])
                out[i, c] = (k * int(self.sumsq[i, c]) - s * s) / (k * (k - ddof))
        return out

    def std(self, ddof=0):
        """float64 [n, C]: sqrt(var(ddof))."""
        return np.sqrt(self.var(ddof))

    def weighted_centroid(self):
        """float64 [n, C, 2]: (sum_xv / sum, sum_yv / sum), the centre of mass of the values in image coordinates of pixel indices
        (scipy.ndimage.center_of_mass, as (x, y)); NaN where sum == 0."""
        return np.stack([self._ratio(self.sum_xv, self.sum), self._ratio(self.sum_yv, self.sum)], axis=-1)


class MaskHistograms(collections.namedtuple("MaskHistograms", "hist count lo shift bins")):
    """hist int64 [n, C, bins], count int64 [n]; bin k holds the values lo + (k << shift) .. lo + ((k + 1) << shift) - 1."""
    __slots__ = ()

    def edge(self, k):
        """The lower edge of bin k (an array of bins gives an array)."""
        return self.lo + (np.asarray(k, np.int64) << self.shift)

    def percentile(self, q):
        """int64 [n, C]: the lower edge of the first bin whose cumulative count reaches ceil(q / 100 * total), at least 1; total is
        what the histogram counted.  A histogram that counted nothing gives edge(bins)."""
        total = self.hist.sum(-1)
        cum = np.cumsum(self.hist, axis=-1)
        out = np.zeros(total.shape, np.int64)
        for idx in np.ndindex(*total.shape):
            need = max(int(math.ceil(float(q) * int(total[idx]) / 100.0)), 1)
            out[idx] = self.edge(int(np.searchsorted(cum[idx], need, side="left")))
        return out

    def median(self):
        return self.percentile(50)

    def mode(self):
        """int64 [n, C]: the lower edge of the fullest bin, the lowest on ties."""
        return self.edge(np.argmax(self.hist, axis=-1))


def _pixels_of(pm, i, H, W):
    """The pixels of instance i inside the image in raster order -> (y, x)."""
    return np.nonzero(pm.full(i, H, W))


# ---- the statements ----

def pixel_stats_numpy(pm, image):
    """The figures as a plain loop on the host -- the specification csrc/mask_pixels.hip is tested against.  -> PixelStats."""
    _check_set("pixel_stats_numpy", pm)
    image, _ = _check_image("pixel_stats_numpy", image)
    H, W, C = image.shape
    n = len(pm)
    count = np.zeros(n, np.int64)
    sums = [np.zeros((n, C), np.int64) for _ in range(4)]
    lo, hi = np.zeros((n, C), np.int32), np.zeros((n, C), np.int32)
    at_lo, at_hi = np.full((n, C, 2), -1, np.int32), np.full((n, C, 2), -1, np.int32)
    for i in range(n):
        y, x = _pixels_of(pm, i, H, W)
        if not y.size:
            continue
        v = image[y, x].astype(np.int64)                                     # [count, C], raster order
        count[i] = y.size
        sums[0][i], sums[1][i] = v.sum(0), (v * v).sum(0)
        sums[2][i], sums[3][i] = (v * x[:, None]).sum(0), (v * y[:, None]).sum(0)
        k_lo, k_hi = v.argmin(0), v.argmax(0)                                # (the first in raster order)
        lo[i], hi[i] = v.min(0), v.max(0)
        at_lo[i], at_hi[i] = np.stack([x[k_lo], y[k_lo]], 1), np.stack([x[k_hi], y[k_hi]], 1)
    return PixelStats(count, sums[0], sums[1], sums[2], sums[3], lo, hi, at_lo, at_hi)


def histogram_numpy(pm, image, bins=256, lo=0, shift=0):
    """The histograms as a plain loop on the host -- the specification csrc/mask_pixels.hip is tested against.
    -> MaskHistograms."""
    _check_set("histogram_numpy", pm)
    image, _ = _check_image("histogram_numpy", image)
    H, W, C = image.shape
    n = len(pm)
    bins, lo, shift = _check_bins("histogram_numpy", n, C, bins, lo, shift)
    hist, count = np.zeros((n, C, bins), np.int64), np.zeros(n, np.int64)
    for i in range(n):
        y, x = _pixels_of(pm, i, H, W)
        count[i] = y.size
        d = image[y, x].astype(np.int64) - lo
        b = d >> shift
        for c in range(C):
            keep = (d[:, c] >= 0) & (b[:, c] < bins)
            hist[i, c] = np.bincount(b[keep, c], minlength=bins)
    return MaskHistograms(hist, count, lo, shift, bins)


# ---- the device ----

def _call(name, *args):
    """An entry whose MNC_ERR_INVALID is this module's ValueError: the library checks the set (a Python loop over the bounds would
    cost more than the call) and finds the int32 range on the device."""
    try:
        _lib.call(name, *args)
    except _lib.MncError as e:
        if e.code == 1:
            raise ValueError(str(e))
        raise


def pixel_stats(pm, image, device_id=None):
    """pixel_stats_numpy on the GPU (mnc_mask_pixel_stats): the same PixelStats field by field; the image goes up once, in its own
    dtype, and 1 + 10 C numbers per instance come back.  ValueError for what the statement refuses.  A device-resident PackedMasks
    is fetched first."""
    pm = pm.fetch()
    image, dtype = _check_image("pixel_stats", image, values=False)
    n, C = len(pm), image.shape[2]
    count, sums, ext = np.zeros(n, np.int64), np.zeros((n, C, 4), np.int64), np.zeros((n, C, 6), np.int32)
    if n:
        _call("mnc_mask_pixel_stats", *(_set_args(pm, areas=False) + (
            _lib.ptr(image), dtype, image.shape[0], image.shape[1], C, _lib.ptr(count), _lib.ptr(sums), _lib.ptr(ext),
            _device_id(device_id))))
    part = lambda a: np.ascontiguousarray(a)                                  # noqa: E731
    return PixelStats(count, part(sums[:, :, 0]), part(sums[:, :, 1]), part(sums[:, :, 2]), part(sums[:, :, 3]), part(ext[:, :, 0]),
                      part(ext[:, :, 3]), part(ext[:, :, 1:3]), part(ext[:, :, 4:6]))


def histogram(pm, image, bins=256, lo=0, shift=0, device_id=None):
    """histogram_numpy on the GPU (mnc_mask_histogram): the same MaskHistograms field by field.  ValueError for what the statement
    refuses.  A device-resident PackedMasks is fetched first."""
    pm = pm.fetch()
    image, dtype = _check_image("histogram", image, values=False)
    n, C = len(pm), image.shape[2]
    bins, lo, shift = _check_bins("histogram", n, C, bins, lo, shift)
    count, hist = np.zeros(n, np.int64), np.zeros((n, C, bins), np.int64)
    if n:
        _call("mnc_mask_histogram", *(_set_args(pm, areas=False) + (
            _lib.ptr(image), dtype, image.shape[0], image.shape[1], C, lo, shift, bins, _lib.ptr(count), _lib.ptr(hist),
            _device_id(device_id))))
    return MaskHistograms(hist, count, lo, shift, bins)


def timing(on):
    """mnc_mask_pixels_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_pixels_timing", on)
