"""Geometric transforms of packed instance masks: the eight lattice isometries plus a translation (flips, the transpose, the
rotations by quarter turns) and the nearest-neighbour gather through an integer affine inverse map (resize, rotate, shear)
(include/mnc_hip.h n18, csrc/mask_warp.hip) on mnc_amd.masks.PackedMasks.

    isometry_numpy(pm, code, tx=0, ty=0)        -> PackedMasks: the CPU statement of an isometry
    warp_numpy(pm, coef, den, window)           -> PackedMasks: the CPU statement of the gather
    warp_frame(box, coef, den, window)          the loose frame of one instance under a map: part of the rule (the size bound)
    isometry_frame(box, code, tx, ty)           the image of a box under an isometry
    isometry_map(code, tx=0, ty=0)              -> (coef, den = 1): the exact inverse of an isometry as a map for warp
    resize_map(H, W, H2, W2)                    -> (coef, den): the centre-aligned nearest-neighbour resize of H x W to H2 x W2
    affine_map(M, frac_bits=16, inverse=False)  -> (coef, den = 2 ** frac_bits): a 2 x 3 float64 matrix in cv2.warpAffine's convention
    rot90_code(k, H, W)                         -> (code, tx, ty) of np.rot90 by k quarter turns in an H x W image
    translate(pm, dx, dy)                       the bounds moved on the host: no bit is touched
    isometry / warp                             the statements through mnc_mask_isometry / mnc_mask_warp (the GPU);
                                                PackedMasks.translate / .fliplr / .flipud / .transpose / .rot90 / .isometry /
                                                .resize / .warp_affine / .warp are the methods

The rules, with the conventions of mnc_amd/algebra.py: a mask is the set of its pixels in image coordinates, empty outside its
bounds; bounds may be negative or unclipped; padding bits of the input are not trusted; every result has the n5 layout -- offsets
in order without gaps, true areas, padding bits 0 -- and TIGHT bounds, (0, 0, -1, -1) and no rows for an instance without a
pixel; classes and scores carry over.

    isometry  a set pixel (x, y) goes to (x', y'):  (u, v) = (y, x) if code & 1, else (x, y);  u = -u if code & 2;  v = -v if
              code & 4;  (x', y') = (u + tx, v + ty).  In an H x W image np.fliplr is (2, W - 1, 0), np.flipud (4, 0, H - 1), .T
              (1, 0, 0), np.rot90 by 1, 2, 3 quarter turns (5, 0, W - 1), (6, W - 1, H - 1), (3, H - 1, 0).  code 0 is a
              translation, which needs no kernel: translate() is host arithmetic on the bounds.
    warp      destination pixel (x, y) inside window = (x1, y1, x2, y2), inclusive and required, is set iff source pixel (sx, sy)
              is set in the instance:  sx = (c0 x + c1 y + c2) // den,  sy = (c3 x + c4 y + c5) // den  with Python's floor
              division, coef = (c0 .. c5) and den > 0 integers.  One denominator serves both axes; resize_map, whose axes have
              2 W2 and 2 H2, brings them to 4 W2 H2 by cross-multiplying and divides the common factor out.
              The loose frame of an instance with bounds (bx1, by1, bx2, by2) is the box -- floor of the least, ceiling of the
              greatest coordinate -- of the parallelogram bx1 den <= c0 x + c1 y + c2 <= (bx2 + 1) den - 1, by1 den <= c3 x + c4 y
              + c5 <= (by2 + 1) den - 1, whose corners are solved exactly over det = c0 c4 - c1 c3, intersected with the window.

Limits (ValueError here, MNC_ERR_INVALID in C, before anything is launched): what combine refuses about a set; code outside
[0, 7]; |tx|, |ty| or a result coordinate >= 2^24; a window coordinate outside that range or an empty window; den outside
[1, 2^32]; |c0|, |c1|, |c3|, |c4| > 2^32; |c2|, |c5| > 2^60; det == 0; more than 2^27 pixels of loose-frame rows in a call.
There is no fallback: without the library or a GPU the device functions raise.  They read host arrays: a device-resident
PackedMasks (engine results) is fetched to the host first."""
import math

import numpy as np

from . import _lib
from . import algebra as AL
from .masks import MAX_COORD, PackedMasks, _device_id, _set_args

MAX_DEN = 2 ** 32
MAX_LINEAR = 2 ** 32
MAX_OFFSET = 2 ** 60


# ---- the arguments ----

def _code(who, code, tx, ty):
    code, tx, ty = int(code), int(tx), int(ty)
    if not 0 <= code <= 7:
        raise ValueError("%s: code=%d not in [0, 7]" % (who, code))
    if abs(tx) >= MAX_COORD or abs(ty) >= MAX_COORD:
        raise ValueError("%s: translation (%d, %d) leaves the coordinate range" % (who, tx, ty))
    return code, tx, ty


def _map(who, coef, den):
    coef = tuple(int(v) for v in np.asarray(coef, object).reshape(-1))
    den = int(den)
    if len(coef) != 6:
        raise ValueError("%s: coef %r is not (c0, c1, c2, c3, c4, c5)" % (who, coef))
    if not 1 <= den <= MAX_DEN:
        raise ValueError("%s: den=%d not in [1, 2^32]" % (who, den))
    if any(abs(coef[k]) > MAX_LINEAR for k in (0, 1, 3, 4)) or any(abs(coef[k]) > MAX_OFFSET for k in (2, 5)):
        raise ValueError("%s: a coefficient of %r exceeds 2^32 (c0, c1, c3, c4) or 2^60 (c2, c5)" % (who, coef))
    if coef[0] * coef[4] == coef[1] * coef[3]:
        raise ValueError("%s: the map %r is singular" % (who, coef))
    return coef, den


def _required_window(who, window):
    if window is None:
        raise ValueError("%s: a window is required" % who)
    return AL._window(who, window, 4)


# ---- the frames ----

def isometry_frame(box, code, tx, ty):
    """The image (x1, y1, x2, y2) of the box under the isometry."""
    x1, y1, x2, y2 = (int(v) for v in box)
    u1, v1, u2, v2 = (y1, x1, y2, x2) if code & 1 else (x1, y1, x2, y2)
    if code & 2:
        u1, u2 = -u2, -u1
    if code & 4:
        v1, v2 = -v2, -v1
    return (u1 + tx, v1 + ty, u2 + tx, v2 + ty)


def warp_frame(box, coef, den, window):
    """The loose frame of an instance with bounds `box` (which has rows) under the map: exact, in Python integers.  -> (x1, y1, x2,
    y2), which may be empty (x2 < x1 or y2 < y1)."""
    c0, c1, c2, c3, c4, c5 = (int(v) for v in coef)
    bx1, by1, bx2, by2 = (int(v) for v in box)
    det = c0 * c4 - c1 * c3
    sign = -1 if det < 0 else 1
    det *= sign
    xs, ys = [], []
    for p in (bx1 * den - c2, (bx2 + 1) * den - 1 - c2):
        for q in (by1 * den - c5, (by2 + 1) * den - 1 - c5):
            xs.append(sign * (c4 * p - c1 * q))
            ys.append(sign * (c0 * q - c3 * p))
    x1, x2 = min(v // det for v in xs), max(-((-v) // det) for v in xs)
    y1, y2 = min(v // det for v in ys), max(-((-v) // det) for v in ys)
    return AL._meet((x1, y1, x2, y2), tuple(int(v) for v in window))


def _check_range(who, frames):
    for f in frames:
        if AL._has(f) and not all(-MAX_COORD < v < MAX_COORD for v in f):
            raise ValueError("%s: the result %r leaves the coordinate range" % (who, f))


# ---- the statements ----

def isometry_numpy(pm, code, tx=0, ty=0):
    """The isometry as a plain loop on the host -- the specification csrc/mask_warp.hip is tested against.  -> PackedMasks.  Raises
    ValueError where mnc_mask_isometry returns MNC_ERR_INVALID for the code, the translation, the count, the range or the pixels."""
    who = "isometry_numpy"
    code, tx, ty = _code(who, code, tx, ty)
    AL._check_set(who, pm)
    frames = [isometry_frame(AL._box(pm, i), code, tx, ty) if AL._rows(pm, i) else None for i in range(len(pm))]
    _check_range(who, frames)
    AL._check_frames(who, frames)
    dense = []
    for i, f in enumerate(frames):
        if f is None:
            dense.append(None)
            continue
        m = pm.dense(i)                                      # [y, x]
        if code & 1:
            m = m.T                                          # [v = x, u = y]
        if code & 2:
            m = m[:, ::-1]                                   # u = -u: the columns in reverse
        if code & 4:
            m = m[::-1]                                      # v = -v: the rows in reverse
        dense.append(m)
    return AL._packed(frames, dense, pm.classes, pm.scores)


def warp_numpy(pm, coef, den, window):
    """The gather as a plain loop on the host -- the specification csrc/mask_warp.hip is tested against.  -> PackedMasks.  Raises
    ValueError where mnc_mask_warp returns MNC_ERR_INVALID for the map, the window, the count or the pixels."""
    who = "warp_numpy"
    coef, den = _map(who, coef, den)
    window = _required_window(who, window)
    AL._check_set(who, pm)
    frames = [warp_frame(AL._box(pm, i), coef, den, window) if AL._rows(pm, i) else None for i in range(len(pm))]
    AL._check_frames(who, frames)
    c = [np.int64(v) for v in coef]
    dense = []
    for i, f in enumerate(frames):
        if not AL._has(f):
            dense.append(None)
            continue
        bx1, by1, bx2, by2 = AL._box(pm, i)
        x = np.arange(f[0], f[2] + 1, dtype=np.int64)[None, :]
        y = np.arange(f[1], f[3] + 1, dtype=np.int64)[:, None]
        sx = (c[0] * x + c[1] * y + c[2]) // np.int64(den)   # (numpy's // on int64 is a floor, as Python's)
        sy = (c[3] * x + c[4] * y + c[5]) // np.int64(den)
        inside = (sx >= bx1) & (sx <= bx2) & (sy >= by1) & (sy <= by2)
        out = np.zeros(inside.shape, bool)
        out[inside] = pm.dense(i)[sy[inside] - by1, sx[inside] - bx1]
        dense.append(out)
    return AL._packed(frames, dense, pm.classes, pm.scores)


# ---- the helpers ----

def isometry_map(code, tx=0, ty=0):
    """-> (coef, 1): the exact inverse of isometry (code, tx, ty), so that warp(pm, *isometry_map(...), window) is isometry(pm,
    ...) inside the window."""
    code, tx, ty = _code("isometry_map", code, tx, ty)
    su, sv = (-1 if code & 2 else 1), (-1 if code & 4 else 1)
    # u = su (x' - tx), v = sv (y' - ty); the source is (v, u) for the transposing codes, else (u, v)
    fu, fv = (su, 0, -su * tx), (0, sv, -sv * ty)
    return (fv + fu if code & 1 else fu + fv), 1


def rot90_code(k, H, W):
    """-> (code, tx, ty) of np.rot90(m, k) for an H x W array m, any integer k."""
    H, W = int(H), int(W)
    return ((0, 0, 0), (5, 0, W - 1), (6, W - 1, H - 1), (3, H - 1, 0))[int(k) % 4]


def resize_map(H, W, H2, W2):
    """-> (coef, den) of the centre-aligned nearest-neighbour resize of an H x W image to H2 x W2: sx = floor((2x + 1) W / (2 W2)),
    sy = floor((2y + 1) H / (2 H2)), the two axes brought to the denominator 4 W2 H2 by cross-multiplying and the common factor
    divided out."""
    H, W, H2, W2 = int(H), int(W), int(H2), int(W2)
    if min(H, W, H2, W2) < 1:
        raise ValueError("resize_map: sizes %r are not positive" % ((H, W, H2, W2),))
    coef, den = [4 * W * H2, 0, 2 * W * H2, 0, 4 * H * W2, 2 * H * W2], 4 * W2 * H2
    g = den
    for v in coef:
        g = math.gcd(g, v)
    return tuple(v // g for v in coef), den // g


def affine_map(M, frac_bits=16, inverse=False):
    """A 2 x 3 float64 matrix in pixel-index coordinates, cv2.warpAffine's convention (destination = M (source, 1); with inverse
    M already takes the destination to the source, cv2.WARP_INVERSE_MAP) -> (coef, den = 2 ** frac_bits): the inverse taken in
    float64, quantised with np.rint, and den // 2 added to c2 and c5, which rounds half up to the nearest source pixel.  The
    floats decide only which integers come out; the rule is stated on the integers."""
    M = np.asarray(M, np.float64).reshape(2, 3)
    frac_bits = int(frac_bits)
    if not 0 <= frac_bits <= 32:
        raise ValueError("affine_map: frac_bits=%d not in [0, 32]" % frac_bits)
    if not inverse:
        A = np.linalg.inv(M[:, :2])
        M = np.concatenate((A, -A.dot(M[:, 2:])), axis=1)
    if not np.isfinite(M).all():
        raise ValueError("affine_map: the matrix is not finite")
    den = 1 << frac_bits
    c = [int(v) for v in np.rint(M.reshape(-1) * float(den))]
    c[2] += den // 2
    c[5] += den // 2
    return tuple(c), den


def translate(pm, dx, dy):
    """The instances moved by (dx, dy): host arithmetic on the bounds of the instances that have rows, the bits shared.  Nothing
    is tightened.  Raises ValueError when a coordinate leaves the range."""
    dx, dy = int(dx), int(dy)
    pm = pm.fetch()
    bounds = pm.bounds.astype(np.int64)
    rows = (bounds[:, 2] >= bounds[:, 0]) & (bounds[:, 3] >= bounds[:, 1])
    bounds[rows] += np.array([dx, dy, dx, dy], np.int64)
    if abs(dx) >= MAX_COORD or abs(dy) >= MAX_COORD or (np.abs(bounds[rows]) >= MAX_COORD).any():
        raise ValueError("translate: (%d, %d) moves a coordinate out of the range" % (dx, dy))
    return PackedMasks(bounds.astype(np.int32), pm.offsets, pm.areas, pm.classes, pm.scores, pm.bits)


# ---- the device ----

def isometry(pm, code, tx=0, ty=0, device_id=None):
    """isometry_numpy on the GPU (mnc_mask_isometry): the same PackedMasks field by field.  Invalid arguments raise ValueError,
    invalid sets _lib.MncError (MNC_ERR_INVALID), before anything is launched.  A device-resident set is fetched to the host
    first."""
    code, tx, ty = _code("isometry", code, tx, ty)
    pm = pm.fetch()
    b = pm.bounds[(pm.bounds[:, 2] >= pm.bounds[:, 0]) & (pm.bounds[:, 3] >= pm.bounds[:, 1])]
    if len(b):                                               # (every extreme of the images is one of the hull's image)
        _check_range("isometry", [isometry_frame((b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()), code, tx, ty)])
    bounds, offsets, areas, bits = AL._one_call("mnc_mask_isometry", _set_args(pm, areas=False) + (code, tx, ty), len(pm),
                                                _device_id(device_id))
    return PackedMasks(bounds, offsets, areas, pm.classes, pm.scores, bits)


def warp(pm, coef, den, window, device_id=None):
    """warp_numpy on the GPU (mnc_mask_warp): the same PackedMasks field by field.  Invalid arguments raise ValueError, invalid
    sets _lib.MncError (MNC_ERR_INVALID), before anything is launched.  A device-resident set is fetched to the host first."""
    coef, den = _map("warp", coef, den)
    window = _required_window("warp", window)
    pm = pm.fetch()
    c, win = np.array(coef, np.int64), np.array(window, np.int32)
    bounds, offsets, areas, bits = AL._one_call("mnc_mask_warp", _set_args(pm, areas=False) + (_lib.ptr(c), den, _lib.ptr(win)),
                                                len(pm), _device_id(device_id))
    return PackedMasks(bounds, offsets, areas, pm.classes, pm.scores, bits)


def timing(on):
    """mnc_mask_warp_timing: switch the event pair on or off -> the kernels' milliseconds of the last timed call (-1.0: none)."""
    return _lib.timing("mnc_mask_warp_timing", on)
