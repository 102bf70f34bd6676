"""Per-instance binary masks at image resolution, one bit per pixel (include/mnc_hip.h n5, csrc/inst_masks.hip): what every
consumer of a voted instance makes first -- round the box, resize the S x S mask to it with cv2's INTER_LINEAR rule, binarise.

    PackedMasks                     the masks of one image: .bounds int32 [n, 4] (x1, y1, x2, y2 of the rounded box), .offsets
                                    int64 [n] (bytes into .bits), .areas int64 [n] (set pixels), .classes int32 [n], .scores
                                    float32 [n], .bits uint64 [...]; .dense(i), .full(i, H, W), .as_sds_gt(i)
    instance_masks(...)             host arrays -> PackedMasks through mnc_instance_masks (the GPU)
    instance_masks_numpy(...)       the same object from the plain utils.blob.resize_to loop: the CPU statement of the rule
    records_masks(...)              device-resident instance records -> PackedMasks through mnc_mask_records, copied on first access
    mask_overlaps(a, b=None)        (inter int64 [na, nb], iou float64 [na, nb]) of every pair of two sets: the reference's
                                    mask_overlap on the packed words (include/mnc_hip.h n6, csrc/mask_overlaps.hip)
    mask_nms(pm, thresh)            greedy suppression by mask IoU in score order -> kept indices int32
    mask_overlaps_numpy / mask_nms_numpy   the CPU statements of both; PackedMasks.overlaps / .nms / .take the methods
    PackedMasks.rle_counts / .rle / .from_rle   COCO run-length encoding of the masks and the way back (mnc_amd/rle.py, n7)
    PackedMasks.from_polygons / .from_segmentations   COCO polygon segmentations rasterised into the layout (mnc_amd/polygons.py, n9)
    PackedMasks.match(gt, iscrowd)  COCO's matching of detections to ground truths (mnc_amd/coco_eval.py, n8)
    PackedMasks.boundary / .match_boundary   the boundary bands and the matching on min(mask IoU, boundary IoU) (mnc_amd/boundary.py, n11)
    PackedMasks.components / .select / .fill_holes / .split   connected components and what is built on them (mnc_amd/components.py, n12)
    PackedMasks.contours / .polygons   the outlines as closed loops of lattice points, and as COCO polygons (mnc_amd/contours.py, n13),
                                       simplified to a tolerance with polygons(epsilon=) (n14)
    PackedMasks.distance / .inscribed / .erode / .dilate / .open / .close   the squared Euclidean distance transform, the deepest
                                       pixel of every instance, and the morphology by a disc (mnc_amd/distance.py, n15)
    PackedMasks.moments / .hull / .solidity / .oriented_boxes   the moments of order up to two, the convex hull, the rectangle of
                                       least area and the diameter (mnc_amd/shape.py, n16)
    PackedMasks.combine / & | ^ - / .tighten / .crop / .complement / .merge / .layered   the set algebra: two sets instance by
                                       instance, groups united or intersected, a set made disjoint (mnc_amd/algebra.py, n17)
    PackedMasks.translate / .fliplr / .flipud / .transpose / .rot90 / .isometry / .resize / .warp_affine / .warp   the geometric
                                       transforms: flips, quarter turns, and nearest-neighbour affine maps (mnc_amd/warp.py, n18)
    PackedMasks.from_labels / .to_labels   the instances of an integer label map as a set, and the label map of a set
                                       (mnc_amd/labels.py, n19)
    PackedMasks.pixel_stats / .histogram   what an image holds under every instance: count, sums, extremes with their positions,
                                       and the histogram of the values (mnc_amd/pixels.py, n21)
    PackedMasks.surface / .surface_stats / .surface_distances   the surfaces, and the distances between the surfaces of pairs of
                                       instances of two sets: Hausdorff, HD95, ASSD, boundary F (mnc_amd/surface.py, n22)
    PackedMasks.targets(ex_boxes, gt_index)   the S x S mask regression targets of boxes against these ground-truth masks: the
                                       reference's intersect_mask for all rows at once (mnc_amd/targets.py, n23)
    PackedMasks.pred_overlaps(boxes, preds, gt_index)   the overlap of predicted S x S masks, resized to their boxes, with these
                                       ground-truth masks: what MaskLayer's TRAIN phase counts (mnc_amd/targets.py, n23)

Bit layout: instance i is h rows of ceil(w / 64) little-endian 64-bit words at byte offsets[i]; bit dx % 64 of word dx / 64 is
pixel dx, padding bits are 0 -- utils.voc_eval.pack_sds_gt's bit order with the row stride rounded up to 8 bytes.  There is no
fallback: without the library or a GPU the device functions raise."""
import ctypes

import numpy as np

from . import _lib

HEAD_BYTES = 256
# mnc_mask_head / mnc_mask_info of include/mnc_hip.h
HEAD = np.dtype({"names": ["kept", "bits_bytes"], "formats": ["<i4", "<i8"], "offsets": [0, 8], "itemsize": HEAD_BYTES})
INFO = np.dtype({"names": ["bounds", "cls", "score", "row", "offset", "area"],
                 "formats": [("<i4", 4), "<i4", "<f4", "<i4", "<i8", "<i8"], "offsets": [0, 16, 20, 24, 32, 40], "itemsize": 64})
MAX_MASK = 32
MAX_COORD = 2 ** 24
MAX_AREA = 2 ** 26
MAX_SIDE = 32768


def row_words(h, w):
    """The uint64 words of one instance of h rows and w columns; 0 when either side is 0."""
    return h * ((w + 63) // 64) if h and w else 0


def pack_rows(m):
    """bool [h, w] -> the uint64 words of its rows: the bit layout above, padding bits 0."""
    h, w = m.shape
    rows = np.zeros((h, (w + 63) // 64 * 8), np.uint8)
    rows[:, :(w + 7) // 8] = np.packbits(m, axis=1, bitorder="little")
    return rows.reshape(-1).view(np.uint64)


def merge_sets(parts, order):
    """Host PackedMasks `parts` and for every output row the (part, row) it comes from -> (bounds, offsets, areas, bits) of one set
    in that order: the offsets repacked without gaps, the bits copied.  The one gather: PackedMasks.take is it over one set."""
    words, at = [], 0
    bounds, offsets, areas = np.zeros((len(order), 4), np.int32), np.zeros(len(order), np.int64), np.zeros(len(order), np.int64)
    for k, (p, i) in enumerate(order):
        pm = parts[p]
        count = row_words(*pm.size(i))
        lo = int(pm.offsets[i]) // 8
        words.append(pm.bits[lo:lo + count])
        bounds[k], offsets[k], areas[k] = pm.bounds[i], at, pm.areas[i]
        at += count * 8
    return bounds, offsets, areas, (np.concatenate(words) if words else np.zeros(0, np.uint64))


def sized_then_filled(call):
    """The two calls of an entry point that reports the bytes of its bits: call(None) for the size, then call(bits) with room.
    call(bits_or_None) -> (bounds, offsets, areas, need); -> (bounds, offsets, areas, bits) with bits.size == need // 8.  A result
    of zero bytes makes the second call with a one-word buffer that is not returned: every entry point takes a non-null pointer
    as "the call with room" and none writes past `need`, whereas null would ask for the sizes again and an empty array's address
    is whatever numpy makes it."""
    need = call(None)[3]
    bits = np.zeros(need // 8, np.uint64)
    bounds, offsets, areas, _ = call(bits if bits.size else np.zeros(1, np.uint64))
    return bounds, offsets, areas, bits


class PackedMasks(object):
    """The packed masks of one image.  Made from host arrays, or from a device result whose arrays are copied on first access
    (the instance table in one copy, the bits in a second) and kept; a device result that was never read refuses a later image's."""
    FIELDS = ("bounds", "offsets", "areas", "classes", "scores", "bits")

    def __init__(self, bounds=None, offsets=None, areas=None, classes=None, scores=None, bits=None, source=None):
        self._host = {}
        self._source = source
        if source is None:
            n = len(bounds)
            self._host = {"bounds": np.ascontiguousarray(bounds, np.int32).reshape(n, 4),
                          "offsets": np.ascontiguousarray(offsets, np.int64).reshape(n),
                          "areas": np.ascontiguousarray(areas, np.int64).reshape(n),
                          "classes": np.ascontiguousarray(np.zeros(n) if classes is None else classes, np.int32).reshape(n),
                          "scores": np.ascontiguousarray(np.zeros(n) if scores is None else scores, np.float32).reshape(n),
                          "bits": np.ascontiguousarray(bits, np.uint64).reshape(-1)}

    def __getattr__(self, name):
        if name.startswith("_") or name not in self.FIELDS:       # (also an object whose __init__ has not run)
            raise AttributeError(name)
        if name not in self._host:
            self._source.load(self._host, name == "bits")
        return self._host[name]

    def fetch(self):
        """Copy everything now (so that it outlives the next image's masks); -> self."""
        for name in self.FIELDS:
            getattr(self, name)
        return self

    def __len__(self):
        return len(self.bounds)

    def size(self, i):
        """-> (h, w) of instance i."""
        x1, y1, x2, y2 = (int(v) for v in self.bounds[i])
        return max(y2 - y1 + 1, 0), max(x2 - x1 + 1, 0)

    def _rows(self, i):
        h, w = self.size(i)
        if h == 0 or w == 0:
            return np.zeros((h, 0), np.uint8), w
        lo = int(self.offsets[i]) // 8
        return self.bits[lo:lo + row_words(h, w)].view(np.uint8).reshape(h, row_words(1, w) * 8), w

    def dense(self, i):
        """bool [h, w]: the mask of instance i inside its bounds."""
        rows, w = self._rows(i)
        return np.unpackbits(rows, axis=1, bitorder="little")[:, :w].astype(bool)

    def full(self, i, H, W):
        """bool [H, W]: instance i in the image (what of it lies inside, when the bounds were not clipped)."""
        out = np.zeros((int(H), int(W)), bool)
        x1, y1, x2, y2 = (int(v) for v in self.bounds[i])
        ax, ay, bx, by = max(x1, 0), max(y1, 0), min(x2, W - 1), min(y2, H - 1)
        if ax <= bx and ay <= by:
            out[ay:by + 1, ax:bx + 1] = self.dense(i)[ay - y1:by - y1 + 1, ax - x1:bx - x1 + 1]
        return out

    def as_sds_gt(self, i):
        """uint8 [h, ceil(w / 8)]: the rows utils.voc_eval.pack_sds_gt makes of this mask (np.packbits(axis=1, bitorder='little')):
        the leading bytes of the packed rows."""
        rows, w = self._rows(i)
        return np.ascontiguousarray(rows[:, :(w + 7) // 8])

    def _device(self):
        """The device result behind this object when its buffers are still the context's current ones, else None (a stale one
        whose arrays were not all copied raises what load raises)."""
        src = self._source
        if src is None:
            return None
        if src.is_current():
            return src
        if all(name in self._host for name in self.FIELDS):
            return None
        src.check()

    def overlaps(self, other=None):
        """(inter int64 [n, m], iou float64 [n, m]) against `other` (a PackedMasks in the same image frame; None: against itself)
        by the rule of mask_overlaps_numpy.  A device-resident result is compared where it lies (mnc_mask_overlaps_dev: its bits
        are not copied to the host, only the matrices come back); anything else goes through mnc_mask_overlaps."""
        dev = self._device()
        if dev is None:
            return mask_overlaps(self, other)
        return dev.overlaps(len(self), None if other is None or other is self else other)

    def nms(self, thresh, class_aware=False):
        """Kept indices int32, in score order, of the greedy mask NMS (mask_nms_numpy's rule) on the GPU; a device-resident
        result through mnc_mask_nms_dev (only the kept list comes back), anything else through mnc_mask_nms."""
        dev = self._device()
        if dev is None:
            return mask_nms(self, thresh, class_aware)
        return dev.nms(thresh, class_aware)

    def match(self, gt, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, return_iou=False,
              device_id=None):
        """COCO's matching of these detections to the ground truths `gt` (a PackedMasks with classes, in the same image frame) by
        the rule of mnc_amd.coco_eval.match_numpy (include/mnc_hip.h n8, csrc/mask_match.hip) on the GPU -> coco_eval.Match.  A
        device-resident result is matched where it lies (mnc_mask_match_dev: only the tables come back); anything else goes
        through mnc_mask_match on GPU device_id (None: cfg.GPU_ID)."""
        from . import coco_eval
        dev = self._device()
        if dev is None:
            return coco_eval.match(self, gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, return_iou, device_id)
        return coco_eval.device_match(dev, len(self), gt, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, return_iou)

    def boundary(self, H, W, d=None, ratio=0.02, device_id=None):
        """The boundary bands of these masks in an H x W image at distance d (None: mnc_amd.boundary.boundary_distance(H, W, ratio))
        -> a host PackedMasks in the same layout, by the rule of mnc_amd.boundary.boundary_numpy (include/mnc_hip.h n11,
        csrc/mask_boundary.hip) on the GPU.  A device-resident result is fetched to the host first."""
        from . import boundary
        return boundary.boundary(self, H, W, d, ratio, device_id)

    def match_boundary(self, gt, H, W, iscrowd=None, ignore=None, eval_area=None, iou_thrs=None, area_rngs=None, max_det=100, d=None,
                       ratio=0.02, return_iou=False, device_id=None):
        """match() on the overlap min(mask IoU, boundary IoU) in an H x W image (COCO's iouType "boundary"), by the rule of
        mnc_amd.coco_eval.match_boundary_numpy through mnc_mask_match_boundary -> coco_eval.Match, with return_iou (Match, biou).
        There is no form that matches a device-resident result where it lies: such a result is fetched to the host first (the
        instance table and the bits, two copies), then uploaded with the call."""
        from . import coco_eval
        return coco_eval.match_boundary(self, gt, H, W, iscrowd, ignore, eval_area, iou_thrs, area_rngs, max_det, d, ratio, return_iou,
                                        device_id)

    def components(self, connectivity=8, device_id=None):
        """The connected components of every instance under 4- or 8-connectivity -> mnc_amd.components.Components(comp_ptr, area,
        bbox, anchor), numbered by first pixel in row-major order, by the rule of mnc_amd.components.components_numpy
        (include/mnc_hip.h n12, csrc/mask_components.hip) on the GPU.  A device-resident result is fetched to the host first."""
        from . import components
        return components.components(self, connectivity, device_id)

    def select(self, connectivity=8, min_area=1, keep=0, device_id=None):
        """The components of area >= min_area and, with keep > 0, among the `keep` largest of their instance -> a host PackedMasks
        with this one's bounds and offsets (mnc_amd.components.select_numpy's rule through mnc_mask_select).  A device-resident
        result is fetched to the host first."""
        from . import components
        return components.select(self, connectivity, min_area, keep, device_id)

    def fill_holes(self, connectivity=4, device_id=None):
        """These masks OR their holes, `connectivity` being the background's -> a host PackedMasks with this one's bounds and
        offsets (mnc_amd.components.fill_holes_numpy's rule through mnc_mask_fill_holes).  A device-resident result is fetched to
        the host first."""
        from . import components
        return components.fill_holes(self, connectivity, device_id)

    def split(self, connectivity=8, device_id=None):
        """One instance per connected component, tight bounds, in component order -> (a host PackedMasks, source int32 [C])
        (mnc_amd.components.split_numpy's rule through mnc_mask_split).  A device-resident result is fetched to the host first."""
        from . import components
        return components.split(self, connectivity, device_id)

    def contours(self, connectivity=8, device_id=None):
        """The outline of every instance as closed rectilinear loops on lattice points, outer loops clockwise on screen and holes
        the other way -> mnc_amd.contours.Contours(loop_ptr, vert_ptr, area, xy), by the rule of mnc_amd.contours.contours_numpy
        (include/mnc_hip.h n13, csrc/mask_contours.hip) on the GPU.  A device-resident result is fetched to the host first."""
        from . import contours
        return contours.contours(self, connectivity, device_id)

    def polygons(self, connectivity=8, device_id=None, epsilon=0.0):
        """One COCO `segmentation` per instance: the outer loops of contours(connectivity) as flat [x0, y0, x1, y1, ...] float
        lists, the holes dropped.  COCO's polygons of one annotation are OR-ed, so they cannot say a hole: for masks inside the
        H x W image, from_polygons(pm.polygons(c), H, W) is pm.fill_holes(4 if c == 8 else 8) -- the holes of the background of the
        complementary connectivity filled -- with tight bounds.  Contours.polygons(i, holes=True) keeps the holes for a reader that
        XORs.  epsilon > 0: the loops simplified to that many pixels on the GPU (Contours.simplify, include/mnc_hip.h n14: what
        cv2.approxPolyDP does after findContours); epsilon == 0, the default, is the exact pixel staircase."""
        from . import contours
        return contours.polygons(self, connectivity, device_id, epsilon)

    def distance(self, device_id=None):
        """The squared Euclidean inside distance of every pixel -> mnc_amd.distance.DistanceMaps(dist_ptr, sq, shapes), .map(i) the
        uint32 [h, w] of instance i, by the rule of mnc_amd.distance.distance_numpy (include/mnc_hip.h n15, csrc/mask_distance.hip)
        on the GPU.  A device-resident result is fetched to the host first."""
        from . import distance
        return distance.distance(self, device_id)

    def inscribed(self, device_id=None):
        """The centre of the largest inscribed disc of every instance -> (xy int32 [n, 2] in image coordinates, r2 int32 [n] its
        squared radius): the pixel of maximal inside distance, the lowest (y, x) on ties; (-1, -1) and 0 for an instance without
        a set pixel (mnc_amd.distance.inscribed_numpy's rule through mnc_mask_inscribed).  A device-resident result is fetched to
        the host first."""
        from . import distance
        return distance.inscribed(self, device_id)

    def erode(self, radius=None, r2=None, device_id=None):
        """These masks eroded by the disc {dx^2 + dy^2 <= r2} (r2 exact, or radius: mnc_amd.distance.radius_sq) -> a host
        PackedMasks with this one's bounds, by the rule of mnc_amd.distance.morph_numpy through mnc_mask_morph.  A device-resident
        result is fetched to the host first."""
        from . import distance
        return distance.morph(self, "erode", radius, r2, None, None, device_id)

    def dilate(self, radius=None, r2=None, H=None, W=None, device_id=None):
        """These masks dilated by the disc -> a host PackedMasks whose bounds are this one's grown by isqrt(r2) on every side, with
        H, W intersected with the image (morph_numpy's rule).  A device-resident result is fetched to the host first."""
        from . import distance
        return distance.morph(self, "dilate", radius, r2, H, W, device_id)

    def open(self, radius=None, r2=None, device_id=None):
        """dilate(erode) by the disc, without leaving the device in between: spurs, necks and specks narrower than the disc go ->
        a host PackedMasks with this one's bounds (morph_numpy's rule).  A device-resident result is fetched to the host first."""
        from . import distance
        return distance.morph(self, "open", radius, r2, None, None, device_id)

    def close(self, radius=None, r2=None, device_id=None):
        """erode(dilate) by the disc, the erosion taken in the unclipped grown frame: notches, pinholes and gaps narrower than the
        disc fill -> a host PackedMasks with this one's bounds (morph_numpy's rule).  A device-resident result is fetched to the
        host first."""
        from . import distance
        return distance.morph(self, "close", radius, r2, None, None, device_id)

    def moments(self, device_id=None):
        """The moments of order up to two of every instance -> mnc_amd.shape.Moments(m int64 [n, 6], origin): (m00, m10, m01, m20,
        m11, m02) relative to the bounds' corner, with .centroid(), .central(), .orientation() and .axes() on the host, by the
        rule of mnc_amd.shape.moments_numpy (include/mnc_hip.h n16, csrc/mask_shape.hip) on the GPU.  A device-resident result
        is fetched to the host first."""
        from . import shape
        return shape.moments(self, device_id)

    def hull(self, device_id=None):
        """The convex hull of every instance's pixel squares -> mnc_amd.shape.Hulls(vert_ptr, xy, area2): lattice vertices in
        image coordinates, clockwise on screen from the smallest (y, x), and twice the area, by the rule of
        mnc_amd.shape.hull_numpy through mnc_mask_hull.  A device-resident result is fetched to the host first."""
        from . import shape
        return shape.hull(self, device_id)

    def solidity(self, device_id=None):
        """float64 [n]: .areas over the hull's area, 2 area / area2; 0 for an instance without a set pixel.  A device-resident
        result is fetched to the host first."""
        from . import shape
        return shape.hull(self, device_id).solidity(self.areas)

    def oriented_boxes(self, device_id=None):
        """The rectangle of least area around every instance and its diameter -> mnc_amd.shape.OrientedBoxes(box int64 [n, 8],
        diameter int64 [n, 3]) with .corners() and .rbox() on the host, by the rule of mnc_amd.shape.oriented_numpy through
        mnc_mask_oriented (hull and calipers in one call).  A device-resident result is fetched to the host first."""
        from . import shape
        return shape.oriented(self, device_id)

    def pixel_stats(self, image, device_id=None):
        """What an integer image [H, W] or [H, W, C] (uint8, uint16, int16, or int32 within +-2^18) holds under every instance ->
        mnc_amd.pixels.PixelStats(count, sum, sumsq, sum_xv, sum_yv, min, max, argmin, argmax) per instance and channel, with
        .mean(), .var(), .std() and .weighted_centroid() on the host, by the rule of mnc_amd.pixels.pixel_stats_numpy
        (include/mnc_hip.h n21, csrc/mask_pixels.hip) on the GPU.  A device-resident result is fetched to the host first."""
        from . import pixels
        return pixels.pixel_stats(self, image, device_id)

    def histogram(self, image, bins=256, lo=0, shift=0, device_id=None):
        """The histogram of such an image's values under every instance, bin (v - lo) >> shift -> mnc_amd.pixels.MaskHistograms(hist
        int64 [n, C, bins], count, lo, shift, bins) with .percentile(q), .median() and .mode() on the host, by the rule of
        mnc_amd.pixels.histogram_numpy through mnc_mask_histogram.  A device-resident result is fetched to the host first."""
        from . import pixels
        return pixels.histogram(self, image, bins, lo, shift, device_id)

    def surface(self, device_id=None):
        """The surfaces of these masks -- the pixels with one of their four edge neighbours outside the mask, M & ~erode(M, r2=1)
        -- as a host PackedMasks in this one's frames: its bounds, areas the surface pixel counts, classes and scores carried
        over, by the rule of mnc_amd.surface.surface_numpy (include/mnc_hip.h n22, csrc/mask_surface.hip) on the GPU.  A
        device-resident result is fetched to the host first."""
        from . import surface
        return surface.surface(self, device_id)

    def surface_stats(self, other, pairs=None, tau2=(), device_id=None):
        """The squared distances from the surface pixels of instance i of these masks to the surface of instance j of `other` and
        back, reduced, for the pairs (i, j) of `pairs` (int [P, 2]; None: all pairs in row-major order) -> mnc_amd.surface.
        SurfaceStats(count, max_d2, argmax, sum_d2, within, tau2), every field [P, 2] over the two directions, with .hausdorff(),
        .precision(t), .recall(t), .boundary_f(t) and .nsd(t) on the host, by the rule of mnc_amd.surface.surface_stats_numpy
        through mnc_mask_surface_stats.  tau2: up to 8 squared tolerances (surface.tolerance_sq gives DAVIS's).  Device-resident
        results are fetched to the host first."""
        from . import surface
        return surface.surface_stats(self, other, pairs, tau2, device_id)

    def surface_distances(self, other, pairs=None, device_id=None):
        """Those squared distances themselves -> mnc_amd.surface.SurfaceDistances(ptr, d2): pair k in direction d owns d2[ptr[2 k +
        d]:ptr[2 k + d + 1]], in raster order of the source's surface, with .slot(k, d), .percentile(q), .hd95() and .assd() on the
        host, by the rule of mnc_amd.surface.surface_distances_numpy through mnc_mask_surface_dist.  Device-resident results are
        fetched to the host first."""
        from . import surface
        return surface.surface_distances(self, other, pairs, device_id)

    def targets(self, ex_boxes, gt_index, S=None, thresh=None, device_id=None):
        """The mask regression targets of the boxes ex_boxes int [K, 4] (x1, y1, x2, y2 inclusive) against these ground-truth
        masks, row k against instance gt_index[k] -> uint8 [K, S, S] of 0 / 1: the ground truth pasted on a canvas of the box's
        size, resized to S x S (None: cfg.MASK_SIZE) by cv2's rule and binarised with >= float32(thresh) (None:
        cfg.BINARIZE_THRESH), zeros where box and bounds do not meet -- the reference's intersect_mask, by the rule of
        mnc_amd.targets.mask_targets_numpy (include/mnc_hip.h n23, csrc/mask_targets.hip) on the GPU.  A device-resident result is
        fetched to the host first."""
        from . import targets
        return targets.mask_targets(self, ex_boxes, gt_index, S, thresh, device_id)

    def pred_overlaps(self, boxes, preds, gt_index, thresh=None, device_id=None):
        """The overlap of the predictions preds float32 [K, S, S], each resized to its box of boxes float64 [K, 4] (rounded half to
        even, not clipped) and binarised, with instance gt_index[k] of these ground-truth masks (-1: a background row, zeros) ->
        (inter int64 [K], area_pred int64 [K], iou float64 [K]), by the rule of mnc_amd.targets.mask_pred_overlaps_numpy through
        mnc_mask_pred_overlaps: no mask bit leaves the device.  A device-resident result is fetched to the host first."""
        from . import targets
        return targets.mask_pred_overlaps(self, boxes, preds, gt_index, thresh, device_id)

    def combine(self, other, op, window=None, device_id=None):
        """These masks combined with `other` instance by instance (len(other) == len(self), or 1: that instance against every
        one) -> a host PackedMasks with tight bounds and this one's classes and scores.  op "and", "or", "xor", "minus" (self &
        ~other), "copy" or "not" (other is not looked at: this set tightened or cropped, resp. its complement inside the
        window, which "not" requires); window (x1, y1, x2, y2), inclusive, cuts the result.  By the rule of
        mnc_amd.algebra.combine_numpy (include/mnc_hip.h n17, csrc/mask_algebra.hip) on the GPU.  Device-resident results are
        fetched to the host first."""
        from . import algebra
        return algebra.combine(self, other, op, window, device_id)

    def __and__(self, other):
        return self.combine(other, "and")

    def __or__(self, other):
        return self.combine(other, "or")

    def __xor__(self, other):
        return self.combine(other, "xor")

    def __sub__(self, other):
        return self.combine(other, "minus")

    def tighten(self, device_id=None):
        """These masks with tight bounds -- the smallest box of every instance's set pixels, (0, 0, -1, -1) and no rows for one
        without a pixel -- and the canonical layout (padding bits 0, true areas): combine's "copy" without a window."""
        return self.combine(None, "copy", None, device_id)

    def crop(self, x1, y1, x2, y2, device_id=None):
        """These masks intersected with the window (x1, y1, x2, y2), inclusive, tight bounds: combine's "copy" in the window."""
        return self.combine(None, "copy", (x1, y1, x2, y2), device_id)

    def complement(self, H, W, device_id=None):
        """The pixels of the H x W image that every instance does not have, tight bounds: combine's "not" in the window (0, 0,
        W - 1, H - 1)."""
        return self.combine(None, "not", (0, 0, int(W) - 1, int(H) - 1), device_id)

    def merge(self, groups=None, intersect=False, by=None, device_id=None):
        """One instance per group of instances: their union, or with intersect their intersection (pycocotools' merge) -> a host
        PackedMasks with tight bounds, the class and score of every group's first member.  groups: a list of index lists (any
        order, repeats allowed, an empty list gives an empty instance); None: everything in one group; by="class": one group
        per distinct class in ascending class order -- the per-class semantic masks.  By the rule of
        mnc_amd.algebra.merge_numpy through mnc_mask_merge.  A device-resident result is fetched to the host first."""
        from . import algebra
        if by is not None:
            if by != "class" or groups is not None:
                raise ValueError("merge: by=%r is not \"class\", or groups were given as well" % (by,))
            groups = algebra.class_groups(self.classes)[1]
        elif groups is None:
            groups = [np.arange(len(self))]
        return algebra.merge(self, *algebra.groups_csr(groups), intersect=intersect, device_id=device_id)

    def layered(self, order=None, device_id=None):
        """These instances made pairwise disjoint: each minus the union of every instance before it in `order` (a permutation;
        None: descending score, the lower index first on equal scores -- nms()'s order), so that every pixel belongs to the best
        instance that covers it -> a host PackedMasks of len(self) instances in this order of indices, tight bounds, by the rule
        of mnc_amd.algebra.layer_numpy through mnc_mask_layer.  A device-resident result is fetched to the host first."""
        from . import algebra
        return algebra.layer(self, order, device_id)

    def translate(self, dx, dy):
        """These masks moved by (dx, dy) -> a host PackedMasks: arithmetic on the bounds, no bit is touched and nothing is
        tightened (mnc_amd.warp.translate)."""
        from . import warp
        return warp.translate(self, dx, dy)

    def isometry(self, code, tx=0, ty=0, device_id=None):
        """A lattice isometry and a translation: pixel (x, y) goes to (u + tx, v + ty) with (u, v) = (y, x) if code & 1 else (x, y),
        u negated if code & 2, v negated if code & 4 -> a host PackedMasks with tight bounds, by the rule of
        mnc_amd.warp.isometry_numpy (include/mnc_hip.h n18, csrc/mask_warp.hip) on the GPU.  A device-resident result is fetched
        to the host first."""
        from . import warp
        return warp.isometry(self, code, tx, ty, device_id)

    def fliplr(self, W, device_id=None):
        """These masks mirrored left to right in an image W wide (np.fliplr of full(i, H, W)): isometry(2, W - 1, 0)."""
        return self.isometry(2, int(W) - 1, 0, device_id)

    def flipud(self, H, device_id=None):
        """These masks mirrored top to bottom in an image H high (np.flipud): isometry(4, 0, H - 1)."""
        return self.isometry(4, 0, int(H) - 1, device_id)

    def transpose(self, device_id=None):
        """These masks with x and y exchanged (.T of full(i, H, W)): isometry(1, 0, 0)."""
        return self.isometry(1, 0, 0, device_id)

    def rot90(self, k, H, W, device_id=None):
        """These masks of an H x W image turned by k quarter turns in numpy's direction (np.rot90(full(i, H, W), k)), any integer
        k; an odd k gives masks of a W x H image."""
        from . import warp
        return self.isometry(*warp.rot90_code(k, H, W), device_id=device_id)

    def warp(self, coef, den, window, device_id=None):
        """The nearest-neighbour gather through an integer affine inverse map: destination pixel (x, y) of window = (x1, y1, x2, y2),
        inclusive, is set iff source pixel ((c0 x + c1 y + c2) // den, (c3 x + c4 y + c5) // den) is -> a host PackedMasks with
        tight bounds, by the rule of mnc_amd.warp.warp_numpy through mnc_mask_warp.  A device-resident result is fetched to the
        host first."""
        from . import warp
        return warp.warp(self, coef, den, window, device_id)

    def resize(self, H, W, H2, W2, device_id=None):
        """These masks of an H x W image in its centre-aligned nearest-neighbour resize to H2 x W2 (mnc_amd.warp.resize_map): warp
        in the window of the new image."""
        from . import warp
        return warp.warp(self, *warp.resize_map(H, W, H2, W2), window=(0, 0, int(W2) - 1, int(H2) - 1), device_id=device_id)

    def warp_affine(self, M, H2, W2, frac_bits=16, inverse=False, device_id=None):
        """These masks under the 2 x 3 float64 matrix M in cv2.warpAffine's convention, nearest neighbour, into an H2 x W2 image:
        warp by mnc_amd.warp.affine_map(M, frac_bits, inverse) in the window of that image."""
        from . import warp
        return warp.warp(self, *warp.affine_map(M, frac_bits, inverse), window=(0, 0, int(W2) - 1, int(H2) - 1), device_id=device_id)

    def rle_counts(self, H, W, device_id=None):
        """(run_ptr int64 [n + 1], runs uint32): the COCO run-length counts of every instance in an H x W image, column-major
        (mnc_amd.rle.rle_counts_numpy's rule; include/mnc_hip.h n7, csrc/mask_rle.hip) on the GPU.  A device-resident result is
        encoded where it lies (mnc_mask_rle_dev: only run_ptr and the runs come back); anything else goes through mnc_mask_rle on
        GPU device_id (None: cfg.GPU_ID)."""
        from . import rle
        dev = self._device()
        if dev is None:
            return rle.rle_counts(self, H, W, device_id)
        return rle.device_rle_counts(dev, H, W)

    def rle(self, H, W, device_id=None):
        """-> [{"size": [H, W], "counts": str}] per instance: COCO's compressed RLE of the instance in an H x W image."""
        from . import rle
        return rle._to_rles(*(self.rle_counts(H, W, device_id) + (H, W)))

    @classmethod
    def from_rle(cls, rles, classes=None, scores=None):
        """COCO RLEs of one image size ({"size": [H, W], "counts": str, bytes or an uncompressed list}) -> PackedMasks with tight
        bounds, decoded on the GPU (mnc_mask_from_rle)."""
        from . import rle
        return rle.masks_from_rle(rles, classes, scores)

    @classmethod
    def from_polygons(cls, segs, H, W, classes=None, scores=None):
        """COCO polygon segmentations of one H x W image -- segs[i] the list of annotation i's polygons, each a flat list [x0, y0,
        x1, y1, ...] -> PackedMasks with tight bounds, rasterised on the GPU by maskApi.c's rule (mnc_mask_from_polygons).  A
        coordinate list of odd length raises ValueError naming its indices."""
        from . import polygons
        return polygons.masks_from_polygons(segs, H, W, classes, scores)

    @classmethod
    def from_segmentations(cls, segs, H, W, classes=None, scores=None):
        """COCO `segmentation` entries of one H x W image, each a polygon list, a compressed RLE dict or an uncompressed RLE dict
        -> PackedMasks in the entries' order: one device call per kind, merged on the host."""
        from . import polygons
        return polygons.masks_from_segmentations(segs, H, W, classes, scores)

    @classmethod
    def from_labels(klass, label, cls=None, background=0, classes=None, device_id=None):
        """The instances of an integer label map [H, W] with values in [0, 2^24) -- the distinct values that are not `background`
        (one value, up to 8, or None), ascending -- -> (a host PackedMasks with tight bounds, ids int32 [n]), on the GPU by the
        rule of mnc_amd.labels.from_labels_numpy (include/mnc_hip.h n19, csrc/mask_labels.hip).  Classes: cls, a map of the same
        shape (an instance of mixed class raises ValueError), or classes, a dict or array looked up by id; else 0."""
        from . import labels
        return labels.from_labels(label, cls, background, classes, device_id)

    def to_labels(self, H, W, values=None, order=None, background=0, device_id=None):
        """The label map int32 [H, W] of these masks: a pixel gets values[i] (None: i + 1) of the first instance i in `order`
        (None: layered()'s, descending score) that has it set, `background` where none has, on the GPU by the rule of
        mnc_amd.labels.to_labels_numpy (mnc_mask_to_labels).  A device-resident result is fetched to the host first."""
        from . import labels
        return labels.to_labels(self, H, W, values, order, background, device_id)

    @classmethod
    def from_dense(cls, bounds, dense, classes=None, scores=None):
        """Per-instance bool [h, w] arrays (None, or one with a zero side: no rows) -> a host PackedMasks: offsets in order without
        gaps, areas the true counts, the given bounds [n, 4] stored as they are."""
        n = len(dense)
        offsets, areas, words, nbytes = np.zeros(n, np.int64), np.zeros(n, np.int64), [], 0
        for i, m in enumerate(dense):
            offsets[i] = nbytes
            if m is None or 0 in np.shape(m):
                continue
            m = np.asarray(m, bool)
            areas[i] = int(m.sum())
            words.append(pack_rows(m))
            nbytes += words[-1].nbytes
        return cls(bounds, offsets, areas, classes, scores, np.concatenate(words) if words else np.zeros(0, np.uint64))

    def take(self, indices):
        """-> a host PackedMasks of these instances, in this order: offsets repacked without gaps, the bits copied."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        bounds, offsets, areas, bits = merge_sets((self,), [(0, i) for i in idx])
        return PackedMasks(bounds, offsets, areas, self.classes[idx], self.scores[idx], bits)

    def arrays(self):
        """{name: array} of the six fields (what tools/demo.py --save-masks writes with np.savez)."""
        return {name: getattr(self, name) for name in self.FIELDS}

    @classmethod
    def load(cls, path):
        with np.load(path) as f:
            return cls(**{name: f[name] for name in cls.FIELDS})


def _flat(boxes, masks):
    boxes = np.asarray(boxes, np.float64)
    boxes = boxes.reshape(-1, boxes.shape[-1] if boxes.ndim > 1 else 4)
    n = boxes.shape[0]
    masks = np.asarray(masks, np.float32)
    S = int(masks.shape[-1]) if masks.ndim >= 2 and n else 0
    return boxes, np.ascontiguousarray(masks.reshape(n, S * S)), n, S


def from_lists(list_mask, list_box, score_thresh=0.0):
    """(list_result_mask, list_result_box) of gpu_mask_voting -> (boxes [n, 5] float64, masks [n, S, S] float32, classes int32
    [n]) of the instances with score >= score_thresh, class-major: the order and the rows tools/demo.py:get_vis_dict keeps."""
    boxes, masks, classes = [], [], []
    for c, (m, b) in enumerate(zip(list_mask, list_box)):
        keep = np.where(np.asarray(b)[:, -1] >= score_thresh)[0] if len(b) else np.zeros(0, int)
        boxes.append(np.asarray(b, np.float64).reshape(-1, 5)[keep])
        mm = np.asarray(m, np.float32)
        masks.append(mm.reshape(len(b), mm.shape[-1], mm.shape[-1])[keep] if len(b) else None)
        classes.append(np.full(len(keep), c + 1, np.int32))
    masks = [m for m in masks if m is not None]
    S = masks[0].shape[-1] if masks else 0
    return (np.concatenate(boxes) if boxes else np.zeros((0, 5)), np.concatenate(masks) if masks else np.zeros((0, S, S), np.float32),
            np.concatenate(classes) if classes else np.zeros(0, np.int32))


def _scores_of(boxes, scores):
    if scores is not None:
        return scores
    return boxes[:, 4] if boxes.shape[1] >= 5 else None


def instance_masks_numpy(boxes, masks, im_h, im_w, clip=True, binarize_thresh=None, classes=None, scores=None):
    """The rule as a plain loop on the host: per instance np.round(box) (clipped to the image with clip=True, as
    utils/vis_seg.py:_convert_pred_to_image; left alone with clip=False, as utils/voc_eval.py:voc_eval_sds),
    utils.blob.resize_to(mask, w, h) >= float32(binarize_thresh), packed.  boxes [n, 4 or 5] (a fifth column is the score), masks
    [n, S, S] or [n, 1, S, S] -> PackedMasks.  Raises ValueError where mnc_instance_masks returns MNC_ERR_INVALID."""
    from mnc_config import cfg
    from utils.blob import resize_to
    thr = np.float32(cfg.BINARIZE_THRESH if binarize_thresh is None else binarize_thresh)
    boxes, masks, n, S = _flat(boxes, masks)
    if n and not 1 <= S <= MAX_MASK:
        raise ValueError("instance_masks_numpy: mask_size %d not in [1, %d]" % (S, MAX_MASK))
    if clip and not (1 <= im_h <= MAX_SIDE and 1 <= im_w <= MAX_SIDE):
        raise ValueError("instance_masks_numpy: image %d x %d not in [1, %d]" % (im_h, im_w, MAX_SIDE))
    bounds, dense = np.zeros((n, 4), np.int32), []
    for i in range(n):
        r = np.round(boxes[i, :4])
        if not (np.abs(r) < MAX_COORD).all():
            raise ValueError("instance_masks_numpy: box %d out of range" % i)
        b = r.astype(int)
        if clip:
            b = np.array([min(max(b[0], 0), im_w - 1), min(max(b[1], 0), im_h - 1), min(max(b[2], 0), im_w - 1),
                          min(max(b[3], 0), im_h - 1)])
        w, h = int(b[2] - b[0] + 1), int(b[3] - b[1] + 1)
        if w < 1 or h < 1:
            raise ValueError("instance_masks_numpy: box %d %s is empty once rounded (cv2.resize would raise)" % (i, boxes[i, :4]))
        if w * h > MAX_AREA:
            raise ValueError("instance_masks_numpy: box %d covers %d pixels (limit %d)" % (i, w * h, MAX_AREA))
        bounds[i] = b
        dense.append(resize_to(masks[i].reshape(S, S), w, h) >= thr)
    return PackedMasks.from_dense(bounds, dense, classes, _scores_of(boxes, scores))


def instance_masks_call(boxes, masks, n, S, im_h, im_w, clip, binarize_thresh, bits=None, device_id=0):
    """mnc_instance_masks as it is: boxes float64 [n, 4], masks float32 [n, S*S]; bits None asks for bounds, offsets and the size
    only (nothing is launched).  -> (bounds, offsets, areas, bytes needed)."""
    bounds, offsets, areas = np.zeros((n, 4), np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    need = ctypes.c_size_t(0)
    _lib.call("mnc_instance_masks", _lib.ptr(boxes), _lib.ptr(masks), int(n), int(S), float(binarize_thresh), int(im_h), int(im_w),
              int(bool(clip)), _lib.ptr(bounds), _lib.ptr(offsets), _lib.ptr(areas), _lib.ptr(bits),
              bits.nbytes if bits is not None else 0, ctypes.addressof(need), int(device_id))
    return bounds, offsets, areas, int(need.value)


def instance_masks(boxes, masks, im_h, im_w, clip=True, binarize_thresh=None, classes=None, scores=None, device_id=None):
    """instance_masks_numpy on the GPU (mnc_instance_masks, csrc/inst_masks.hip): same arguments, the same PackedMasks bit for bit.
    Invalid boxes and sizes raise _lib.MncError (MNC_ERR_INVALID) before anything is launched."""
    from mnc_config import cfg
    thr = cfg.BINARIZE_THRESH if binarize_thresh is None else binarize_thresh
    device_id = _device_id(device_id)
    boxes, masks, n, S = _flat(boxes, masks)
    b4 = np.ascontiguousarray(boxes[:, :4])
    S = S if n else int(cfg.MASK_SIZE)
    bounds, offsets, areas, bits = sized_then_filled(
        lambda bits: instance_masks_call(b4, masks, n, S, im_h, im_w, clip, thr, bits, device_id))
    return PackedMasks(bounds, offsets, areas, classes, _scores_of(boxes, scores), bits)


def _from_info(raw, kept):
    info = raw[HEAD_BYTES:HEAD_BYTES + kept * INFO.itemsize].view(INFO)
    return {"bounds": np.ascontiguousarray(info["bounds"]), "offsets": np.ascontiguousarray(info["offset"]),
            "areas": np.ascontiguousarray(info["area"]), "classes": np.ascontiguousarray(info["cls"]),
            "scores": np.ascontiguousarray(info["score"])}


class _DeviceResult(object):
    """One mnc_mask_records result in the context's arena, which the next call on that context reuses."""
    FIRST = 128                                 # instances the first copy brings along (max_per_image is 100)

    def __init__(self, ctx, d_info, d_bits, rows):
        self._ctx, self._gen = ctx, ctx._mask_gen
        self.d_info, self.d_bits, self.rows = d_info, d_bits, int(rows)
        self._bytes = None

    def is_current(self):
        return self._ctx._mask_gen == self._gen

    def check(self):
        if not self.is_current():
            raise RuntimeError("these masks' device buffers have been reused by a later masks() on this context (read them, or "
                               ".fetch(), before the next image if they must outlive it)")

    def overlaps(self, kept, other):
        """mnc_mask_overlaps_dev of this result against `other` (a PackedMasks, read on the host; None: itself), the matrices
        copied to the host: -> (inter [kept, m], iou [kept, m])."""
        self.check()
        m = self.rows if other is None else len(other)
        d_inter, d_iou = ctypes.c_void_p(), ctypes.c_void_p()
        args = (None, None, None, None, 0, 0) if other is None else _set_args(other)
        _lib.call("mnc_mask_overlaps_dev", self._ctx.h, self.d_info, self.d_bits, self.rows, *(args + (
            ctypes.addressof(d_inter), ctypes.addressof(d_iou))))
        inter, iou = np.zeros((self.rows, m), np.int64), np.zeros((self.rows, m), np.float64)
        if inter.size:
            _lib.call("mnc_d2h_async", self._ctx.h, _lib.ptr(inter), d_inter.value, inter.nbytes)
            _lib.call("mnc_d2h", self._ctx.h, _lib.ptr(iou), d_iou.value, iou.nbytes)
        cols = kept if other is None else m
        return np.ascontiguousarray(inter[:kept, :cols]), np.ascontiguousarray(iou[:kept, :cols])

    def nms(self, thresh, class_aware):
        self.check()
        d_keep = ctypes.c_void_p()
        _lib.call("mnc_mask_nms_dev", self._ctx.h, self.d_info, self.d_bits, self.rows, float(thresh), int(bool(class_aware)),
                  ctypes.addressof(d_keep))
        raw = np.zeros(HEAD_BYTES // 4 + self.rows, np.int32)
        _lib.call("mnc_d2h", self._ctx.h, _lib.ptr(raw), d_keep.value, raw.nbytes)
        return raw[HEAD_BYTES // 4:HEAD_BYTES // 4 + int(raw[0])].copy()

    def load(self, host, want_bits):
        self.check()
        h = self._ctx.h
        if self._bytes is None:
            first = min(self.rows, self.FIRST)
            raw = np.zeros(HEAD_BYTES + self.rows * INFO.itemsize, np.uint8)
            _lib.call("mnc_d2h", h, _lib.ptr(raw), self.d_info, HEAD_BYTES + first * INFO.itemsize)
            head = raw[:HEAD_BYTES].view(HEAD)[0]
            kept = int(head["kept"])
            if kept > first:
                at = HEAD_BYTES + first * INFO.itemsize
                _lib.call("mnc_d2h", h, raw[at:].ctypes.data, self.d_info + at, (kept - first) * INFO.itemsize)
            host.update(_from_info(raw, kept))
            self._bytes = int(head["bits_bytes"])
        if want_bits:
            bits = np.zeros(self._bytes // 8, np.uint64)
            if bits.size:
                _lib.call("mnc_d2h", h, _lib.ptr(bits), self.d_bits, bits.nbytes)
            host["bits"] = bits


def records_masks(ctx, records_ptr, counts_ptr, record_cap, num_classes, mask_size, H, W, score_thresh=0.0, binarize_thresh=None):
    """Enqueue mnc_mask_records for the records at (records_ptr, counts_ptr) on the stream of `ctx` (an engine context object);
    -> PackedMasks whose arrays are copied on first access."""
    if binarize_thresh is None:
        from mnc_config import cfg
        binarize_thresh = cfg.BINARIZE_THRESH
    d_info, d_bits = ctypes.c_void_p(), ctypes.c_void_p()
    ctx._mask_gen = getattr(ctx, "_mask_gen", 0) + 1
    _lib.call("mnc_mask_records", ctx.h, records_ptr, counts_ptr, int(record_cap), int(num_classes), int(mask_size),
              float(score_thresh), float(binarize_thresh), int(H), int(W), ctypes.addressof(d_info), ctypes.addressof(d_bits))
    return PackedMasks(source=_DeviceResult(ctx, d_info.value, d_bits.value, record_cap))


def net_masks(net_handle, rows_cap, score_thresh, binarize_thresh):
    """mnc_net_masks: the last image of a native net -> PackedMasks on the host (a sizes-only call, then the call with room)."""
    raw = np.zeros(HEAD_BYTES + int(rows_cap) * INFO.itemsize, np.uint8)
    need = ctypes.c_size_t(0)
    _lib.call("mnc_net_masks", net_handle, float(score_thresh), float(binarize_thresh), _lib.ptr(raw), int(rows_cap), None, 0,
              ctypes.addressof(need))
    bits = np.zeros(need.value // 8, np.uint64)
    _lib.call("mnc_net_masks", net_handle, float(score_thresh), float(binarize_thresh), _lib.ptr(raw), int(rows_cap),
              _lib.ptr(bits) if bits.size else None, bits.nbytes, ctypes.addressof(need))
    return PackedMasks(bits=bits, **_from_info(raw, int(raw[:HEAD_BYTES].view(HEAD)[0]["kept"])))


def _pair_numpy(box1, box2, mask1, mask2):
    """inter of transform.mask_transform.mask_overlap: the same slices, the count alone."""
    x1, y1 = max(box1[0], box2[0]), max(box1[1], box2[1])
    x2, y2 = min(box1[2], box2[2]), min(box1[3], box2[3])
    if x1 > x2 or y1 > y2:
        return 0
    w, h = x2 - x1 + 1, y2 - y1 + 1
    ya, xa, yb, xb = y1 - box1[1], x1 - box1[0], y1 - box2[1], x1 - box2[0]
    return int(np.logical_and(mask2[yb:yb + h, xb:xb + w], mask1[ya:ya + h, xa:xa + w]).sum())


def mask_overlaps_numpy(a, b=None):
    """The rule as a plain double loop on the host: iou[i, j] = transform.mask_transform.mask_overlap(a.bounds[i], b.bounds[j],
    a.dense(i), b.dense(j)) (the reference's lib/transform/mask_transform.py:16-46; its int 0 read as 0.0), inter[i, j] the
    count behind it.  b None: a against itself.  -> (inter int64 [na, nb], iou float64 [na, nb])."""
    from transform.mask_transform import mask_overlap
    b = a if b is None else b
    da, db = [a.dense(i) for i in range(len(a))], [b.dense(j) for j in range(len(b))]
    ba, bb = [[int(v) for v in r] for r in a.bounds], [[int(v) for v in r] for r in b.bounds]
    inter, iou = np.zeros((len(a), len(b)), np.int64), np.zeros((len(a), len(b)), np.float64)
    for i in range(len(a)):
        for j in range(len(b)):
            inter[i, j] = _pair_numpy(ba[i], bb[j], da[i], db[j])
            iou[i, j] = mask_overlap(ba[i], bb[j], da[i], db[j])
    return inter, iou


def mask_nms_numpy(pm, thresh, class_aware=False):
    """The mask NMS as a plain loop on the host: the instances in score order (descending, equal scores lower index first), each
    kept unless one kept earlier has iou > thresh with it (strict) and, with class_aware, its class.  -> kept indices int32 in
    score order.  Raises ValueError on a NaN score or threshold."""
    thresh = float(thresh)
    scores = np.asarray(pm.scores, np.float32)
    if thresh != thresh or np.isnan(scores).any():
        raise ValueError("mask_nms_numpy: NaN score or threshold")
    _, iou = mask_overlaps_numpy(pm)
    keep = []
    for i in np.argsort(-scores, kind="stable"):
        if not any(iou[k, i] > thresh and (not class_aware or pm.classes[k] == pm.classes[i]) for k in keep):
            keep.append(int(i))
    return np.array(keep, np.int32)


def _set_args(pm, areas=True):
    """The six arguments of one host set; five, without the areas, for the entries that take none (mnc_mask_rle).  (An empty bits
    array still has an address: NULL would mean "B is A".)"""
    bits = pm.bits if pm.bits.size else np.zeros(1, np.uint64)
    return ((_lib.ptr(pm.bounds), _lib.ptr(pm.offsets)) + ((_lib.ptr(pm.areas),) if areas else ()) +
            (_lib.ptr(bits), int(pm.bits.nbytes), len(pm)))


def _device_id(device_id):
    if device_id is not None:
        return int(device_id)
    from mnc_config import cfg
    return int(cfg.get("GPU_ID", 0))


def mask_overlaps(a, b=None, device_id=None):
    """mask_overlaps_numpy on the GPU (mnc_mask_overlaps, csrc/mask_overlaps.hip): the same two matrices bit for bit.  Invalid
    sets raise _lib.MncError (MNC_ERR_INVALID) before anything is launched."""
    nb = len(a) if b is None or b is a else len(b)
    inter, iou = np.zeros((len(a), nb), np.int64), np.zeros((len(a), nb), np.float64)
    args_b = (None, None, None, None, 0, 0) if b is None or b is a else _set_args(b)
    _lib.call("mnc_mask_overlaps", *(_set_args(a) + args_b + (_lib.ptr(inter), _lib.ptr(iou), _device_id(device_id))))
    return inter, iou


def mask_nms(pm, thresh, class_aware=False, device_id=None):
    """mask_nms_numpy on the GPU (mnc_mask_nms): order, IoU, suppression words and the greedy scan on the device, the kept
    indices back in one copy."""
    n = len(pm)
    keep, num = np.zeros(max(n, 1), np.int32), ctypes.c_int(0)
    _lib.call("mnc_mask_nms", *(_set_args(pm)[:5] + (n, _lib.ptr(pm.classes), _lib.ptr(pm.scores), float(thresh),
                                                     int(bool(class_aware)), _lib.ptr(keep), ctypes.addressof(num),
                                                     _device_id(device_id))))
    return keep[:num.value].copy()
