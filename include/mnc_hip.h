/* mnc_hip.h -- C ABI of libmnc_hip.so: MNC's per-image inference hot path on MI355X (gfx950).
 *
 * This header is the drop-in boundary.  Plain C: pointers, ints, floats; no torch / C++
 * types.  Every entry point returns an int status (MNC_OK == 0) except the two reference-compatible `void`
 * wrappers `_nms` / `_mv`; the text of the last error on the calling thread is available from mnc_last_error().
 * Citations `file:line` are into the reference repository (daijifeng001/MNC).
 *
 * Pointer naming:  *_host = host memory owned by the caller;  d_* = device memory on the context's GPU.
 *
 * Device tensor layouts ("c8" = channel-blocked, chosen so that a wave's MFMA epilogue stores and the next layer's
 * halo loads are both fully coalesced -- see DESIGN.md section 3):
 *   feature map        c8   float [C/8][H][W][8]                      (batch is always 1, proposal_layer.py:65)
 *   conv3x3 weights    packed by mnc_pack_conv3x3_weights             float [Cin/8][Cout][76]  (9 taps x 8 cin + 4 pad)
 *   per-RoI features   hwc  float [R][PH][PW][C]   (a row of the FC GEMM is one RoI, k = (ph*PW+pw)*C + c)
 *   FC weights         packed by mnc_pack_fc_weights: rows = outputs, columns permuted from Caffe's (c,h,w) order
 *                      (test.prototxt InnerProduct, SURVEY App. A graph-5) to the hwc order above
 *   everything else    as in Caffe: rois [R][5], masks [R][1][21][21], probabilities [R][21], ... row-major.
 */
#ifndef MNC_HIP_H_
#define MNC_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNC_API __attribute__((visibility("default")))

enum {
  MNC_OK = 0,
  MNC_ERR_INVALID = 1,     /* bad argument (null pointer, negative size, unsupported shape) */
  MNC_ERR_HIP = 2,         /* a HIP runtime call or kernel launch failed */
  MNC_ERR_NOMEM = 3,       /* device or host allocation failed */
  MNC_ERR_STATE = 4,       /* call order violated (e.g. forward before weights were loaded) */
  MNC_ERR_UNSUPPORTED = 5  /* valid request this build cannot serve */
};

/* Thread-local, never NULL; "" when the last call on this thread succeeded. */
MNC_API const char* mnc_last_error(void);
MNC_API int mnc_device_count(int* count);
/* Free and total bytes of device `device_id` (hipMemGetInfo): what a host that keeps several nets per GPU checks its budget with
 * (bench.py prints total - free per rank: four images in flight x 1.1 GB of replicated weights + activations). */
MNC_API int mnc_device_mem_info(int device_id, size_t* free_bytes, size_t* total_bytes);
MNC_API const char* mnc_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * b1  nms.gpu_nms  --  replaces `_nms` (lib/nms/gpu_nms.hpp:1-2, lib/nms/nms_kernel.cu:91-144), called from
 *     gpu_nms.pyx:16-31.  boxes_host: [boxes_num][boxes_dim] float32 ALREADY SORTED by descending score; only
 *     columns 0..3 are read.  keep_out has capacity boxes_num and receives positions in the sorted array.
 *     Suppression is `IoU > thresh` (strict, nms_kernel.cu:71) with +1 widths; results are bit-exact with the
 *     reference.  boxes_num == 0 is legal (num_out = 0).  Synchronous.  max_keep < 0 means "all".
 * ------------------------------------------------------------------------------------------------------------- */
MNC_API int mnc_nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
                    float nms_overlap_thresh, int device_id);
/* Same, but stops after max_keep survivors (ProposalLayer only uses keep[:300], proposal_layer.py:151-153);
 * the first max_keep indices are identical to the unbounded call. */
MNC_API int mnc_nms_topk(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
                         float nms_overlap_thresh, int max_keep, int device_id);
/* Batched form for gpu_mask_voting's per-class loop (lib/transform/mask_transform.py:228-240): `batch` NMS problems
 * over ONE box set.  order_host: [batch][boxes_num] int32, item b's boxes in descending score order (indices into
 * boxes_host, i.e. the `argsort()[::-1]` gpu_nms.pyx:26 computes per call).  keep_out: [batch][boxes_num] int32 positions in
 * item b's order (first num_out[b] valid); num_out: [batch].  Each item's result is bit-identical to mnc_nms_topk on
 * boxes_host[order_host[b]].  One mask launch + one scan launch + one copy each way. */
MNC_API int mnc_nms_batched(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
                            const int* order_host, int batch, float nms_overlap_thresh, int max_keep, int device_id);
/* The raw 64x64-tiled suppression bitmask (nms_kernel.cu:34-78) for word-for-word parity tests:
 * mask_host has boxes_num * ceil(boxes_num/64) uint64 words, row-major.  Lower-triangle words (never read by the
 * scan, nms_kernel.cu:135) are written as 0. */
MNC_API int mnc_nms_mask(unsigned long long* mask_host, const float* boxes_host, int boxes_num, int boxes_dim,
                         float nms_overlap_thresh, int device_id);
/* The reference's own symbol, twice.
 *  (1) C++ linkage -- `_Z4_nmsPiS_PKfiifi` -- which is what the reference's extension links: gpu_nms.pyx:13-14 declares it with
 *      `cdef extern from "gpu_nms.hpp"` and lib/setup.py:126-130 compiles that extension with language='c++', so the call is a
 *      C++ call of `void _nms(int*, int*, const float*, int, int, float, int)` (gpu_nms.hpp:1-2).  libmnc_hip.so exports that
 *      mangled name (csrc/ref_cxx_abi.hip); a C++ translation unit gets the declaration by including the reference's
 *      gpu_nms.hpp itself, or this header with MNC_HIP_REF_CXX_NAMES defined.
 *  (2) C linkage `_nms`, same arguments, for dlsym / ctypes / cgo callers (the default declaration of this header).
 * Both report errors through mnc_last_error() and a line on stderr, and set *num_out = 0 (the reference aborts in CUDA_CHECK). */
#if defined(__cplusplus) && defined(MNC_HIP_REF_CXX_NAMES)
}  /* leave extern "C" for the two C++-linkage names */
MNC_API void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
                  float nms_overlap_thresh, int device_id);
MNC_API void _mv(const float* all_boxes, const float* all_masks, const int all_boxes_num, const int* candidate_inds,
                 const int* candidate_start, const float* candidate_weights, const int candidate_num,
                 const int image_height, const int image_width, const int box_dim, const int mask_size,
                 const int result_num, float* finalize_output_mask, int* finalize_output_box, const int device_id);
extern "C" {
#else
MNC_API void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
                  float nms_overlap_thresh, int device_id);
#endif

/* ---------------------------------------------------------------------------------------------------------------
 * b2  nms.mv  --  replaces `_mv` (lib/nms/gpu_mv.hpp:1-4, lib/nms/mv_kernel.cu:242-348), called from
 *     gpu_mv.pyx:13-31.  Same 15 arguments, same meaning.  candidate_start[r] is the END offset of result r
 *     (mask_transform.py:268).  finalize_output_mask: [result_num][mask_size][mask_size] float32;
 *     finalize_output_box: [result_num][4] int32 (x1,y1,x2,y2).  result_num == 0 or candidate_num == 0 is legal.
 *     The render -> aggregate -> reduce -> resize chain is fused; the N*H*W render buffer is never materialised.
 *     Results are bit-exact with the reference kernels evaluated without FMA contraction.  device_id IS honoured
 *     (the reference ignores it).
 * ------------------------------------------------------------------------------------------------------------- */
MNC_API int mnc_mv(const float* all_boxes, const float* all_masks, int all_boxes_num, const int* candidate_inds,
                   const int* candidate_start, const float* candidate_weights, int candidate_num, int image_height,
                   int image_width, int box_dim, int mask_size, int result_num, float* finalize_output_mask,
                   int* finalize_output_box, int device_id);
/* `_mv`: exported with C++ linkage (`_Z3_mvPKfS0_iPKiS2_S0_iiiiiiPfPii`, what gpu_mv.pyx:7-8 + lib/setup.py:143-147 link)
 * and with C linkage, as `_nms` above. */
#if !(defined(__cplusplus) && defined(MNC_HIP_REF_CXX_NAMES))
MNC_API void _mv(const float* all_boxes, const float* all_masks, const int all_boxes_num, const int* candidate_inds,
                 const int* candidate_start, const float* candidate_weights, const int candidate_num,
                 const int image_height, const int image_width, const int box_dim, const int mask_size,
                 const int result_num, float* finalize_output_mask, int* finalize_output_box, const int device_id);
#endif

/* gpu_mask_voting in ONE call (lib/transform/mask_transform.py:213-286): per-class NMS (batched on the device) -> global
 * score threshold -> candidate sets {IoU_f64 >= iou_thresh} with class-score weights divided by float32(sequential float64 sum)
 * (python's sum() under the numpy 1.x the reference ran on, :266) -> fused mask voting kernels.  All host pointers.
 *   boxes [n][4] f32 (original-image pixels), masks [n][S][S] f32, scores [n][num_classes] f32 (column 0 = background),
 *   order [num_classes-1][n] i32: for class c+1, box indices by descending scores[:,c+1] (the caller's argsort()[::-1],
 *         gpu_nms.pyx:26), or NULL: the library orders each class itself (on the device) exactly as
 *         np.argsort(-scores[:, c+1], kind="stable") does -- ties in index order, NaN last.
 * Order, NMS, the global threshold, result rows, candidate sets (double-precision IoU) and voting all run on the device as one
 * asynchronous launch sequence; the host copies the inputs up and the result records down.
 * Limit: (num_classes-1) * min(max_per_image, n) <= 8192 kept boxes.
 * Outputs (capacity (num_classes-1)*min(max_per_image, n) rows): out_mask [R][S][S], out_box [R][4] i32, out_score [R],
 * class_count [num_classes-1] (rows per class, in class order), *result_num = R.
 * Bit-identical to running nms.gpu_nms x (num_classes-1), utils.cython_bbox.bbox_overlaps and nms.mv.mv as the reference does. */
MNC_API int mnc_mask_voting(const float* boxes, const float* masks, const float* scores, const int* order, int n,
                            int num_classes, int mask_size, int max_per_image, float nms_thresh, float iou_thresh,
                            int image_height, int image_width, float* out_mask, int* out_box, float* out_score,
                            int* class_count, int* result_num, int device_id);

/* cpu_mask_voting (lib/transform/mask_transform.py:107-210; cfg.TEST.USE_GPU_MASK_MERGE = False) in ONE call, host pointers:
 * the arguments of mnc_mask_voting (the library orders each class itself: order = NULL semantics) plus the binarisation
 * threshold (cfg.BINARIZE_THRESH).  Rows, candidate sets and weights are those of mnc_mask_voting with one difference: the kept
 * boxes of a class are re-sorted by the reference's ind_scores.argsort()[::-1] (:173-175), pinned as a stable ascending sort
 * reversed -- equal scores come out in reverse keep order -- before the max_per_image cut.  The voting is image-space: every
 * box rounded half to even, its mask resized to the rounded box with cv2.resize INTER_LINEAR (oracle/host.py:
 * resize_bilinear_cv_to), binarised with >= float32(binarize_thresh), weighted and summed in float64 on an image canvas in
 * candidate order; the result box is the extent of {canvas >= binarize_thresh} (none: the centre pixel (W // 2, H // 2)), the
 * mask that region cast to float32 and resized to S x S with the same rule.  The canvas is never stored (csrc/mv_image.hip).
 * Every rounded box must have x1 <= x2 and y1 <= y2 (the reference's cv2.resize raises otherwise): MNC_ERR_INVALID.  Boxes are
 * expected inside the image, as clipped boxes are.  Outputs as mnc_mask_voting's, bit-identical to the reference's
 * cpu_mask_voting with the tie order above. */
MNC_API int mnc_mask_voting_image(const float* boxes, const float* masks, const float* scores, int n, int num_classes,
                                  int mask_size, int max_per_image, float nms_thresh, float iou_thresh, double binarize_thresh,
                                  int image_height, int image_width, float* out_mask, int* out_box, float* out_score,
                                  int* class_count, int* result_num, int device_id);

/* ---------------------------------------------------------------------------------------------------------------
 * n1  The pixel counting of the SDS mAP^r evaluation (lib/utils/voc_eval.py:195-283 voc_eval_sds with
 *     lib/transform/mask_transform.py:16-46 mask_overlap), host pointers, one call for a whole dataset (csrc/sds_eval.hip).
 * ------------------------------------------------------------------------------------------------------------- */
/* For every prediction p: boxes [P][4] float64 (x1, y1, x2, y2), rounded half to even; masks [P][mask_size^2] bytes, taken as
 * float32, resized to the rounded box with cv2.resize INTER_LINEAR and binarised with >= float32(binarize_thresh).  Its GTs are
 * [gt_begin[p], gt_end[p]) of the GT arrays: gt_bounds [G][4] int (x1, y1, x2, y2), gt_offsets [G] byte offsets into gt_bits
 * (gt_bytes bytes) of the GT's bit rows, each ceil(w / 8) bytes with bit x at bit x % 8 of byte x / 8
 * (np.packbits(mask, axis=1, bitorder='little')), gt_areas [G] its set bits.  With inter = pixels set in both inside the
 * intersection of the two rectangles and union = area_g + area_p - inter, ov = (double)inter / (double)union (0 when the
 * rectangles do not meet or union < 1); best_gt[p] is the first GT of the range with a strictly greater ov than all before it,
 * starting from -1000 (-1 for an empty range), best_inter[p] / best_union[p] its inter and union (0 / 0 for -1).  Already
 * matched GTs are not excluded: matching at a threshold is the caller's (utils/voc_eval.py:voc_eval_sds_device).
 * P == 0 returns before any device work.  MNC_ERR_INVALID for bad sizes, ranges or GT rows outside gt_bytes, and for any rounded
 * box with x2 < x1 or y2 < y1 (cv2.resize raises on it), checked before anything is launched; limits: mask_size <= 32,
 * |coordinates| < 2^24, at most 2^26 pixels per rounded box or GT bound. */
MNC_API int mnc_sds_best_overlap(const double* boxes, const unsigned char* masks, int P, int mask_size, const int* gt_begin,
                                 const int* gt_end, int G, const int* gt_bounds, const long long* gt_offsets,
                                 const unsigned char* gt_bits, size_t gt_bytes, const long long* gt_areas,
                                 double binarize_thresh, int* best_gt, long long* best_inter, long long* best_union,
                                 int device_id);

/* ---------------------------------------------------------------------------------------------------------------
 * n4  The visualisation tail: instance-id and class-id label maps of the voted instances (lib/utils/vis_seg.py:101-130
 *     _convert_pred_to_image), their VOC colours (:134-147) and the blend over the photograph (csrc/render.hip).
 * ------------------------------------------------------------------------------------------------------------- */
/* _convert_pred_to_image in ONE call, host pointers.  boxes [n][4] float64 (the rows of pred_dict['boxes'] without the score),
 * masks [n][mask_size^2] float32, classes [n].  Per instance i, in list order: the box is rounded half to even and each coordinate
 * clipped to [0, W-1] / [0, H-1]; the mask is resized to the box with cv2.resize INTER_LINEAR and binarised with
 * >= float32(binarize_thresh); set pixels get i + 1 in inst_img and classes[i] in cls_img; then cls_img gets the box outline, value
 * 150, as the four numpy slices [y1:y2+1, x1-1:x1+1], [y1:y2+1, x2-1:x2+1], [y1-1:y1+1, x1:x2+1], [y2-1:y2+1, x1:x2+1] -- a slice
 * that would start at -1 is EMPTY, so a side at coordinate 0 is not drawn at all.  Later instances overwrite earlier ones; the
 * kernel evaluates that order-free per pixel (csrc/render.hip).  inst_img / cls_img [H][W] int32, either may be NULL; n == 0 gives
 * zero images.  Bit-identical to the reference function.
 * MNC_ERR_INVALID, checked before anything is launched: mask_size > 32, a rounded |coordinate| >= 2^24, H or W outside
 * [2, 32768] (below 2 the -1 slices would wrap instead of being empty), and any rounded, clipped box with x2 < x1 or y2 < y1
 * (cv2.resize raises on it). */
MNC_API int mnc_render_instances(const double* boxes, const float* masks, const int* classes, int n, int mask_size,
                                 double binarize_thresh, int image_height, int image_width, int* inst_img, int* cls_img,
                                 int device_id);

/* ---------------------------------------------------------------------------------------------------------------
 * n5  The instances themselves: one binary mask per instance at image resolution, one bit per pixel (csrc/inst_masks.hip) --
 *     the rule of _convert_pred_to_image (clip = 1) and of voc_eval_sds (clip = 0, lib/utils/voc_eval.py:197-199) without the
 *     painting over one another resp. the counting against ground truth that follow it there.
 * ------------------------------------------------------------------------------------------------------------- */
/* One instance of mnc_mask_records / mnc_net_masks (64 bytes).  Its mask is h = y2 - y1 + 1 rows of ceil(w / 64) little-endian
 * 64-bit words, w = x2 - x1 + 1, at byte `offset` of the bits: bit dx % 64 of word dx / 64 of row dy is pixel (x1 + dx, y1 + dy),
 * padding bits are 0 -- np.unpackbits(rows.view(np.uint8), axis=1, bitorder='little')[:, :w]; the first ceil(w / 8) bytes of a
 * row are utils.voc_eval.pack_sds_gt's row.  x2 < x1 or y2 < y1 (mnc_mask_records only): no rows. */
typedef struct mnc_mask_info {
  int x1, y1, x2, y2;   /* the rounded (and clipped) box: the bounds of the mask */
  int cls;              /* the record's class id */
  float score;          /* the record's score */
  int row;              /* row of the record array */
  int reserved0;
  long long offset;     /* byte offset of the first row; a multiple of 8, instances follow one another without gaps */
  long long area;       /* set bits */
  long long work;       /* the pack kernel's own (first work item of the instance) */
  long long reserved1;
} mnc_mask_info;
/* What stands in front of the mnc_mask_info array: 256 bytes. */
typedef struct mnc_mask_head {
  int kept;             /* instances */
  int reserved0;
  long long bits_bytes; /* bytes of all masks */
  long long items;      /* the pack kernel's own */
  long long reserved1[29];
} mnc_mask_head;
/* Host pointers, one call per image.  boxes [n][4] float64 (x1, y1, x2, y2), masks [n][mask_size^2] float32.  Per instance i:
 * every coordinate is rounded half to even (np.round); with clip = 1 it is then clipped to [0, W-1] / [0, H-1] exactly as
 * _convert_pred_to_image does, with clip = 0 (the evaluation's rule) nothing more happens, the bounds may leave the image and H, W
 * are not looked at.  w = x2 - x1 + 1, h = y2 - y1 + 1; pixel (dy, dx) of the mask is set when cv2.resize(mask, (w, h)),
 * INTER_LINEAR, is >= float32(binarize_thresh) there.  Outputs: bounds [n][4] int, offsets [n] (bytes into bits, each a multiple
 * of 8, in order without gaps), areas [n] (set bits), the rows of every instance in bits (layout: mnc_mask_info above),
 * *bits_bytes = the bytes they take.  bounds, offsets and *bits_bytes follow from the boxes alone and are computed on the host
 * before anything is launched: with bits == NULL the call returns them and launches nothing (masks and areas may be NULL then).
 * n == 0 returns before any device work (*bits_bytes = 0).  Bit-identical to utils.blob.resize_to(...) >= float32(thresh).
 * MNC_ERR_INVALID, checked before anything is launched: mask_size outside [1, 32], a rounded |coordinate| >= 2^24, more than
 * 2^26 pixels in one box, clip = 1 with H or W outside [1, 32768], bits_cap < *bits_bytes, and any rounded (and clipped) box with
 * x2 < x1 or y2 < y1 (cv2.resize raises on it; the rule of mnc_render_instances). */
MNC_API int mnc_instance_masks(const double* boxes, const float* masks, int n, int mask_size, double binarize_thresh,
                               int image_height, int image_width, int clip, int* bounds, long long* offsets, long long* areas,
                               void* bits, size_t bits_cap, size_t* bits_bytes, int device_id);

/* ---------------------------------------------------------------------------------------------------------------
 * n6  Comparing the instances: the mask IoU of every pair of two sets of packed masks, and the greedy mask NMS built on it
 *     (csrc/mask_overlaps.hip) -- the rule of transform.mask_transform.mask_overlap (lib/transform/mask_transform.py:16-46)
 *     on the layout of n5, without unpacking a mask.  The forms that read a device-resident mnc_mask_records result
 *     (mnc_mask_overlaps_dev, mnc_mask_nms_dev) stand beside that entry below.
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers.  Two sets A (na instances) and B (nb) in the same image frame, each given as n5 gives them: bounds [n][4] int
 * (x1, y1, x2, y2), offsets [n] (bytes into bits), areas [n], bits (h rows of ceil(w / 64) little-endian 64-bit words per
 * instance, layout: mnc_mask_info above), *_bytes = the bytes bits holds.  b_bits == NULL: B is A (the other b arguments and nb
 * are not looked at).  For every pair (a, b):
 *   ix1 = max(ax1, bx1), iy1 = max(ay1, by1), ix2 = min(ax2, bx2), iy2 = min(ay2, by2); ix1 > ix2 or iy1 > iy2: inter = 0 and
 *   iou = 0.0.  Otherwise inter = the pixels of that rectangle set in both masks, union = a_areas[a] + b_areas[b] - inter (the
 *   areas as given: the reference takes mask.sum() of what it is handed), iou = union < 1 ? 0.0 : (double)inter / (double)union.
 *   An instance without rows (x2 < x1 or y2 < y1) gives 0 / 0.0 against everything.  Bounds may leave the image (clip = 0);
 *   pixels outside it count like any others.  Padding bits are not trusted: a bit at column >= w of either operand is never
 *   counted, whatever it holds.
 * Outputs inter [na][nb] and iou [na][nb], row-major; either may be NULL.  With the areas the true bit counts every element
 * equals mask_overlap(A.bounds[a], B.bounds[b], A.dense(a), B.dense(b)) bit for bit (its int 0 read as 0.0).  na == 0 or nb == 0
 * returns before any device work.  MNC_ERR_INVALID, checked on the host before anything is launched: a negative count,
 * na * nb > 2^22, both outputs NULL, |coordinate| >= 2^24, more than 2^26 pixels in one bound, an offset that is negative or
 * not a multiple of 8, rows that reach past *_bytes. */
MNC_API int mnc_mask_overlaps(const int* a_bounds, const long long* a_offsets, const long long* a_areas, const void* a_bits,
                              size_t a_bytes, int na, const int* b_bounds, const long long* b_offsets, const long long* b_areas,
                              const void* b_bits, size_t b_bytes, int nb, long long* inter, double* iou, int device_id);
/* Greedy mask NMS of one set (host pointers; the set as above, classes [n] (may be NULL when class_aware = 0), scores [n]
 * float32; n <= 2048).  This library's own rule, the reference has none: order the instances by score descending, equal scores
 * lower index first (np.argsort(-scores, kind="stable")); walk that order; instance i is kept unless an instance k kept earlier
 * has iou(k, i) > thresh (strict, as nms_kernel.cu:71) and, with class_aware = 1, classes[k] == classes[i].  keep_out [n]
 * receives the kept indices in score order, *num_out their count.  Order, IoU, suppression words and the greedy scan (nms.hip's)
 * run on the device; the count and the kept rows come back in one copy.  MNC_ERR_INVALID as mnc_mask_overlaps, and: n outside
 * [0, 2048], a NaN score, a NaN thresh, class_aware not 0 / 1. */
MNC_API int mnc_mask_nms(const int* bounds, const long long* offsets, const long long* areas, const void* bits, size_t bytes,
                         int n, const int* classes, const float* scores, double thresh, int class_aware, int* keep_out,
                         int* num_out, int device_id);

/* ---------------------------------------------------------------------------------------------------------------
 * n7  The way out and back: COCO run-length encoding of packed instance masks (csrc/mask_rle.hip) -- the rule of the published
 *     maskApi.c (rleEncode, rleDecode, rleToBbox) on the layout of n5, without unpacking a mask.  An H x W image is read column
 *     by column: pixel (x, y) stands at position p = x * H + y.  The counts of a mask are the lengths of its runs of 0 and of 1
 *     in turn, beginning with a run of 0 (of length 0 when pixel (0, 0) is set): with t_0 < t_1 < ... the positions whose pixel
 *     differs from the pixel before (the one before position 0 counts as 0), counts = diff([0, t_0, ..., t_{T-1}, H * W]), T + 1
 *     entries that sum to H * W.  An empty mask gives [H * W], a full one [0, H * W]; apart from the first, no count is 0.  The
 *     compressed ASCII form of the counts (rleToString) is made on the host: mnc_amd/rle.py.  The form that reads a
 *     device-resident mnc_mask_records result (mnc_mask_rle_dev) stands beside that entry below.
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers.  The set as mnc_mask_overlaps takes it: bounds [n][4] int, offsets [n], bits, bytes = the bytes bits holds
 * (the areas are not needed).  Instance i covers the bits inside its bounds that also lie inside the H x W image (bounds may
 * leave it: clip = 0); an instance without rows is empty; padding bits (column >= w of a row) are not trusted and never counted.
 * Outputs: run_ptr [n + 1] (run_ptr[0] = 0; the counts of instance i are runs[run_ptr[i] .. run_ptr[i + 1])), runs (uint32),
 * *runs_total = run_ptr[n].  runs == NULL: run_ptr and *runs_total only (the counting passes alone run).  Otherwise runs_cap is
 * the room of runs in entries; runs_cap < *runs_total is MNC_ERR_INVALID with run_ptr and *runs_total set, so that the caller
 * calls again with room.  The order of the output comes from a scan over columns and instances, never from atomics: the result
 * is the same bits from run to run.  n == 0 returns before any device work (*runs_total = 0).  MNC_ERR_INVALID, checked on
 * the host before anything is launched: n outside [0, 2048], H or W outside [1, 32768] (H * W <= 2^30: counts and positions fit
 * 32 bits), |coordinate| >= 2^24, more than 2^26 pixels in one bound, an offset that is negative or not a multiple of 8, rows
 * that reach past bytes. */
MNC_API int mnc_mask_rle(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int H, int W,
                         long long* run_ptr, unsigned* runs, size_t runs_cap, size_t* runs_total, int device_id);
/* The reverse (host pointers): n masks of one H x W image given as counts -- run_ptr [n + 1] (non-negative, not decreasing),
 * runs (uint32) -- to the layout of n5.  Pixel p is set when it lies in a run of odd index; runs of length 0 are accepted
 * anywhere (the published decoder accepts them; encoding the result gives the canonical counts).  The bounds of an instance are
 * the tight box of its set pixels (rleToBbox); an empty mask gets (0, 0, -1, -1), no rows and area 0.  Outputs: bounds [n][4],
 * offsets [n] (multiples of 8, in order without gaps), areas [n] (the true bit counts), the rows in bits (padding bits 0),
 * *bits_bytes = the bytes they take.  A first kernel reduces bounds and areas over the runs of 1, the host forms the offsets, a
 * second kernel writes every word of every row once (nothing needs to be zeroed beforehand).  bits == NULL: bounds, offsets,
 * areas and *bits_bytes only.  n == 0 returns before any device work.  MNC_ERR_INVALID, checked on the host before anything is
 * launched: n outside [0, 2048], H or W outside [1, 32768], a negative or decreasing run_ptr, a mask whose counts do not sum to
 * H * W exactly; and, after the bounds pass, bits_cap < *bits_bytes (*bits_bytes is set). */
MNC_API int mnc_mask_from_rle(const long long* run_ptr, const unsigned* runs, int n, int H, int W, int* bounds, long long* offsets,
                              long long* areas, void* bits, size_t bits_cap, size_t* bits_bytes, int device_id);

/* ---------------------------------------------------------------------------------------------------------------
 * n8  Scoring the instances: COCO's matching of one image's detections to its ground truths (csrc/mask_match.hip) -- the rule of
 *     the published cocoeval.py (computeIoU, evaluateImg) and of rleIou in maskApi.c on the layout of n5, the counts those of
 *     n6.  The statement of the rule is mnc_amd/coco_eval.py:match_numpy; accumulation and the twelve summary numbers are host
 *     numpy there.  The form that reads a device-resident mnc_mask_records result (mnc_mask_match_dev) stands beside that
 *     entry below.
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers.  The detections (nd, with dt_classes [nd] and dt_scores [nd] float32) and the ground truths (ng, with
 * gt_classes [ng], gt_crowd [ng] bytes 0 / 1, gt_ignore_in [ng] bytes 0 / 1 or NULL for all 0, gt_eval_area [ng] or NULL for
 * gt_areas) are two sets in the same image frame as mnc_mask_overlaps takes them.  iou_thrs [T], area_rngs [A][2] (lo, hi),
 * max_det.  A detection only sees ground truths of its class.
 *   rank[d]     = the detections of d's class with a higher score, or the same score and a lower index
 *                 (np.argsort(-scores, kind="mergesort") per class).  rank[d] >= max_det: d takes no part (unmatched, not ignored).
 *   iou[d][g]   = union < 1 ? 0.0 : (double)inter / (double)union, inter the count of mnc_mask_overlaps (padding bits never
 *                 counted), union = dt_areas[d] + gt_areas[g] - inter, for a crowd ground truth dt_areas[d]; pairs of different
 *                 classes included.
 *   gt_ignore[a][g] = gt_ignore_in[g] or gt_crowd[g] or gt_eval_area[g] < lo_a or gt_eval_area[g] > hi_a.
 *   Per (a, t) the class's participating detections in rank order; each takes, among the not-ignored ground truths of its class
 *   that no earlier detection took and whose iou >= min(iou_thrs[t], 1 - 1e-10), the one of largest iou, of several equal the
 *   highest index; if there is none, the same choice among the ignored ones that are crowd or not yet taken (a not-ignored
 *   ground truth wins over an ignored one of larger iou) -- the closed form of evaluateImg's walk.  A match m sets
 *   dt_match[a][t][d] = m, gt_match[a][t][m] = d (a crowd ground truth keeps the last detection that took it) and
 *   dt_ignore[a][t][d] = gt_ignore[a][m]; a participating detection without a match gets dt_ignore = 1 when dt_areas[d] < lo_a
 *   or > hi_a.
 * Outputs, in the caller's index order, -1 for "none": rank [nd], dt_match [A][T][nd], dt_ignore [A][T][nd] (bytes), gt_match
 * [A][T][ng], gt_ignore [A][ng] (bytes), iou [nd][ng] (may be NULL).  Ranks, lists, IoU table and matching run on the device
 * without atomics and without a read-back in between: the same bits from run to run.  nd == 0 or ng == 0 returns before any
 * device work with every table filled as the rule gives.  MNC_ERR_INVALID, checked on the host before anything is launched:
 * everything mnc_mask_overlaps refuses; nd or ng outside [0, 2048]; T outside [1, 16]; A outside [1, 8]; max_det outside
 * [1, 2048]; a NaN score, threshold or range bound; lo > hi; a crowd or ignore byte other than 0 / 1; a NULL output other than
 * iou. */
MNC_API int mnc_mask_match(const int* dt_bounds, const long long* dt_offsets, const long long* dt_areas, const void* dt_bits,
                           size_t dt_bytes, int nd, const int* dt_classes, const float* dt_scores, const int* gt_bounds,
                           const long long* gt_offsets, const long long* gt_areas, const void* gt_bits, size_t gt_bytes, int ng,
                           const int* gt_classes, const unsigned char* gt_crowd, const unsigned char* gt_ignore_in,
                           const double* gt_eval_area, const double* iou_thrs, int T, const double* area_rngs, int A, int max_det,
                           int* rank, int* dt_match, unsigned char* dt_ignore, int* gt_match, unsigned char* gt_ignore,
                           double* iou, int device_id);

/* ---------------------------------------------------------------------------------------------------------------
 * n9  The way in from annotation files: COCO polygon segmentations rasterised into the layout of n5 (csrc/mask_poly.hip) -- the
 *     rule of the published maskApi.c (rleFrPoly per polygon, then the union of an annotation's polygons as annToRLE's
 *     frPyObjects + merge).  The statement of the rule is mnc_amd/polygons.py:polygon_counts_numpy / masks_from_polygons_numpy.
 *     One polygon of k >= 1 vertices (x_j, y_j) (doubles) in an H x W image; all arithmetic IEEE double in exactly this order,
 *     nothing contracted into an FMA, (int) truncates toward zero:
 *     1. X[j] = (int)(5 * x_j + .5), Y[j] = (int)(5 * y_j + .5) for j < k; X[k] = X[0], Y[k] = Y[0].
 *     2. Edge j: xs, xe, ys, ye = X[j], X[j+1], Y[j], Y[j+1]; dx = |xe - xs|, dy = |ys - ye|; flip = (dx >= dy && xs > xe) ||
 *        (dx < dy && ys > ye), and a flipped edge swaps xs with xe and ys with ye.  dx >= dy: s = (double)(ye - ys) / dx and for
 *        d = 0 .. dx, t = flip ? dx - d : d, the point u = t + xs, v = (int)(ys + s * t + .5).  Otherwise s = (double)(xe - xs) / dy
 *        and for d = 0 .. dy, t = flip ? dy - d : d, the point v = t + ys, u = (int)(xs + s * t + .5).  dx == dy == 0 gives the one
 *        point (xs, ys) (the published code forms 0 / 0 for a v that is never read).  The points of all edges are one list.
 *     3. Every point j >= 1 of the list with u[j] != u[j-1] is a crossing when xd = ((u[j] < u[j-1] ? u[j] : u[j] - 1) + .5) / 5
 *        - .5 is an integer with 0 <= xd <= W - 1; its row is yd = ceil(clamp(((v[j] < v[j-1] ? v[j] : v[j-1]) + .5) / 5 - .5,
 *        0, H)), and it toggles position a = (int)xd * H + (int)yd of the column-major pixel order of n7 (p = x * H + y).
 *     4. The positions sorted, H * W appended, their differences taken and every run of length 0 merged into its neighbours are
 *        the polygon's counts: pixel p is set when the number of toggles at positions <= p is odd.  A crossing clamped to yd == H
 *        stands at position (x + 1) * H, the first pixel of the next column: parity is carried from a column into the next one.
 *     The mask of an annotation is the OR of its polygons' masks; an annotation without polygons is empty.
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers.  Annotation i owns the polygons poly_ptr[i] .. poly_ptr[i + 1]), polygon q the vertices vert_ptr[q] ..
 * vert_ptr[q + 1]) (counted in vertices); xy holds two doubles per vertex, x then y.  Outputs exactly as mnc_mask_from_rle gives
 * them: bounds [n][4] the tight box of the set pixels (rleToBbox; an empty mask gets (0, 0, -1, -1), no rows and area 0),
 * offsets [n] (multiples of 8, in order without gaps), areas [n] (the true bit counts), the rows in bits (padding bits 0),
 * *bits_bytes = the bytes they take.  bits == NULL: bounds, offsets, areas and *bits_bytes only; bits_cap < *bits_bytes is
 * MNC_ERR_INVALID with *bits_bytes set.  n == 0 returns before any device work.
 * The host rounds the vertices and makes the table of edges with the prefix of their walk lengths (O(vertices)); one thread per
 * walk point forms its point and the one before it in closed form and XORs a crossing's bit into its polygon's toggle plane
 * (atomic XOR commutes: the same bits from run to run); one workgroup per annotation turns the toggles into pixels -- a running
 * XOR down every column plus the parity carried in from the columns to its left -- ORs the polygons together and reduces the
 * tight box and the area; the host forms the offsets; a last kernel shifts the rows into the box and writes every word once.
 * MNC_ERR_INVALID, checked on the host before anything is launched: n outside [0, 2048]; H or W outside [1, 32768] or
 * H * W > 2^30; a negative or decreasing poly_ptr or vert_ptr (vert_ptr has poly_ptr[n] + 1 entries); a polygon without
 * vertices; a coordinate that is NaN, infinite or of magnitude > 2^20; walks of more than 2^30 points in all. */
MNC_API int mnc_mask_from_polygons(const double* xy, const long long* vert_ptr, const long long* poly_ptr, int n, int H, int W,
                                   int* bounds, long long* offsets, long long* areas, void* bits, size_t bits_cap,
                                   size_t* bits_bytes, int device_id);
/* For tools/mask_poly_bench.py.  on = 1: the following mnc_mask_from_polygons calls put a HIP event pair around their fill and
 * launches (the plane fill, the toggle and fill kernels; the write kernel) and keep the sum of the last call, in milliseconds; on
 * = 0: they do not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is none;
 * switching on forgets it. */
MNC_API int mnc_mask_poly_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n10 Scoring a whole set: COCO's accumulate -- the match tables of n8 of all images turned into precision [T][R][K][A][M] and
 *     recall [T][K][A][M] (the published cocoeval.py:accumulate) -- in one call (csrc/coco_accum.hip).  The statement of the rule
 *     is mnc_amd/coco_eval.py:accumulate; mnc_amd/coco_eval.py:flatten_records makes the arguments.
 *     The image records flattened in image order, within an image in the caller's index order: N detections with dt_class_idx [N]
 *     (the index into the K evaluated classes, -1 for a class not evaluated), dt_score [N] float32, dt_rank [N] (the rank of n8),
 *     dt_flags [A][T][N] bytes (bit 0: dt_match >= 0, bit 1: dt_ignore != 0); Gn ground truths with gt_class_idx [Gn] (-1 alike)
 *     and gt_ignore [A][Gn] bytes 0 / 1; max_dets [M] (int), rec_thrs [R].
 *     npig[k][a] = the ground truths of class k with gt_ignore[a] == 0; a cell (k, a, m) with npig == 0 stays -1 everywhere.
 *     The list of cell (k, a, m): the detections with dt_class_idx == k and dt_rank < max_dets[m], by score descending, equal
 *     scores (-0.0 == +0.0) in the order given (np.argsort(-scores, kind="mergesort") over the images' concatenation).  Per
 *     threshold t along a list of nd entries: tp_i, fp_i the inclusive counts of flags == 1 (matched, not ignored) and flags == 0
 *     (not matched, not ignored); rc_i = (double)tp_i / (double)npig; pr_i = (double)tp_i / ((double)(fp_i + tp_i) + 2^-52);
 *     recall[t][k][a][m] = rc_{nd-1} (0 when nd == 0); precision[t][r][k][a][m] = max over j >= at_r of pr_j, at_r the first i
 *     with rc_i >= rec_thrs[r] (0 when there is none).  All arithmetic IEEE double in this order.
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers.  Outputs precision [T][R][K][A][M], recall [T][K][A][M], npig [K][A] (may be NULL).  One stable
 * least-significant-digit radix sort of all detections by (class, score descending) on the device (per pass: tile histograms, a
 * scan, a scatter ranked by wave ballots), the flag planes gathered into that order once, then one workgroup per (k, a, m, t)
 * over its class segment: a count, and a walk from the right with the carried maximum of pr.  Integer atomics only where the
 * result is a sum (histograms, npig), no floating-point atomics: the same bits from run to run, and the bits of the host rule.
 * N == 0 or Gn == 0 returns before any device work with the tables as the rule gives them (-1 where npig == 0, else 0).
 * MNC_ERR_INVALID, checked on the host before anything is launched: N or Gn outside [0, 2^24]; K outside [1, 4096]; T outside
 * [1, 16]; A outside [1, 8]; M outside [1, 8]; R outside [1, 1024]; a max_det outside [1, 2048]; a class index outside [-1, K);
 * a negative rank; a NaN score or recall threshold; a flag byte above 3; an ignore byte above 1; a NULL precision or recall (or
 * a NULL input that has entries). */
MNC_API int mnc_coco_accumulate(const int* dt_class_idx, const float* dt_score, const int* dt_rank, const unsigned char* dt_flags,
                                int N, const int* gt_class_idx, const unsigned char* gt_ignore, int Gn, int K, int T, int A,
                                const int* max_dets, int M, const double* rec_thrs, int R, double* precision, double* recall,
                                long long* npig, int device_id);
/* For tools/coco_accum_bench.py.  on = 1: the following mnc_coco_accumulate calls put a HIP event pair around their launches (from
 * the keys to the cells, without the copies) and keep the last call's time in milliseconds; on = 0: they do not (the default).
 * *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is none; switching on forgets it. */
MNC_API int mnc_coco_accum_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n11 Scoring the contours: the boundary bands of packed masks and COCO's matching on min(mask IoU, boundary IoU)
 *     (csrc/mask_boundary.hip, csrc/mask_match.hip) -- Boundary IoU (Cheng et al., CVPR 2021; iouType = "boundary" of the COCO
 *     toolkit, the measure of LVIS) on the layout of n5.  The statements of the rule are mnc_amd/boundary.py:boundary_numpy and
 *     mnc_amd/coco_eval.py:match_boundary_numpy.
 *     The distance is made on the host: d = max(1, (int)round(ratio * sqrt(H * H + W * W))), round half to even (Python 3's round
 *     of the double), ratio 0.02 by default (mnc_amd/boundary.py:boundary_distance; 375 x 500 gives 12, 600 x 1000 gives 23).
 *     The boundary of a mask M in an H x W image at distance d >= 1: M is first cropped to the image (bounds may leave it;
 *     padding bits are never trusted).  E = the pixels p of M for which every q with |qx - px| <= d and |qy - py| <= d lies
 *     inside the image and in M; B = M \ E.  This is the published mask_to_boundary: a one-pixel zero border, cv2.erode with a
 *     3 x 3 kernel of ones d times, the border removed, the difference.
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers.  The set as mnc_mask_rle takes it: bounds [n][4] int, offsets [n], bits, bytes = the bytes bits holds (the areas
 * are not needed).  The result has the layout of n5: instance i has the input bounds intersected with [0, W-1] x [0, H-1], not
 * tightened; an instance without rows or with an empty intersection gets (0, 0, -1, -1), no rows and area 0; out_offsets [n] are
 * multiples of 8, in order without gaps; out_areas [n] are the true bit counts of B; padding bits are 0.  out_bounds, out_offsets
 * and *bits_bytes follow from the bounds alone and are computed on the host before anything is launched: with out_bits == NULL the
 * call returns them and launches nothing (out_areas may be NULL then); bits_cap < *bits_bytes is MNC_ERR_INVALID with *bits_bytes
 * set.  n == 0 returns before any device work.
 * The erosion is separable.  One thread per output word erodes along the row -- in the word itself a log-step shift-OR of the
 * mask's zeros by min(d, 63), from each of the ceil(d / 64) words to either side the reach of its nearest zero, everything beyond
 * the row's ends counting as zero -- into a scratch plane in device memory; for d > 4 a second kernel turns blocks of 2d + 1 rows
 * of every word column into prefix and suffix ANDs, so that the last kernel reads two words per output word whatever d is (for
 * d <= 4 it reads the 2d + 1 rows themselves); it stores B = M & ~E, every word once (nothing is zeroed beforehand), and adds
 * the bit counts to the areas with integer atomics: the same bits from run to run.
 * MNC_ERR_INVALID, checked on the host before anything is launched: everything mnc_mask_rle refuses about a set (n outside
 * [0, 2048], |coordinate| >= 2^24, more than 2^26 pixels in one bound, an offset that is negative or not a multiple of 8, rows
 * that reach past bytes); H or W outside [1, 32768]; d outside [1, 1024]. */
MNC_API int mnc_mask_boundary(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int H, int W,
                              int d, int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits,
                              size_t bits_cap, size_t* bits_bytes, int device_id);
/* mnc_mask_match (n8; the same 23 inputs, the same five tables) on the overlap min(iou[d][g], biou[d][g]) in an H x W image at
 * distance d.  With Db, Gb the boundaries of the detections and of the ground truths as mnc_mask_boundary gives them, biou[d][g]
 * is iou exactly as n8 defines it, computed on (Db, Gb): inter the count of n6 on the two bands, union = area(Db[d]) +
 * area(Gb[g]) - inter, for a crowd ground truth area(Db[d]); union < 1 gives 0.0; (double)inter / (double)union.  Everything else
 * of the rule is n8's: ranks and class lists, the area-range rules on dt_areas and gt_eval_area (not on the bands' areas), the
 * min(thr, 1 - 1e-10) rule and the tie rules.  iou [nd][ng] (may be NULL) receives the minimum that was matched on, biou [nd][ng]
 * (may be NULL) the boundary IoU alone.  Both sets are uploaded once; both boundary sets are made on the device and never visit the
 * host; the counts of n6 run twice, on the masks and on the bands; then the lists and the cells of n8 run on the minimum.  nd == 0
 * or ng == 0 returns before any device work, as n8 does.  MNC_ERR_INVALID, checked on the host before anything is launched:
 * everything mnc_mask_match refuses, H or W outside [1, 32768], d outside [1, 1024].  (There is no form that reads a
 * device-resident result: PackedMasks.match_boundary fetches such a result first.) */
MNC_API int mnc_mask_match_boundary(const int* dt_bounds, const long long* dt_offsets, const long long* dt_areas, const void* dt_bits,
                                    size_t dt_bytes, int nd, const int* dt_classes, const float* dt_scores, const int* gt_bounds,
                                    const long long* gt_offsets, const long long* gt_areas, const void* gt_bits, size_t gt_bytes,
                                    int ng, const int* gt_classes, const unsigned char* gt_crowd, const unsigned char* gt_ignore_in,
                                    const double* gt_eval_area, const double* iou_thrs, int T, const double* area_rngs, int A,
                                    int max_det, int H, int W, int d, int* rank, int* dt_match, unsigned char* dt_ignore,
                                    int* gt_match, unsigned char* gt_ignore, double* iou, double* biou, int device_id);
/* For tools/mask_boundary_bench.py.  on = 1: the following mnc_mask_boundary and mnc_mask_match_boundary calls put a HIP event
 * pair around their launches (the boundary kernels; for the matching also the uploads of the ground truths, the fills, the counts
 * and the matching kernels) and keep the last call's time in milliseconds; on = 0: they do not (the default).  *last_ms (may be
 * NULL) receives the figure kept before this call, -1.0 when there is none; switching on forgets it. */
MNC_API int mnc_mask_boundary_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n12 The masks as shapes: connected components of packed masks, and what is built on them -- the component table, the
 *     selection by area, the filling of holes, one instance per region (csrc/mask_components.hip, csrc/mask_cc.h) -- on the
 *     layout of n5.  The statements of the rule are mnc_amd/components.py:components_numpy, select_numpy, fill_holes_numpy
 *     and split_numpy.
 *     A component of instance i is a maximal set of its set pixels connected under `connectivity` 4 (edge neighbours) or 8
 *     (edge and corner neighbours).  Padding bits are not trusted; pixels outside the instance's bounds are background; an
 *     instance without rows has no components.  The components of an instance are numbered by their first pixel in row-major
 *     order (lowest y, then lowest x: scipy.ndimage.label's numbering); the components of a set are those of instance 0, then
 *     of instance 1, ...: comp_ptr [n + 1], comp_ptr[0] = 0, instance i has the components comp_ptr[i] .. comp_ptr[i + 1] - 1.
 *     Runs are labelled, not pixels.  Per 64-bit word the run starts are v & ~((v << 1) | carry), a scan of their counts over
 *     the words of the set numbers the runs in raster order; one thread per word unites its runs with the runs of the row
 *     above that they touch, in a lock-free union-find whose smaller id always becomes the parent (parent[i] <= i at every
 *     moment, so every find ends whatever the interleaving); a run is a root when it is its own parent, a scan of the root
 *     flags numbers the components in first-pixel order.  Integer atomics only (min, max, add, compare-and-swap); no output
 *     depends on the order in which they arrive: the same input gives the same bytes on every run.
 *     Every entry takes the set as mnc_mask_rle takes it: bounds [n][4] int, offsets [n], bits, bytes = the bytes bits holds
 *     (the areas are not needed).  n == 0 and sets without a single row are answered on the host.  MNC_ERR_INVALID, checked on
 *     the host before anything is launched, for every entry: connectivity not 4 or 8; everything mnc_mask_rle refuses about a
 *     set (n outside [0, 2048], |coordinate| >= 2^24, more than 2^26 pixels in one bound, an offset that is negative or not a
 *     multiple of 8, rows that reach past bytes); more than 2^25 words (256 MiB) of rows in the set, for mnc_mask_fill_holes
 *     counted on the boxes grown by one pixel on every side (a word holds at most 32 runs: run ids stay below 2^30); a null
 *     pointer where one is needed.  (There are no forms that read a device-resident mnc_mask_records result: the PackedMasks
 *     methods fetch such a result first.)
 * ------------------------------------------------------------------------------------------------------------- */
/* The component table.  Outputs: comp_ptr [n + 1], *n_comp = C = comp_ptr[n]; per component area [C] (pixels), bbox [C][4]
 * (x1, y1, x2, y2 in image coordinates, inclusive and tight), anchor [C][2] (x, y of its first pixel).  area == NULL: comp_ptr
 * and *n_comp only (bbox and anchor are not looked at).  Otherwise comp_cap is the room of area, bbox and anchor in components;
 * comp_cap < C is MNC_ERR_INVALID with comp_ptr and *n_comp set and nothing else written, so that the caller calls again with
 * room.  Entries past C are never written. */
MNC_API int mnc_mask_components(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
                                long long* comp_ptr, long long* area, int* bbox, int* anchor, size_t comp_cap, size_t* n_comp,
                                int device_id);
/* The selection.  A component stays when its area is >= min_area and, with keep > 0, it is among the keep largest of its
 * instance (larger area first, equal areas to the lower component number).  The result has the input's bounds and offsets:
 * out_bits receives the words of every instance at the input's offsets (every word of every row once, padding bits 0; bytes
 * between and behind the rows are not written), out_areas [n] the true bit counts.  bits_cap below the bytes the rows reach is
 * MNC_ERR_INVALID.  min_area = 1, keep = 0 gives the input with its padding cleared.  MNC_ERR_INVALID as above, and: a negative
 * min_area or keep; rows of two instances that overlap or stand out of order (offsets[i] below the end of the rows before). */
MNC_API int mnc_mask_select(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
                            int min_area, int keep, long long* out_areas, void* out_bits, size_t bits_cap, int device_id);
/* The filling of holes.  `connectivity` is that of the background.  A hole of instance i is a component of the unset pixels of
 * its box that is not connected to the outside of the box: the labelling above on the complement of the box grown by a frame of
 * one background pixel, every component but the frame's.  The result is the mask OR its holes, in the layout and under the
 * rules of mnc_mask_select (scipy.ndimage.binary_fill_holes with the 4- or 8-neighbour structure). */
MNC_API int mnc_mask_fill_holes(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
                                long long* out_areas, void* out_bits, size_t bits_cap, int device_id);
/* One instance per component, in component order: out_bounds [C][4] the tight boxes, out_offsets [C] (multiples of 8, in order
 * without gaps), out_areas [C], out_source [C] (the instance the component came from), the rows in out_bits (padding bits 0),
 * *n_comp = C, *bits_bytes = the bytes of the rows.  out_bits == NULL: *n_comp and *bits_bytes only.  Otherwise comp_cap < C or
 * bits_cap < *bits_bytes is MNC_ERR_INVALID with both sizes set and nothing else written.  Entries and bytes past the reported
 * sizes are never written.  Also MNC_ERR_INVALID, after the table pass: more than 2^31 words of rows in the result. */
MNC_API int mnc_mask_split(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
                           int* out_bounds, long long* out_offsets, long long* out_areas, int* out_source, size_t comp_cap,
                           size_t* n_comp, void* out_bits, size_t bits_cap, size_t* bits_bytes, int device_id);
/* For tools/mask_components_bench.py.  on = 1: the following calls of the four entries above put a HIP event pair around their
 * launches (with the read-back of the run total between them, without the copies of the set and of the results) and keep the
 * last call's time in milliseconds; on = 0: they do not (the default).  *last_ms (may be NULL) receives the figure kept before
 * this call, -1.0 when there is none; switching on forgets it. */
MNC_API int mnc_mask_components_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n13 The masks as outlines: the boundary of every instance of a packed set as closed rectilinear polygons
 *     (csrc/mask_contours.hip, csrc/mask_contour.h) -- on the layout of n5.  The statement of the rule is
 *     mnc_amd/contours.py:contours_numpy.
 *     Pixel (x, y) of the image is the unit square [x, x + 1] x [y, y + 1]; vertices are lattice points in image coordinates
 *     (the instance's bounds added in), int32.  A boundary edge is a unit side between a set pixel of instance i and an unset
 *     one; pixels outside the instance's bounds are unset, padding bits are not trusted.  An edge is directed so that the set
 *     pixel is on its right, y pointing down: the top side runs +x, the right side +y, the bottom side -x, the left side -y.
 *     Outer boundaries then run clockwise on screen and holes the other way.  The successor of an edge is the boundary edge
 *     that leaves its head vertex.  Two leave only where two set pixels touch at a corner alone: there connectivity = 8 takes
 *     the left turn, so that the two pixels share one loop, and connectivity = 4 the right turn, so that each keeps its own.
 *     The successor relation is a permutation of the edges; its cycles are the loops.
 *     The vertices of a loop are the tails of those of its edges whose predecessor has another direction: consecutive
 *     vertices differ in exactly one coordinate, horizontal and vertical sides alternate, no three consecutive vertices are
 *     collinear.  The list starts at the loop's smallest vertex in (y, x) order and follows the direction of travel; the
 *     first vertex is not repeated at the end.  A loop passes through that start vertex once, and it is the start of at most
 *     one loop.  A loop is a hole exactly when its first side runs +y.  The loops of an instance are ordered by their start
 *     vertex (y, x); the loops of a set are those of instance 0, then of instance 1, ...: loop_ptr [n + 1], loop_ptr[0] = 0,
 *     instance i has the loops loop_ptr[i] .. loop_ptr[i + 1] - 1; loop l has the vertices vert_ptr[l] .. vert_ptr[l + 1] - 1
 *     of xy.  An instance without rows or without a set pixel has no loops.  area[l] is the signed shoelace area of loop l,
 *     exact: positive for an outer loop, negative for a hole; the areas of an instance's loops sum to its pixel count.
 *     (A rectilinear polygon on lattice points is rasterised exactly by n10's rule: the XOR of the loops of an instance,
 *     rasterised one by one, is the instance.)
 *     Edges are numbered, not pixels.  The four masks of the edges that leave the 64 lattice points of a word are bit
 *     expressions of the pixel words above and below and their carries; a scan of their counts numbers the edges in the order
 *     instance, tail y, tail x, direction, so the smallest id of a cycle is the edge that leaves the loop's start vertex and a
 *     scan of the leader flags numbers the loops in the order above.  The leaders are found by pointer jumping with a running
 *     minimum and the vertex slots by Wyllie's list ranking of the cycles cut in front of their leaders, ceil(log2(E)) rounds
 *     each for E edges, every round a launch of its own from one pair of buffers into the other.  Integer atomics only (the
 *     64-bit adds of the areas); every other slot is written once: the same input gives the same bytes on every run.
 * ------------------------------------------------------------------------------------------------------------- */
/* The set as mnc_mask_rle takes it: bounds [n][4] int, offsets [n], bits, bytes = the bytes bits holds.  Outputs: loop_ptr
 * [n + 1], *n_loops = L = loop_ptr[n], *n_verts = V; vert_ptr [L + 1] (vert_ptr[L] = V), area [L], xy [V][2] (x, y).
 * xy == NULL: loop_ptr and the two sizes only (vert_ptr and area are not looked at).  Otherwise loop_cap is the room of area
 * in loops (vert_ptr has room for loop_cap + 1 entries) and vert_cap the room of xy in vertices; loop_cap < L or vert_cap < V
 * is MNC_ERR_INVALID with loop_ptr and the two sizes set and nothing else written, so that the caller calls again with room.
 * Entries past the reported sizes are never written.  n == 0 and sets without a single row are answered on the host.
 * MNC_ERR_INVALID, checked on the host before anything is launched: connectivity not 4 or 8; everything mnc_mask_rle refuses
 * about a set; more than 2^25 words of rows in the set, counted on the lattice points ((h + 1) rows of ceil((w + 1) / 64)
 * words per instance); a null pointer where one is needed.  MNC_ERR_INVALID after the counting pass: more than 2^30 boundary
 * edges in the set.  (There is no form that reads a device-resident mnc_mask_records result: the PackedMasks method fetches
 * such a result first.) */
MNC_API int mnc_mask_contours(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
                              long long* loop_ptr, long long* vert_ptr, long long* area, int* xy, size_t loop_cap, size_t vert_cap,
                              size_t* n_loops, size_t* n_verts, int device_id);
/* For tools/mask_contours_bench.py.  on = 1: the following calls of mnc_mask_contours put a HIP event pair around their launches
 * (with the read-backs of the totals between them, without the copies of the results) and keep the last call's time in
 * milliseconds; on = 0: they do not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when
 * there is none; switching on forgets it. */
MNC_API int mnc_mask_contours_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n14 Outlines simplified to a pixel tolerance: Douglas-Peucker on closed loops in exact integer arithmetic
 *     (csrc/contour_simplify.hip), so that the parallel form equals a sequential one bit for bit.  The statement of the rule
 *     is mnc_amd/contours.py:simplify_numpy.
 *     Input: loops as n13 gives them (vert_ptr, xy int32) -- any closed integer loops, not only rectilinear ones; the first
 *     vertex is not repeated.  The tolerance is q sixteenths of a pixel (the host quantises: q = round-half-even(16 epsilon)).
 *     A loop v_0 .. v_(k-1), v_k = v_0, of k <= 3 vertices is unchanged.  Otherwise the anchors are index 0 and B, the index in
 *     1 .. k - 1 with the largest |v_B - v_0|^2 (the lowest on ties), and the two chains are (0, B) and (B, k).
 *     The deviation of m in the segment (i, j), i < m < j, with a = v_i, b = v_(j mod k), p = v_m, ab = b - a, ap = p - a,
 *     L = ab.ab and t = ap.ab, is the pair (N, D): L == 0 gives (|ap|^2, 1); t <= 0 gives (|ap|^2 L, L); t >= L gives
 *     (|p - b|^2 L, L); otherwise ((ab x ap)^2, L).  N / D is the squared distance of p from the segment; D is common to the
 *     segment.  split(i, j) does nothing when j - i < 2; else m* is the m with the largest N (the lowest on ties), and if
 *     256 N > q^2 D, m* is kept and split(i, m*) and split(m*, j) follow.  Both chains are split.  If neither keeps a vertex
 *     (only 0 and B are kept), the third anchor applies: the m with the largest N over both chains -- they share L -- is kept
 *     whatever q is (the lowest index on ties), and the two halves of its chain are split.  So a closed loop never comes out
 *     with fewer than three vertices.  The output is the kept vertices in index order; v_0 is always first; loops are never
 *     dropped.  Like every plain Douglas-Peucker the rule does not preserve topology: a simplified loop may touch or cross
 *     itself or another one.
 *     Coordinates are accepted in [-2^24, 2^24]: ab x ap is below 2^51 in size, N below 2^102, 256 N and q^2 D below 2^110.
 *     The device works in 128-bit integers; there is no floating point.  A decision is a pure function of its segment's
 *     vertices, so the segments may be taken in any order: loops of at most 64 vertices go one per wave, longer ones one per
 *     workgroup (staged in LDS up to 4096 vertices) whose rounds over a double-buffered list of open segments run inside the
 *     one launch; only the kept flags leave those kernels, a scan in index order places the vertices.  One memset and five
 *     launches whatever the data, one read-back of V': the same input gives the same bytes on every run.
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers.  vert_ptr [n_loops + 1], xy [n_verts][2] (x, y).  Outputs: out_vert_ptr [n_loops + 1], *out_verts = V' =
 * out_vert_ptr[n_loops]; out_xy [V'][2] the kept vertices, out_index [V'] their positions in xy.  out_xy and out_index have room
 * for n_verts vertices (V' <= n_verts): there is no second call.  Entries past n_loops + 1 of out_vert_ptr and past V' of out_xy and
 * out_index are never written.  n_loops == 0 or n_verts == 0 is answered on the host.  MNC_ERR_INVALID, checked on the host before
 * anything is launched and with nothing written: q outside [0, 2^20]; n_loops > 2^24 or n_verts > 2^27; a null pointer where one
 * is needed (xy, out_xy and out_index may be null when n_verts == 0); a vert_ptr that does not start at 0, decreases, or does not
 * end at n_verts; a coordinate outside [-2^24, 2^24]. */
MNC_API int mnc_contours_simplify(const long long* vert_ptr, const int* xy, size_t n_loops, size_t n_verts, int q,
                                  long long* out_vert_ptr, int* out_xy, long long* out_index, size_t* out_verts, int device_id);
/* For tools/contours_simplify_bench.py.  on = 1: the following calls of mnc_contours_simplify put a HIP event pair around their
 * launches (without the copies of the loops and of the result and without the read-back of V') and keep the last call's time in
 * milliseconds; on = 0: they do not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when
 * there is none; switching on forgets it. */
MNC_API int mnc_contours_simplify_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n15 The masks as distances: the squared Euclidean distance transform of packed masks, the largest inscribed disc, and
 *     erosion, dilation, opening and closing by a disc (csrc/mask_distance.hip) -- on the layout of n5.  The statements of the
 *     rules are mnc_amd/distance.py:distance_numpy, inscribed_numpy and morph_numpy.
 *     All arithmetic is integer and all rules are frame-free: a mask M is a set of lattice pixels that is empty outside its
 *     bounds (padding bits are not trusted); the image size enters only as an optional final clip of the dilation.
 *     Inside distance: D(p) = min |p - q|^2 over all pixels q not in M, pixels beyond the bounds included, for p in M; D(p) = 0
 *     for p not in M.  (scipy.ndimage.distance_transform_edt of the mask padded by one pixel of zeros, squared.)  D <=
 *     ((min(w, h) + 1) / 2)^2.
 *     Inscribed disc: per instance the pixel of maximal D, the lowest (y, x) on ties, and that D.
 *     Disc morphology: the structuring element of squared radius R2 >= 0 is {(dx, dy): dx^2 + dy^2 <= R2}, rho = isqrt(R2).
 *     erode keeps p iff D(p) > R2.  dilate sets p iff some pixel of M lies within R2 -- the same transform on the complement,
 *     in the bounds grown by rho on every side, beyond which nothing is set.  open = dilate(erode), close = erode(dilate) with
 *     the erosion taken in the unclipped grown frame.  Opening and closing never leave the input's bounds.
 *     Two passes per transform.  The first gives every pixel g, the distance along its row to the nearest pixel outside the set
 *     (count-leading / -trailing-zero walks over the packed words, cut off at a cap that no reader can mistake: rho + 1 for the
 *     morphology, (min(w, h) + 1) / 2 + 1 for the maps), as uint16; the second, one lane per pixel, takes min(g^2 + dy^2) over
 *     the rows y +- dy while dy^2 is below the best so far (for the morphology: dy <= rho, and until the decision is made) and
 *     writes the distance, or one ballot word per wave with its popcount added to the area, or joins a 64-bit integer maximum
 *     of (D << 32) | (0xffffffff - linear index).  2 launches (4 for open and close) whatever the data, no read-back between
 *     them; integer atomics only: the same input gives the same bytes on every run.
 *     Every entry takes the set as mnc_mask_rle takes it: bounds [n][4] int, offsets [n], bits, bytes = the bytes bits holds.
 *     n == 0 and sets without a single row are answered on the host.  MNC_ERR_INVALID, checked on the host before anything is
 *     launched, for every entry: everything mnc_mask_boundary refuses about a set (n outside [0, 2048], |coordinate| >= 2^24,
 *     more than 2^26 pixels in one bound, an offset that is negative or not a multiple of 8, rows that reach past bytes); more
 *     than 2^27 pixels of rows in the call; a null pointer where one is needed.  (There are no forms that read a
 *     device-resident mnc_mask_records result: the PackedMasks methods fetch such a result first.)
 * ------------------------------------------------------------------------------------------------------------- */
/* The maps.  Outputs: dist_ptr [n + 1] (dist_ptr[0] = 0; instance i has the h * w entries dist_ptr[i] .. dist_ptr[i + 1] - 1,
 * row-major with row stride w; none without rows), *dist_total = dist_ptr[n], dist [*dist_total] the D of every pixel.
 * dist == NULL: dist_ptr and *dist_total only, nothing is launched.  Otherwise dist_cap is the room of dist in entries;
 * dist_cap < *dist_total is MNC_ERR_INVALID with dist_ptr and *dist_total set and nothing else written.  Entries past
 * *dist_total are never written. */
MNC_API int mnc_mask_distance(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n,
                              long long* dist_ptr, unsigned* dist, size_t dist_cap, size_t* dist_total, int device_id);
/* The inscribed discs.  Outputs: xy [n][2] (x, y of the pixel in image coordinates: bounds x1 + dx, bounds y1 + dy), r2 [n] its
 * D.  An instance without rows or without a set pixel gives (-1, -1) and 0. */
MNC_API int mnc_mask_inscribed(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int* xy, int* r2,
                               int device_id);
/* The morphology.  op: 0 erode, 1 dilate, 2 open, 3 close; r2 = R2; H, W both 0: no clip, else the image the dilation's bounds
 * are intersected with (looked at by op 1 only).  The result has the layout of n5 as mnc_mask_boundary writes it: out_offsets
 * [n] are multiples of 8, in order without gaps; out_areas [n] are the true bit counts; padding bits are 0.  erode, open and
 * close keep the input's bounds (an instance without rows keeps them and gets no rows).  dilate gives (x1 - rho, y1 - rho,
 * x2 + rho, y2 + rho), not tightened; with H, W these intersected with [0, W-1] x [0, H-1], (0, 0, -1, -1) where nothing is left
 * or where the instance had no rows (without H, W an instance without rows keeps its bounds).  out_bounds, out_offsets and
 * *bits_bytes follow from the bounds alone and are computed on the host: with out_bits == NULL the call returns them and
 * launches nothing (out_areas may be NULL then); bits_cap < *bits_bytes is MNC_ERR_INVALID with the three set and nothing else
 * written.  Bytes past *bits_bytes are never written.  MNC_ERR_INVALID as above, with nothing written, and: op outside [0, 3];
 * r2 outside [0, 1024^2]; H and W neither both 0 nor both in [1, 32768]; for dilate and close, whose frames are the bounds grown
 * by rho: a grown coordinate with |c| >= 2^24, a grown instance of more than 2^26 pixels, more than 2^27 pixels of grown rows
 * in the call. */
MNC_API int mnc_mask_morph(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int op, int r2,
                           int H, int W, int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits,
                           size_t bits_cap, size_t* bits_bytes, int device_id);
/* For tools/mask_distance_bench.py.  on = 1: the following calls of the three entries above put a HIP event pair around their
 * launches (without the copies of the set and of the results) and keep the last call's time in milliseconds; on = 0: they do
 * not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is none; switching on
 * forgets it. */
MNC_API int mnc_mask_distance_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n16 The masks as shapes: the moments of order up to two, the convex hull, the rectangle of least area and the diameter
 *     of packed masks (csrc/mask_shape.hip) -- on the layout of n5.  The statements of the rules are
 *     mnc_amd/shape.py:moments_numpy, hull_numpy and oriented_numpy.  Every result is an integer; the floats a caller wants
 *     (centroid, axes, corners, angle) follow from them on the host.
 *     Moments: m_pq = sum of x^p y^q over the set pixels, x and y the pixel's column and row relative to the bounds' (x1, y1);
 *     six sums per instance in the order m00, m10, m01, m20, m11, m02, each below 2^56.  Padding bits are not counted.
 *     Hull: the convex hull of the union of the closed unit squares [x, x + 1] x [y, y + 1] of the set pixels.  Vertices are
 *     lattice points in image coordinates with n13's conventions: clockwise on screen (the set on the right of every edge, y
 *     pointing down), from the smallest vertex in (y, x) order on, no three consecutive vertices collinear, the first not
 *     repeated.  area2 is twice the shoelace area.  The candidates are, per lattice row Y, the least first set column and the
 *     greatest (last set column + 1) over the pixel rows Y - 1 and Y; a candidate is a vertex exactly when its extreme tangents
 *     to the candidates above and below make a strictly convex angle, which every candidate decides by itself.
 *     Rectangle of least area: for hull edge k with tail a and vector e, over the hull vertices p, t = (p - a) . e and s =
 *     ex (p_y - a_y) - ey (p_x - a_x) >= 0; the rectangle on the edge has the area (tmax - tmin) smax / |e|^2 (numerator below
 *     2^64, denominator below 2^32); the least wins, compared by cross-multiplication in 128 bits, the lowest k on ties.
 *     Diameter: the greatest squared distance between two hull vertices i < j, the lexicographically lowest pair on ties.
 *     An instance without rows or without a set pixel gives zeros and no vertices.
 *     Every entry takes the set as mnc_mask_rle takes it: bounds [n][4] int, offsets [n], bits, bytes = the bytes bits holds.
 *     n == 0 and sets without a single row are answered on the host.  MNC_ERR_INVALID, checked on the host before anything is
 *     launched and with nothing written: everything mnc_mask_boundary refuses about a set (n outside [0, 2048], |coordinate|
 *     >= 2^24, more than 2^26 pixels in one bound, an offset that is negative or not a multiple of 8, rows that reach past
 *     bytes); a bound wider or taller than 32768; a null pointer where one is needed.  The launch counts do not depend on the
 *     data; the only atomics are the 64-bit integer adds of the moments: the same input gives the same bytes on every run.
 *     (There are no forms that read a device-resident mnc_mask_records result: the PackedMasks methods fetch such a result
 *     first.)
 * ------------------------------------------------------------------------------------------------------------- */
/* moments [n][6]. */
MNC_API int mnc_mask_moments(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, long long* moments,
                             int device_id);
/* Outputs: vert_ptr [n + 1] (vert_ptr[0] = 0; instance i has the vertices vert_ptr[i] .. vert_ptr[i + 1] - 1), *n_verts = V =
 * vert_ptr[n]; xy [V][2] (x, y), area2 [n].  xy == NULL: vert_ptr and *n_verts only (area2 is not looked at).  Otherwise vert_cap
 * is the room of xy in vertices; vert_cap < V is MNC_ERR_INVALID with vert_ptr and *n_verts set and nothing else written, so that
 * the caller calls again with room.  Entries past V are never written. */
MNC_API int mnc_mask_hull(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, long long* vert_ptr,
                          int* xy, long long* area2, size_t vert_cap, size_t* n_verts, int device_id);
/* Hull and calipers in one call; the hull's vertices do not come to the host.  box [n][8] = (k, ax, ay, ex, ey, tmin, tmax, smax)
 * with a in image coordinates and k the edge's index in the hull mnc_mask_hull gives; diameter [n][3] = (d2, i, j). */
MNC_API int mnc_mask_oriented(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, long long* box,
                              long long* diameter, int device_id);
/* For tools/mask_shape_bench.py.  on = 1: the following calls of the three entries above put a HIP event pair around their
 * launches (without the copies of the set and of the results) and keep the last call's time in milliseconds; on = 0: they do
 * not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is none; switching on
 * forgets it. */
MNC_API int mnc_mask_shape_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n17 The set algebra of packed masks: and, or, xor, minus, copy and complement of two sets instance by instance, the union
 *     or intersection of groups of instances, and the layering of a set into disjoint instances (csrc/mask_algebra.hip) --
 *     on the layout of n5.  The statements of the rules are mnc_amd/algebra.py:combine_numpy, merge_numpy and layer_numpy.
 *     Frame-free integer set arithmetic on lattice pixels: a mask is empty outside its bounds, bounds may be negative or
 *     unclipped, input padding bits are not trusted.
 *     Every result has the layout of n5 as mnc_mask_boundary writes it -- out_offsets are multiples of 8, in order without
 *     gaps; out_areas are the true bit counts; padding bits are 0 -- and TIGHT bounds: the smallest box that holds the
 *     instance's set pixels; an instance without a set pixel gets (0, 0, -1, -1) and no rows.
 *     The size of a result depends on the data; an upper bound, *bits_bound, depends on the bounds alone: the bytes of the
 *     LOOSE FRAMES.  The loose frame of an output instance is the intersection of the operands' bounds (and; an intersecting
 *     merge), the hull of the bounds of the operands that have rows (or, xor; a uniting merge), a's own bounds (minus, copy,
 *     layer) or the window (not), each intersected with the window where one is given.
 *     Protocol, alike for the three entries: out_bits == NULL sets *bits_bound on the host and launches nothing (the other
 *     outputs are not looked at); with bits_cap >= *bits_bound one call writes the tight result and sets *bits_bytes (and
 *     *bits_bound); a smaller bits_cap is MNC_ERR_INVALID with only *bits_bound set.  Bytes past *bits_bytes are never written.
 *     Three passes, five launches whatever the data, nothing read back in between: every lane forms a result word of the
 *     loose frame from funnel-shifted reads of the operands' rows and the wave joins an integer min / max of the non-zero
 *     rows and bit columns per instance; the extents become the result's table and a prefix sum places the offsets; one lane
 *     per word of the tight frame evaluates the same expression again, writes its word once and the wave adds its popcount
 *     to the area.  No floating point; integer atomics only: the same input gives the same bytes on every run.
 *     Every entry takes a set as mnc_mask_rle takes it: bounds [n][4] int, offsets [n], bits, bytes = the bytes bits holds.
 *     n == 0, G == 0 and calls whose loose frames have no row are answered on the host.  MNC_ERR_INVALID, checked on the
 *     host before anything is launched and with nothing written: everything mnc_mask_boundary refuses about a set (n outside
 *     [0, 2048], |coordinate| >= 2^24, more than 2^26 pixels in one bound, an offset that is negative or not a multiple of
 *     8, rows that reach past bytes); more than 2^27 pixels of loose-frame rows in the call; a null pointer where one is
 *     needed; and what the entries name below.  (There are no forms that read a device-resident mnc_mask_records result: the
 *     PackedMasks methods fetch such a result first.)
 * ------------------------------------------------------------------------------------------------------------- */
/* Instance i of a with instance i of b (n_b == n_a) or with b's only instance (n_b == 1); n_b == 0: no b (its other arguments
 * are not looked at).  op: 0 and, 1 or, 2 xor, 3 minus (a & ~b), 4 copy (a alone: tightens, or crops to the window), 5 not (the
 * complement of a inside the window).  window: NULL or (x1, y1, x2, y2) inclusive, which the result is intersected with before
 * it is tightened.  Outputs: out_bounds [n_a][4], out_offsets [n_a], out_areas [n_a], out_bits.  MNC_ERR_INVALID as above, and:
 * op outside [0, 5]; n_b outside {0, 1, n_a}; op 0 .. 3 with n_b == 0 (and n_a > 0); op 5 without a window; a window coordinate
 * with |c| >= 2^24; a window with x2 < x1 or y2 < y1. */
MNC_API int mnc_mask_combine(const int* a_bounds, const long long* a_offsets, const void* a_bits, size_t a_bytes, int n_a,
                             const int* b_bounds, const long long* b_offsets, const void* b_bits, size_t b_bytes, int n_b, int op,
                             const int* window, int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits,
                             size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id);
/* One result instance per group g: the union (intersect == 0) or the intersection of the instances members[group_ptr[g] ..
 * group_ptr[g + 1] - 1], indices into the set in any order, repeats allowed; a group without members gives an instance
 * without a pixel either way.  Outputs [G].  MNC_ERR_INVALID as above, and: G outside [0, 2048]; group_ptr[0] != 0 or group_ptr
 * not monotone; more than 2^20 members; a member outside [0, n - 1]. */
MNC_API int mnc_mask_merge(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n,
                           const long long* group_ptr, const int* members, int G, int intersect, int* out_bounds,
                           long long* out_offsets, long long* out_areas, void* out_bits, size_t bits_cap, size_t* bits_bound,
                           size_t* bits_bytes, int device_id);
/* Instance i minus the union of every instance before it in the order: pairwise disjoint instances with the same union, in
 * input index order.  order [n]: a permutation of 0 .. n - 1, first the instance that keeps all its pixels; NULL: by scores [n]
 * descending, the lower index first on equal scores (mnc_mask_nms's order; scores is not looked at when order is given).
 * Outputs [n].  The earlier instances whose bounds meet instance i's are listed on the host and uploaded with the set.
 * MNC_ERR_INVALID as above, and: order that is not a permutation; neither order nor scores; a NaN score when the order comes
 * from the scores. */
MNC_API int mnc_mask_layer(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const float* scores,
                           const int* order, int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits,
                           size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id);
/* For tools/mask_algebra_bench.py.  on = 1: the following calls of the three entries above put a HIP event pair around their
 * launches (without the copies of the set and of the results) and keep the last call's time in milliseconds; on = 0: they do
 * not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is none; switching on
 * forgets it. */
MNC_API int mnc_mask_algebra_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n18 Geometric transforms of packed masks: the eight lattice isometries plus a translation -- flips, the transpose, the
 *     rotations by quarter turns -- and the nearest-neighbour gather through an integer affine inverse map -- resize, rotate,
 *     shear (csrc/mask_warp.hip) -- on the layout of n5.  The statements of the rules are mnc_amd/warp.py:isometry_numpy and
 *     warp_numpy.  Frame-free integer arithmetic on lattice pixels: a mask is empty outside its bounds, bounds may be negative
 *     or unclipped, input padding bits are not trusted.  Output instance i is the image of input instance i.
 *     Every result has the layout and the TIGHT bounds of n17: out_offsets multiples of 8, in order without gaps; out_areas
 *     the true bit counts; padding bits 0; (0, 0, -1, -1) and no rows for an instance without a set pixel.
 *     The protocol is n17's, unchanged: out_bits == NULL sets *bits_bound -- the bytes of the LOOSE FRAMES, which follow from
 *     the bounds, the map and the window alone -- on the host and launches nothing; with bits_cap >= *bits_bound one call
 *     writes the tight result and sets *bits_bytes; a smaller bits_cap is MNC_ERR_INVALID with only *bits_bound set.  Bytes
 *     past *bits_bytes are never written.
 *     Three passes, five launches whatever the data, nothing read back in between: a wave forms a 64 x 64 bit block of the
 *     loose frame and joins an integer min / max of its non-zero rows and bit columns per instance; the extents become the
 *     result's table and a prefix sum places the offsets; a wave per block of the tight frame evaluates the same expression
 *     again, writes each word once and adds its popcount to the area.  No floating point; integer atomics only: the same
 *     input gives the same bytes on every run.
 *     n == 0 and calls whose loose frames have no row are answered on the host.  MNC_ERR_INVALID, checked on the host before
 *     anything is launched and with nothing written: everything mnc_mask_combine refuses about a set; more than 2^27 pixels
 *     of loose-frame rows in the call; a null pointer where one is needed; and what the entries name below.  (There are no
 *     forms that read a device-resident mnc_mask_records result: the PackedMasks methods fetch such a result first.)
 * ------------------------------------------------------------------------------------------------------------- */
/* A set pixel (x, y) goes to (x', y'):  (u, v) = (y, x) if code & 1, else (x, y);  u = -u if code & 2;  v = -v if code & 4;
 * (x', y') = (u + tx, v + ty).  In an H x W image np.fliplr is (2, W - 1, 0), np.flipud (4, 0, H - 1), the transpose (1, 0, 0),
 * np.rot90 by k = 1, 2, 3 quarter turns (5, 0, W - 1), (6, W - 1, H - 1), (3, H - 1, 0).  The loose frame of an instance is the
 * image of its bounds.  Codes without bit 0 read each result word from one funnel-shifted (and bit-reversed) word of a source
 * row; codes with bit 0 transpose 64 x 64 bit blocks with ballots.  Outputs [n].  MNC_ERR_INVALID as above, and: code outside
 * [0, 7]; |tx| or |ty| >= 2^24; a coordinate of the image of an instance's bounds with |c| >= 2^24. */
MNC_API int mnc_mask_isometry(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int code, int tx,
                              int ty, int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits,
                              size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id);
/* Destination pixel (x, y) inside window = (x1, y1, x2, y2), inclusive, is set iff source pixel (sx, sy) is set in the
 * instance: sx = floor((coef[0] x + coef[1] y + coef[2]) / den), sy = floor((coef[3] x + coef[4] y + coef[5]) / den), the floor
 * towards minus infinity, the numerators in int64.  One denominator serves both axes: a map whose axes have denominators of
 * their own (the centre-aligned resize, sx = floor((2x + 1) W / (2 W2)), sy = floor((2y + 1) H / (2 H2))) is brought to one by
 * cross-multiplying, coef = (4 W H2, 0, 2 W H2, 0, 4 H W2, 2 H W2) over den = 4 W2 H2, which a common factor may be divided out
 * of (mnc_amd/warp.py:resize_map).  The loose frame of an instance is the box, floor of the least and ceiling of the greatest
 * coordinate, of the parallelogram x1 den <= coef[0] x + coef[1] y + coef[2] <= (x2 + 1) den - 1 (alike in y) of destination
 * pixels whose source lies in its bounds (x1, y1, x2, y2) -- its corners solved exactly as rationals over det = coef[0] coef[4]
 * - coef[1] coef[3] in 128-bit integers -- intersected with the window.  Outputs [n].  MNC_ERR_INVALID as above, and: den outside
 * [1, 2^32]; |coef[0]|, |coef[1]|, |coef[3]| or |coef[4]| > 2^32; |coef[2]| or |coef[5]| > 2^60 (every numerator stays below
 * 2^62); det == 0; a window coordinate with |c| >= 2^24; a window with x2 < x1 or y2 < y1. */
MNC_API int mnc_mask_warp(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const long long* coef,
                          long long den, const int* window, int* out_bounds, long long* out_offsets, long long* out_areas,
                          void* out_bits, size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id);
/* For tools/mask_warp_bench.py.  on = 1: the following calls of the two entries above put a HIP event pair around their
 * launches (without the copies of the set and of the results) and keep the last call's time in milliseconds; on = 0: they do
 * not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is none; switching on
 * forgets it. */
MNC_API int mnc_mask_warp_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n19 Label maps in and out of packed masks: the instances of an integer label map -- SBD's inst / cls arrays, Cityscapes'
 *     instanceIds, the ids of a COCO panoptic PNG, a superpixel map -- as a set in the layout of n5, and the label map of a
 *     set (csrc/mask_labels.hip).  The statements of the rules are mnc_amd/labels.py:from_labels_numpy and to_labels_numpy.
 *     Integer arithmetic only; integer atomics only (or, min, max, add), all of which commute: the same input gives the same
 *     bytes on every run.  A label map is int [H][W], row-major, with H and W in [1, 32768] and H * W <= 2^26.
 *     From a map, two calls: mnc_label_table gives the instances -- the distinct values that are not skipped, ascending --
 *     with their tight boxes, pixel counts and the bytes of their rows; mnc_label_masks, with room for those bytes, writes the
 *     rows (offsets in order without gaps, as the host derives them from the boxes; padding bits 0).  Each call uploads the
 *     map.  MNC_ERR_INVALID is checked on the host before anything is launched, with nothing written, except where an entry
 *     says otherwise.
 * ------------------------------------------------------------------------------------------------------------- */
/* label [H][W] with every value in [0, 2^24) (the host walks the map for this check and learns the largest id, which sizes
 * the presence bitmap); cls NULL or [H][W], any int; skip [n_skip], n_skip <= 8: the values that are no instance (a skip value
 * that does not occur, or lies outside the range, changes nothing).  Outputs, each [cap] with the first *n entries written:
 * ids ascending, bounds [cap][4] = (x1, y1, x2, y2) inclusive, areas, cls_lo / cls_hi = the least and greatest value of cls on
 * the instance's pixels (0 without cls; the caller decides what cls_lo != cls_hi means), *bits_bytes = the bytes of the rows
 * of the boxes.  Six launches whatever the data: presence bits of the values by integer atomicOr, the skip values cleared
 * and the words' popcounts, their prefix sum (two launches; at most 2^19 words of 32 bits, the largest count this file hands
 * the scan), the boxes / areas / class ranges by one set of integer atomics per run of equal values of a row, the ids
 * compacted by the prefix.  MNC_ERR_INVALID: a null label, n or bits_bytes; n_skip outside [0, 8]; cap < 0, or cap > 0 with a
 * null output; H, W or H * W outside the limits; a value outside [0, 2^24).  A map with more than min(cap, 2048) instances is
 * MNC_ERR_INVALID after the device work, with *n set to their number and nothing else written. */
MNC_API int mnc_label_table(const int* label, const int* cls, int H, int W, const int* skip, int n_skip, int cap, int* n, int* ids,
                            int* bounds, long long* areas, int* cls_lo, int* cls_hi, size_t* bits_bytes, int device_id);
/* The rows of the n instances of the table (ids [n] strictly ascending in [0, 2^24), bounds [n][4] non-empty and inside the
 * image) into out_bits: instance i is set where label == ids[i] inside bounds[i].  *bits_bytes = the bytes of the boxes; bytes
 * past them are never written.  One launch over the zeroed output: a wave per 64 pixels of a row ballots the lanes of each
 * distinct value, finds the value in ids by binary search and ORs the ballot, shifted by the box's x1, into one or two words by
 * a 64-bit integer atomicOr.  The label values are not range-checked again: a value that is not in ids is no instance, and
 * pixels of an id outside its box are dropped.  Areas are not recomputed.  n == 0 is answered on the host.  MNC_ERR_INVALID: a
 * null label or bits_bytes; n outside [0, 2048]; n > 0 with null ids, bounds or out_bits; H, W or H * W outside the limits;
 * ids out of range or not ascending; a box that is empty or leaves the image; bits_cap below the bytes of the boxes. */
MNC_API int mnc_label_masks(const int* label, int H, int W, const int* ids, const int* bounds, int n, void* out_bits, size_t bits_cap,
                            size_t* bits_bytes, int device_id);
/* The label map out [H][W] of a set given as mnc_mask_rle takes one (bounds [n][4], offsets [n], bits, bytes): a pixel gets
 * values[i] (NULL: i + 1) of the first instance i in the order that has it set, background where none has -- the painting loop
 * run over the order backwards.  order [n]: a permutation, first the instance that is on top; NULL: by scores [n] descending,
 * the lower index first on equal scores (mnc_mask_layer's order, made on the host the same way).  A mask is empty outside its
 * bounds, bounds may be negative or unclipped (what lies outside the image is dropped), padding bits are not trusted, an
 * instance without rows paints nothing.  One launch, no atomics, every pixel stored exactly once: a wave per 64-pixel strip
 * of a row tests the bounds of 64 instances at a time, walks those that meet the strip in order and leaves when every pixel
 * of the strip is taken.  n == 0 fills out with background on the host.  MNC_ERR_INVALID: a null out; everything
 * mnc_mask_combine refuses about a set; H, W or H * W outside the limits; neither order nor scores (n > 0); order that is not a
 * permutation; a NaN score when the order comes from the scores. */
MNC_API int mnc_mask_to_labels(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const float* scores,
                               const int* order, const int* values, int background, int H, int W, int* out, int device_id);
/* For tools/mask_labels_bench.py.  on = 1: the following calls of the three entries above put a HIP event pair around their
 * launches (without the copies of the map, the set and the results) and keep the last call's time in milliseconds; on = 0:
 * they do not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is none;
 * switching on forgets it. */
MNC_API int mnc_mask_labels_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n20 The contingency table of two label maps: for every pair of values (a, b) that occurs at the same pixel, the number of
 *     such pixels (csrc/label_pairs.hip) -- the table panoptic quality matches segments on, and the confusion matrix of a
 *     semantic result.  The statement of the rule is mnc_amd/pairs.py:label_pairs_numpy.  Integer arithmetic only; integer
 *     atomics only (or, add), which commute, and the order of the output comes from prefix sums, never from the arrival order
 *     of an atomic: the same input gives the same bytes on every run.  The maps are int [H][W], row-major, of one shape, with
 *     H and W in [1, 32768] and H * W <= 2^26, every value in [0, 2^24); no value is background.
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers; one call uploads each map once.  Outputs: *na / *nb = the number of distinct values of a / b, at most 65536
 * each with na * nb <= 2^22 cells; a_ids / b_ids [cap_ids] with the first *na / *nb entries written, ascending; *n_pairs = m, the
 * number of pairs that occur; ia, ib, count [cap_pairs] with the first m entries written: the ranks of the pair's values in
 * a_ids / b_ids and its pixels (positive, summing to H * W), sorted by (ia, ib) ascending.  The launches: the presence bits of
 * both maps by integer atomicOr into one bitmap (a value outside the range sets none and joins a flag word instead: the host
 * does not walk the maps), the words' popcounts, their prefix sum; after a read-back of *na, *nb and the flag, the counts of the
 * pairs' runs by integer atomicAdd into a zeroed int32 table [na][nb] -- tables of at most 16384 cells are counted per workgroup
 * in LDS and added to it once, the others, and every size after mnc_label_pairs_plan(1), in device memory; both give the
 * same integers --, the non-zero cells per 64 by ballot, their prefix sum, the pairs written at
 * prefix plus rank, the ids at their ranks.  MNC_ERR_INVALID, checked on the host before anything is launched, with nothing
 * written: a null a, b, na, nb or n_pairs; a negative cap; a positive cap with a null output of its kind; H, W or H * W outside
 * the limits.  MNC_ERR_INVALID after the device work: a value outside [0, 2^24), with nothing written (mnc_last_error names the
 * first one as "a[y][x]=v not in [0, 16777216)"); more than min(cap_ids, 65536) values in a map or more than 2^22 cells, with
 * *na and *nb set and nothing else written; more than cap_pairs pairs, with *na, *nb and *n_pairs set and nothing else
 * written. */
MNC_API int mnc_label_pairs(const int* a, const int* b, int H, int W, int cap_ids, long long cap_pairs, int* na, int* a_ids, int* nb,
                            int* b_ids, long long* n_pairs, int* ia, int* ib, long long* count, int device_id);
/* For tools/label_pairs_bench.py and the tests.  plan = 1: the following calls of mnc_label_pairs, on every device and thread of the
 * process, count every table in device memory (the global plan); plan = 0: tables of at most 16384 cells in LDS (the default).
 * MNC_ERR_INVALID: any other value. */
MNC_API int mnc_label_pairs_plan(int plan);
/* For tools/label_pairs_bench.py.  on = 1: the following calls of mnc_label_pairs put HIP event pairs around their two groups of
 * launches (without the copies of the maps and of the results, and without the read-back between the groups) and keep the last
 * call's summed time in milliseconds; on = 2: the pair is put around the counting launch alone; on = 0: they do not (the
 * default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is none; switching on forgets
 * it. */
MNC_API int mnc_label_pairs_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n21 The picture under the masks: per instance and channel the pixel count, the sums of v, v^2, x v and y v, the least and
 *     the greatest value with their positions, and the histogram of the values of an image under packed masks
 *     (csrc/mask_pixels.hip) -- on the layout of n5.  The statements of the rules are mnc_amd/pixels.py:pixel_stats_numpy and
 *     histogram_numpy.  Every result is an integer; the floats a caller wants (mean, variance, weighted centroid, percentiles)
 *     follow from them on the host.
 *     Image: row-major [H][W][C] with H and W in [1, 32768], H * W <= 2^26 (n19's limits) and C in [1, 32], of dtype 0 uint8,
 *     1 uint16, 2 int16 or 3 int32; an int32 image has every value in [-2^18, 2^18], so that every sum fits 64 signed bits
 *     (sum v^2 < 2^62, sum x v < 2^59).  It is uploaded once per call, in its own dtype.
 *     Pixels: those of an instance are its set bits inside its bounds that also lie inside [0, W) x [0, H).  Bounds may be
 *     negative, unclipped or wholly outside the image; padding bits are not trusted.  x and y are image coordinates.
 *     Every entry takes the set as mnc_mask_moments takes it.  n == 0 and sets without a row inside the image are answered on
 *     the host (the values of the image are not looked at then).  MNC_ERR_INVALID, checked on the host before anything is
 *     launched and with nothing written: everything mnc_mask_moments refuses about a set; H, W, H * W or C outside the limits;
 *     an unknown dtype; a null pointer where one is needed.  MNC_ERR_INVALID after the device work, with nothing written: a
 *     value of an int32 image outside the range -- a kernel ORs it into a flag word; the host does not walk the image.
 *     One or two launches for the statistics (tiles of 4, 3 or 1 channels), one for the histogram, one more for an int32 image,
 *     whatever the data.  The only atomics are 64-bit integer add, min and max and 32-bit integer LDS adds, which commute:
 *     the same input gives the same bytes on every run.
 *     (There are no forms that read a device-resident mnc_mask_records result: the PackedMasks methods fetch such a result
 *     first.)
 * ------------------------------------------------------------------------------------------------------------- */
/* dtype: 0 uint8, 1 uint16, 2 int16, 3 int32.  sums [n][C][4] = sum, sumsq, sum x v, sum y v;  extrema [n][C][6] = min, min_x, min_y, max, max_x, max_y */
/* count [n].  On equal values the position that is lowest in (y, x) order is given.  An instance without a pixel inside the
 * image has count 0, sums 0 and extrema (0, -1, -1, 0, -1, -1). */
MNC_API int mnc_mask_pixel_stats(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n,
                                 const void* image, int dtype, int H, int W, int C,
                                 long long* count, long long* sums, int* extrema, int device_id);
/* hist [n][C][bins], count [n] (the instance's pixels inside the image, counted or dropped).  A pixel of value v is counted in
 * bin (v - lo) >> shift when that lies in [0, bins), and dropped otherwise.  Each workgroup counts a group of channels of at most
 * 16384 cells in LDS and adds its non-zero cells to the table once.  MNC_ERR_INVALID as above, and: bins outside [1, 4096];
 * shift outside [0, 31]; n * C * bins above 2^24. */
MNC_API int mnc_mask_histogram(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n,
                               const void* image, int dtype, int H, int W, int C, int lo, int shift, int bins,
                               long long* count, long long* hist, int device_id);
/* For tools/pixel_stats_bench.py.  on = 1: the following calls of the two entries above put a HIP event pair around their
 * launches (without the copies of the set, of the image and of the results) and keep the last call's time in milliseconds;
 * on = 0: they do not (the default).  *last_ms (may be NULL) receives the figure kept before this call, -1.0 when there is
 * none; switching on forgets it. */
MNC_API int mnc_mask_pixels_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n22 The distance between outlines: the surfaces of packed masks and, for pairs of instances of two sets, the squared
 *     distances from the surface pixels of the one to the surface of the other -- what the Hausdorff distance, its 95th
 *     percentile, the average symmetric surface distance, the boundary F-measure (the F of DAVIS's J&F) and the normalised
 *     surface Dice are made of (csrc/mask_surface.hip) -- on the layout of n5.  The statements of the rules are
 *     mnc_amd/surface.py:surface_numpy, surface_stats_numpy and surface_distances_numpy.
 *     All arithmetic is integer and all rules are frame-free, by the conventions of n15 and n17: a mask M is a set of
 *     lattice pixels that is empty outside its bounds, bounds may be negative or unclipped, padding bits are not trusted.
 *     Surface: S(M) = the pixels of M with at least one of their four edge neighbours outside M = M & ~erode(M, R2 = 1).
 *     Distances: for a pair (i, j) of instances of the sets A and B and a direction -- 0: A_i -> B_j, 1: B_j -> A_i -- and every
 *     pixel p of S(src), d2(p) = min over q in S(dst) of |p - q|^2 in image coordinates.  pairs [P][2] int = (i, j), in any
 *     order, repeats allowed; slot 2 k + d is pair k in direction d.
 *     The surface words are made by one lane per word from its four neighbours and kept in a scratch plane; every instance
 *     some pair measures against gets, per pixel of its bounds, the distance along the row to its nearest surface pixel
 *     (uint16, 0xffff for a row without one: n15's first pass on the surface words); a lane with a source surface pixel clamps
 *     its x into the destination's columns, where dx = |x - clamp(x)| + that distance, and walks the destination's rows
 *     outward from clamp(y) while dy^2 is below the best so far.  The workgroups are listed on the host from the bounds, so the
 *     launch count is fixed whatever the data.  Integer add and max atomics only: the same input gives the same bytes on
 *     every run.
 *     Every entry takes a set as mnc_mask_rle takes it: bounds [n][4] int, offsets [n], bits, bytes = the bytes bits holds.
 *     n == 0, m == 0, P == 0 and sets without a single row are answered on the host.  MNC_ERR_INVALID, checked on the host
 *     before anything is launched and with nothing written, for every entry: everything mnc_mask_boundary refuses about
 *     either set (n outside [0, 2048], |coordinate| >= 2^24, more than 2^26 pixels in one bound, an offset that is negative or
 *     not a multiple of 8, rows that reach past bytes); P outside [0, 65536]; a pair index out of range; T outside [0, 8]; a
 *     tau2 outside [0, 2^31); a hull of the bounds of all instances with rows of both sets that spans 32768 or more pixels in
 *     either axis (below it every d2 < 2^31 and every sum fits 64 signed bits); more than 2^27 pixels of rows in the call
 *     (n15's limit); a null pointer where one is needed.  (There are no forms that read a device-resident mnc_mask_records
 *     result: the PackedMasks methods fetch such a result first.)
 * ------------------------------------------------------------------------------------------------------------- */
/* The surfaces as a set.  The result has the layout of n5 as mnc_mask_boundary writes it and the input's bounds (an instance
 * without rows keeps them and gets no rows): out_offsets [n] are multiples of 8, in order without gaps; out_areas [n] are the
 * surface pixel counts; padding bits are 0.  out_bounds, out_offsets and *bits_bytes follow from the bounds alone and are
 * computed on the host: with out_bits == NULL the call returns them and launches nothing (out_areas may be NULL then);
 * bits_cap < *bits_bytes is MNC_ERR_INVALID with the three set and nothing else written.  Bytes past *bits_bytes are never
 * written.  One launch. */
MNC_API int mnc_mask_surface(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int* out_bounds,
                             long long* out_offsets, long long* out_areas, void* out_bits, size_t bits_cap, size_t* bits_bytes,
                             int device_id);
/* The distances reduced.  Outputs, every one indexed by slot: count [P][2] = |S(src)|; max_d2 [P][2] the greatest d2;
 * argmax [P][2][2] the (x, y) of the source pixel that attains it, the lowest (y, x) on ties; sum_d2 [P][2] the sum of d2;
 * within [P][2][T] the source pixels with d2 <= tau2[t].  Where S(src) or S(dst) is empty: max_d2 -1, argmax (-1, -1), sum_d2 0,
 * within 0, count as it is.  The kernel reduces the sum, the counts and the 64-bit key (d2 << 32) | (0xffffffff - raster index
 * in the source's bounds) by shuffles, then LDS, then one 64-bit atomic add resp. max per workgroup and figure.  Three launches,
 * no read-back between them. */
MNC_API int mnc_mask_surface_stats(const int* a_bounds, const long long* a_offsets, const void* a_bits, size_t a_bytes, int n,
                                   const int* b_bounds, const long long* b_offsets, const void* b_bits, size_t b_bytes, int m,
                                   const int* pairs, int P, const int* tau2, int T, long long* count, long long* max_d2,
                                   int* argmax, long long* sum_d2, long long* within, int device_id);
/* The distances themselves.  Outputs: ptr [2 P + 1] (ptr[0] = 0; slot s owns the entries ptr[s] .. ptr[s + 1] - 1: the d2 of
 * the source's surface pixels in raster (y, x) order), *total = ptr[2 P], d2 [*total]; a slot whose destination has no surface
 * pixel holds 0xffffffff.  The protocol is mnc_mask_distance's: d2 == NULL gives ptr and *total only and launches nothing more
 * than the surfaces and their counts need; otherwise cap is the room of d2 in entries, and cap < *total is MNC_ERR_INVALID with
 * ptr and *total set and nothing else written.  Entries past *total are never written.  One read-back, of the instances'
 * surface pixel counts, from which the host makes ptr; a pixel's place is ptr[s] plus its rank, the prefix sum of the surface
 * words' popcounts before its word plus the popcount below its bit.  MNC_ERR_INVALID after that read-back, with nothing
 * written: more than 2^28 entries. */
MNC_API int mnc_mask_surface_dist(const int* a_bounds, const long long* a_offsets, const void* a_bits, size_t a_bytes, int n,
                                  const int* b_bounds, const long long* b_offsets, const void* b_bits, size_t b_bytes, int m,
                                  const int* pairs, int P, long long* ptr, unsigned* d2, size_t cap, size_t* total, int device_id);
/* For tools/surface_dist_bench.py.  on = 1: the following calls of the three entries above put HIP event pairs around their
 * launches (without the copies of the sets and of the results, and without the raw entry's read-back) and keep the last call's
 * summed time in milliseconds; on = 0: they do not (the default).  *last_ms (may be NULL) receives the figure kept before this
 * call, -1.0 when there is none; switching on forgets it. */
MNC_API int mnc_mask_surface_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n23 Training targets on packed ground-truth masks: the two per-RoI loops of the reference's training step
 *     (csrc/mask_targets.hip) -- the mask regression target of a box (lib/transform/mask_transform.py:49-80 intersect_mask,
 *     called per foreground RoI by ProposalTargetLayer and StageBridgeLayer) and the overlap of a predicted mask with its
 *     ground truth (lib/pylayer/mask_layer.py:68-83) -- on the layout of n5.  The statements of the rules are
 *     mnc_amd/targets.py:mask_targets_numpy and mask_pred_overlaps_numpy.
 *     Both entries take the ground truth as mnc_mask_overlaps takes a set: bounds [G][4] int (the rounded, unscaled
 *     ground-truth boxes), offsets [G], areas [G], bits, bytes = the bytes bits holds.  Padding bits are not trusted.  Each
 *     is one launch and one read-back; the counters are integer atomics: two calls give the same bytes.
 *     MNC_ERR_INVALID, checked on the host before anything is launched and with nothing written, for both: everything
 *     mnc_mask_overlaps refuses about a set (|coordinate| >= 2^24, more than 2^26 pixels in one bound, an offset that is
 *     negative or not a multiple of 8, rows that reach past bytes); K outside [0, 65536]; mask_size outside [1, 32]; a null
 *     pointer where one is needed.  K == 0 launches nothing.
 * ------------------------------------------------------------------------------------------------------------- */
/* ex_boxes [K][4] int (x1, y1, x2, y2, inclusive), gt_index [K] -> out [K][mask_size][mask_size] bytes 0 / 1.  Row k, with e
 * its box, g the bounds of instance gt_index[k] and M that instance's mask: all zeros when e and g do not intersect (an
 * instance without rows intersects nothing); else (cv2.resize(C, (S, S)) >= (float)thresh), C the float32 canvas of e's size
 * that is M on e & g and 0 elsewhere, INTER_LINEAR as in n5 (source coordinate in float64 rounded to float32, horizontal pass
 * then vertical in float32).  The canvas is not made: one lane per output cell reads four bits.
 * MNC_ERR_INVALID also for: a box with x2 < x1 or y2 < y1; a coordinate with |c| >= 2^24; a box of more than 2^26 pixels;
 * gt_index[k] outside [0, G); a NaN thresh. */
MNC_API int mnc_mask_targets(const int* gt_bounds, const long long* gt_offsets, const long long* gt_areas, const void* gt_bits,
                             size_t gt_bytes, int G, const int* ex_boxes, const int* gt_index, int K, int mask_size, double thresh,
                             unsigned char* out, int device_id);
/* boxes [K][4] float64, preds [K][mask_size][mask_size] float32, gt_index [K] (-1: a background row, skipped) -> inter [K],
 * area_pred [K].  The mask of row k is mnc_instance_masks's with clip = 0: the box rounded half to even and not clipped, the
 * prediction resized to it and binarised with >= (float)thresh; area_pred[k] = its set pixels, inter[k] = those also set in
 * instance gt_index[k] (what mnc_mask_overlaps counts for that pair).  A row with gt_index -1 gets 0 and 0.  No mask bit is
 * written anywhere: the ballots are counted as they are made.
 * MNC_ERR_INVALID also for what mnc_instance_masks refuses with clip = 0, in any row (a rounded coordinate with |c| >= 2^24,
 * a box that is empty once rounded, more than 2^26 pixels), and gt_index[k] outside [-1, G). */
MNC_API int mnc_mask_pred_overlaps(const int* gt_bounds, const long long* gt_offsets, const long long* gt_areas,
                                   const void* gt_bits, size_t gt_bytes, int G, const double* boxes, const float* preds,
                                   const int* gt_index, int K, int mask_size, double thresh, long long* inter,
                                   long long* area_pred, int device_id);
/* For tools/train_targets_bench.py.  on = 1: the following calls of the two entries above put a HIP event pair around their
 * launch (and the clearing of the counters; without the copies of the set, of the rows and of the results) and keep the last
 * call's time in milliseconds; on = 0: they do not (the default).  *last_ms (may be NULL) receives the figure kept before this
 * call, -1.0 when there is none; switching on forgets it. */
MNC_API int mnc_mask_targets_timing(int on, double* last_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * n24 The differentiable half of the training graph that is MNC's own: the backward passes of ROIWarping (with respect to the
 *     feature map AND to the box: "enables gradient back-propagation with respect to RoI coordinates", arXiv:1512.04412 section
 *     3), of the MAX 2x2/2 pooling behind the 28x28 warp, of MaskResize and of MaskPooling (csrc/roi_backward.hip).  Device-pointer
 *     graph ops on an engine context (declared further down), in the style of mnc_roi_warp; the statements of the rules are
 *     mnc_amd/backward.py: roi_warp_backward_numpy, maxpool2_backward_numpy, mask_resize_backward_numpy, mask_pool_backward_numpy.
 *     All rules are the derivatives of oracle/SPEC.md sections 1-3 under the SPEC's default conventions; floor is piecewise
 *     constant, so x0, y0 are constants and the sample position enters only through ax = sx - x0, ay = sy - y0.  No
 *     floating-point atomics anywhere: two calls on the same inputs give the same bytes.
 *
 *     ROIWarping backward.  Grid PH x PW (the unfused layer); F is zero outside the map.  For RoI r and cell (ph, pw) the float32
 *     quantities x1s, y1s, bw, bh, sx, sy, x0, y0, ax, ay are the FORWARD'S OWN: the identical expressions in the identical order
 *     as mnc_roi_warp / orc_roi_warp.  g = dtop[r][ph][pw][c].
 *       dfeat[c][y][x] = the sum of w * g over all (r, ph, pw, tap) whose tap lands on (y, x); w00 = (1-ax)(1-ay), w01 = ax(1-ay),
 *         w10 = (1-ax)ay, w11 = ax ay, each formed as in the forward and then multiplied by g; taps outside the map are dropped.
 *         ORDER OF SUMMATION, part of the rule: ascending r, then ph, then pw, within one sample 00, 01, 10, 11; float32, from
 *         +0.0f, no contraction.  The kernel equals the float32 statement bit for bit.
 *       drois[r][0] = 0.  Per sample dsx_c = (1-ay)(F01-F00) + ay(F11-F10), dsy_c = (1-ax)(F10-F00) + ax(F11-F01), Gx = sum_c g dsx_c,
 *         Gy = sum_c g dsy_c; drois[r][1] += scale (1-tx) Gx, [3] += scale tx Gx, [2] += scale (1-ty) Gy, [4] += scale ty Gy, with
 *         tx = pw / PW when the width is FREE, else 0 (ty alike): free iff the float32 value x2s - x1s + 1 is >= 1, the max(., 1)
 *         clamp inactive or tied (the sub-gradient of torch's clamp(min=1)); a clamped width sends all of Gx to x1.  The order of
 *         this sum is the launch geometry's: one workgroup per RoI, one fixed reduction tree.
 *     MAX 2x2/2 backward: the gradient of an output goes to the FIRST maximum of its window in the order (0,0), (0,1), (1,0),
 *       (1,1) -- a later element wins only when strictly greater, the forward's max4 order and Caffe's rule -- the other three
 *       inputs get +0.0f.  The argmax is recomputed from the forward's input; no index tensor exists.  Bit-exact.
 *     MaskResize backward: din[r][iy][ix] = the sum over output cells (h, w), ascending h then w, of weight * dout[r][h][w], the
 *       weight of the input cell in that output exactly SPEC section 2's: the bilinear four, or 1 on the nearest cell when
 *       sx == IW - 1 or sy == IH - 1.  Bit for bit with the statement.
 *     MaskPooling backward: dfeat[r][h][w][c] = dtop[r][h][w][c] * mask[r][h][w] (bit-exact); dmask[r][h][w] = sum_c dtop * feat,
 *       one wave per position in a fixed order.
 *
 *     Every output is fully written, zeros included.  The entries make their forward entries' argument checks: MNC_ERR_INVALID
 *     before any launch.  MNC_ERR_UNSUPPORTED, before any launch too, when the context carries a convention other than the SPEC's
 *     for the layer in question (mnc_layer_conventions: the four warp_ fields; resize_mode; maskpool_binary).  RoI coordinates
 *     are expected finite.
 * ------------------------------------------------------------------------------------------------------------- */
struct mnc_ctx;   /* the engine context, declared below */
/* d_feat_c8 and d_dfeat_c8 [C/8][H][W][8], the forward's input layout; d_dtop [R][PH][PW][C], its output layout; d_drois [R][5].
 * d_dfeat_c8 or d_drois may be NULL to skip that half (not both; d_feat_c8 is read for d_drois only and may be NULL without it).
 * R == 0 writes a zero dfeat and returns.  MNC_ERR_INVALID also for PH or PW >= 32768.  The pixel-major copies and the range
 * tables live in the context's scratch arena. */
MNC_API int mnc_roi_warp_backward(struct mnc_ctx* ctx, const float* d_feat_c8, int C, int H, int W, const float* d_rois, int R, int PH,
                                  int PW, float spatial_scale, const float* d_dtop, float* d_dfeat_c8, float* d_drois);
/* d_in [R][PH][PW][C] = the forward's input (PH, PW even, as mnc_maxpool2_rhwc takes them), d_dout [R][PH/2][PW/2][C] ->
 * d_din [R][PH][PW][C]. */
MNC_API int mnc_maxpool2_rhwc_backward(struct mnc_ctx* ctx, const float* d_in, const float* d_dout, float* d_din, int R, int PH, int PW,
                                       int C);
/* d_dout [R][OH][OW] -> d_din [R][IH][IW]. */
MNC_API int mnc_mask_resize_backward(struct mnc_ctx* ctx, const float* d_dout, float* d_din, int R, int IH, int IW, int OH, int OW);
/* d_feat, d_dtop, d_dfeat [R][PH][PW][C]; d_mask, d_dmask [R][PH][PW].  d_dfeat or d_dmask may be NULL to skip that half (not
 * both); d_mask is read for d_dfeat only, d_feat for d_dmask only. */
MNC_API int mnc_mask_pool_backward(struct mnc_ctx* ctx, const float* d_feat, const float* d_mask, const float* d_dtop, float* d_dfeat,
                                   float* d_dmask, int R, int PH, int PW, int C);

/* ---------------------------------------------------------------------------------------------------------------
 * n25 The loss layers that end the five stages of models/VGG16/mnc_5stage/train.prototxt -- SoftmaxWithLoss, SmoothL1Loss,
 *     SigmoidCrossEntropyLoss: the value and the gradient with respect to the prediction -- and the backward passes of ReLU and
 *     Sigmoid that carry that gradient to the next InnerProduct (csrc/loss.hip).  Device-pointer graph ops on an engine context
 *     like n24: everything is stream-ordered on the context's stream, no entry reads anything back or synchronises (the
 *     context's scratch arena is grown on first use, as for every entry that uses it).  The statements of the rules are
 *     mnc_amd/losses.py: softmax_loss_numpy, smooth_l1_loss_numpy, sigmoid_ce_loss_numpy, eltwise_backward_numpy; the rules are
 *     public BVLC Caffe's and py-faster-rcnn's (caffe-mnc's own layer sources are not available); what those leave open is a
 *     CHOICE of DESIGN.md.  All tensors are float32; labels are float32 as in a Caffe blob and are cast with (int).  exp of a
 *     float32 is np_exp_f32 (csrc/np_exp.h) and the file is compiled without contraction: every gradient, the probabilities
 *     and the SmoothL1 terms equal the float32 statement BIT FOR BIT; the softmax and sigmoid terms differ from it by logf.
 *
 *     d_result, 16 bytes on the device: float loss (unweighted, Caffe's top), float normaliser, int32 count, int32 status.
 *     The loss is a sum of per-workgroup partials in a fixed geometry, added in index order by one workgroup: no floating-point
 *     atomics, the same bytes on every run.  At most three launches per entry.  A null optional output is skipped; a call
 *     with d_result alone writes nothing else.  MNC_ERR_INVALID before any launch: a null ctx, d_result or input; a shape
 *     outside the limits.  A zero-size call (outer * inner == 0; N == 0; count == 0) zeroes the 16 bytes and launches nothing.
 *
 *     SoftmaxWithLoss on score [outer][C][inner], label [outer][inner]; 1 <= C <= 4096, outer * inner < 2^31.  m = max_c score;
 *       e_c = exp(score_c - m); s = the sum of e_c in ASCENDING c from +0.0; p_c = e_c / s.  li = (int)label.  A position is
 *       ignored when has_ignore and li == ignore_label; otherwise INVALID when the label is non-integral, outside [0, C), NaN or
 *       outside int's range: never used as an index, counted as ignored, bit 0 of the status set.  term = -log(max(p_li,
 *       FLT_MIN)) at valid positions, 0 elsewhere; count = the valid positions; normaliser = max(count, 1) when normalize, else
 *       outer; loss = sum of terms / normaliser.  dscore_c = (p_c - [c == li]) * (loss_weight / normaliser) at valid positions,
 *       +0.0 in all C channels elsewhere.  Scores are expected finite.  Two layouts: one lane per position with class stride
 *       inner (inner > 1), one wave per position (inner == 1); the same bits.
 *     SmoothL1Loss on count elements: s2 = sigma * sigma, thr = 1 / s2, d = (pred - target) * w_in,
 *       term = (|d| < thr ? 0.5 * s2 * d * d : |d| - 0.5 / s2) * w_out, operations left to right, the comparison strict;
 *       loss = sum / N; dpred = (|d| < thr ? s2 * d : (0 < d) - (d < 0)) * w_in * w_out * (loss_weight / N).  The gradient with
 *       respect to target is its negation and has no output.  count of the result = the elements.
 *     SigmoidCrossEntropyLoss on count elements: pos = [x >= 0], term = -(x * (t - pos) - log(1 + exp(x - 2 * x * pos))) * w,
 *       loss = sum / N, dx = (1 / (1 + exp(-x)) - t) * w * (loss_weight / N); d_w NULL = ones.  exp(-x) may be +inf: dx is then
 *       -t * w * (loss_weight / N).
 *     Activation backward from the layer's OUTPUT y: ReLU dx = y > 0 ? dy : +0.0; Sigmoid dx = (dy * y) * (1 - y).
 * ------------------------------------------------------------------------------------------------------------- */
/* d_prob and d_dscore [outer][C][inner], d_terms [outer][inner]; each may be NULL. */
MNC_API int mnc_softmax_loss(struct mnc_ctx* ctx, const float* d_score, const float* d_label, int outer, int C, int inner, int has_ignore,
                             int ignore_label, int normalize, float loss_weight, float* d_prob, float* d_terms, float* d_dscore,
                             void* d_result);
/* For tools/loss_bench.py and the tests.  plan = 1: the following calls of mnc_softmax_loss, on every context of the process, run
 * the one-lane-per-position layout on any shape; plan = 2: the one-wave-per-position layout; plan = 0: by inner (the default).
 * MNC_ERR_INVALID: any other value. */
MNC_API int mnc_softmax_loss_plan(int plan);
/* All five tensors hold count elements, count < 2^31; N = shape[0] of the layer's bottoms.  d_terms and d_dpred may be NULL. */
MNC_API int mnc_smooth_l1_loss(struct mnc_ctx* ctx, const float* d_pred, const float* d_target, const float* d_w_in, const float* d_w_out,
                               int N, long long count, float sigma, float loss_weight, float* d_terms, float* d_dpred, void* d_result);
/* d_w NULL: no weight bottom.  d_terms and d_dx may be NULL. */
MNC_API int mnc_sigmoid_ce_loss(struct mnc_ctx* ctx, const float* d_x, const float* d_t, const float* d_w, int N, long long count,
                                float loss_weight, float* d_terms, float* d_dx, void* d_result);
/* op as mnc_eltwise: 1 ReLU, 2 Sigmoid.  d_y is the forward's output; count == 0 launches nothing. */
MNC_API int mnc_eltwise_backward(struct mnc_ctx* ctx, const float* d_y, const float* d_dy, float* d_dx, size_t count, int op);

/* ---------------------------------------------------------------------------------------------------------------
 * n3  The input edge of the CFM task: the MCG proposal maskdb of one image, the validation branch of
 *     tools/prepare_mcg_maskdb.py:55-97 (csrc/mcg_maskdb.hip).
 * ------------------------------------------------------------------------------------------------------------- */
/* Host pointers, one call per image.  superpixels [H][W] ids; proposal i is the union P_i of the superpixels
 * label_ids[label_ptr[i] .. label_ptr[i + 1]) (np.in1d: duplicates and ids that occur nowhere in the map change nothing).
 * boxes[i] = (min col, min row, max col, max row) of P_i as float64; masks[i] [mask_size][mask_size] bytes 0 / 1 =
 * cv2.resize(P_i cropped to its box, (mask_size, mask_size), INTER_NEAREST): mask[dy][dx] = P_i[y1 + sy(dy)][x1 + sx(dx)],
 * sx(dx) = min(floor(dx * ifx), w - 1) with ifx = 1.0 / ((double)mask_size / w) in float64, w = x2 - x1 + 1; sy alike with h
 * (OpenCV's resizeNN: the inverse scale formed in two steps, then cvFloor -- stated from OpenCV's published source).
 * n == 0 returns before any device work.  MNC_ERR_INVALID, checked before anything is launched: n < 0, mask_size outside
 * [1, 32], H or W outside [1, 32768], label_ptr[0] != 0 or label_ptr decreasing, any id of superpixels or label_ids outside
 * [0, 65535].  A proposal with empty P_i (an empty list, or none of its ids in the map; the reference dies in np.min) is
 * detected by the kernel from its own data: MNC_ERR_INVALID after the call's device work, mnc_last_error names the smallest
 * such index, and boxes / masks are then unspecified. */
MNC_API int mnc_mcg_maskdb(const int* superpixels, int H, int W, const int* label_ptr, const int* label_ids, int n,
                           int mask_size, double* boxes, unsigned char* masks, int device_id);

/* ---------------------------------------------------------------------------------------------------------------
 * b3  utils.cython_bbox.bbox_overlaps (lib/utils/bbox.pyx:15-55): float64 IoU with +1 widths, [N][K] row-major.
 *     A host function in the reference (Cython) and here (C); it is not a GPU kernel and has no GPU counterpart.
 * ------------------------------------------------------------------------------------------------------------- */
MNC_API int mnc_bbox_overlaps(const double* boxes, int n, const double* query_boxes, int k, double* overlaps);

/* ---------------------------------------------------------------------------------------------------------------
 * Engine context: one per process per GPU (b5: `caffe.set_device`, one `caffe.Net` per process).  Owns a HIP
 * stream and all device scratch.  Not thread-safe; use one context per thread.
 * Hosts that keep several images in flight use one context (stream) per image.  The HIP runtime maps streams onto
 * GPU_MAX_HW_QUEUES hardware queues (default 4; streams that share a queue serialise; round 6, profiles/r06_streams.txt), and
 * reads that variable once, at the process's first HIP call.  When this library is loaded it therefore makes a REQUEST
 * (profiles/hw_queues.txt): the environment variable MNC_HW_QUEUES -- unset: 16; "0": leave GPU_MAX_HW_QUEUES alone; any other
 * integer, clamped to 4 .. 32 (text that is no integer counts as unset).  A GPU_MAX_HW_QUEUES that is absent, no positive integer
 * or LOWER than the request is set to the request; an equal or higher one is kept: the library never lowers it, and MNC_HW_QUEUES
 * is the one way to opt out or to choose (raising a value the host exported prints one line on stderr).  The request is void when HIP was initialised before the library was loaded (another
 * library's import came first): mnc_stream_concurrency measures what the process really has.  The load-time hook uses getenv /
 * setenv, which are not safe against other threads using the environment at that moment: a host that dlopen()s the library late,
 * beside running threads, exports GPU_MAX_HW_QUEUES itself beforehand and sets MNC_HW_QUEUES=0.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct mnc_ctx mnc_ctx;

/* What the request did to GPU_MAX_HW_QUEUES. */
#define MNC_HWQ_UNTOUCHED 0   /* MNC_HW_QUEUES=0: the variable was left as it was */
#define MNC_HWQ_KEPT 1        /* the exported value was already the request or more */
#define MNC_HWQ_RAISED 2      /* the variable was absent, unusable or lower: set to the request */
/* The policy itself, a pure function of two strings (either may be NULL = not in the environment): exported = GPU_MAX_HW_QUEUES,
 * setting = MNC_HW_QUEUES.  *value = what GPU_MAX_HW_QUEUES holds afterwards (0: still absent / unusable), *action = MNC_HWQ_*.
 * Reads and changes nothing; no HIP call. */
MNC_API int mnc_hw_queue_policy(const char* exported, const char* setting, int* value, int* action);
/* What the load-time hook did in this process: *requested = the request (0 = MNC_HW_QUEUES=0), *exported_before = the value
 * GPU_MAX_HW_QUEUES had when the library was loaded (-1: absent or no positive integer), *action = MNC_HWQ_*.  No HIP call. */
MNC_API int mnc_hw_queue_request(int* requested, int* exported_before, int* action);
/* The number of hardware queues n_streams streams really get in this process, measured (csrc/queue_probe.hip): n_streams
 * (1 .. 32) non-blocking streams are created, each runs one 64-thread workgroup that spins for 1 ms of the device's wall clock
 * (an iteration cap bounds it whatever the clock does), and *concurrent = the largest number of those intervals that overlap --
 * kernels of streams that share a queue run one after the other.  A few milliseconds; the streams are destroyed again.  The
 * figure is a lower bound when other work keeps the device's CUs full meanwhile.  MNC_ERR_INVALID: n_streams out of range. */
MNC_API int mnc_stream_concurrency(int device, int n_streams, int* concurrent);

MNC_API int mnc_ctx_create(mnc_ctx** out, int device_id);
MNC_API int mnc_ctx_destroy(mnc_ctx* ctx);
MNC_API int mnc_ctx_sync(mnc_ctx* ctx);
MNC_API int mnc_ctx_device(const mnc_ctx* ctx, int* device_id);
/* Number of times one of the context's internal device arenas (split-K / Winograd scratch, proposal state, voting scratch) has
 * been re-allocated.  A captured HIP graph holds their addresses: mnc_forward_image drops its graph when this value has moved
 * since the capture; a caller that captures library launches into its own graph must do the same. */
MNC_API int mnc_ctx_arena_generation(const mnc_ctx* ctx, unsigned long* generation);

/* Conventions of the three Caffe layers whose source (caffe-mnc) is not available: ROIWarping, MaskResize, MaskPooling
 * (models/VGG16/mnc_5stage/test.prototxt:479-492, 558-567, 631-637, 809-820).  Every SPEC-CHOICE of oracle/SPEC.md is a field;
 * all fields zero (maskpool_thresh unused) IS the SPEC and the default of every context -- PARITY UNPINNED either way.  A user who
 * can read caffe-mnc (or holds the published mnc_model.caffemodel.h5 and an image with known output) selects the matching
 * convention here / in mnc_net_config / with `caffe.Net(..., layer_conventions={...})` / cfg.LAYER_CONVENTIONS; nothing is
 * recompiled.  The CPU oracle evaluates the same switches (oracle/mnc_oracle.c: orc_roi_warp_ex, orc_mask_resize_ex,
 * orc_mask_pool_ex), bit for bit; oracle/SPEC.md section 6 tabulates how far each alternative moves the outputs.
 * Read by mnc_roi_warp[_sm], mnc_mask_resize, mnc_mask_pool[_sm], mnc_box_mask_pool at launch time. */
typedef struct mnc_layer_conventions {
  int warp_sample;       /* ROIWarping sample position in bin g: 0 x1s + g*bin (top-left, SPEC) | 1 x1s + (g+0.5)*bin (bin centre)
                          * | 2 x1s + (g+0.5)*bin - 0.5 (bin centre, pixel-centre coordinates) */
  int warp_round_edges;  /* 0 scaled RoI edges un-rounded (SPEC) | 1 floor(x*scale + 0.5), as ROIPooling */
  int warp_no_plus_one;  /* 0 roi_w = max(x2s - x1s + 1, 1) (SPEC) | 1 roi_w = max(x2s - x1s, 1) */
  int warp_oob;          /* 0 bilinear taps outside the map contribute 0 (SPEC) | 1 taps clamped to the border */
  int resize_mode;       /* MaskResize source position: 0 dst*in/out, nearest on the last row/column (mv_kernel.cu:193-240, SPEC)
                          * | 1 (dst+0.5)*in/out - 0.5 (half-pixel centres) | 2 dst*(in-1)/(out-1) (align_corners) */
  int maskpool_binary;   /* MaskPooling: 0 feature * continuous mask (SPEC) | 1 feature * (mask >= maskpool_thresh) */
  float maskpool_thresh; /* 0.4 = cfg.BINARIZE_THRESH */
  int inherit;           /* read by mnc_net_create only (mnc_net_config.conventions): 1 = leave the conventions in force on the
                          * context alone (what mnc_net_default_config sets), 0 = apply this struct to the context -- all other
                          * fields zero then selects the SPEC explicitly, whatever an earlier net or the host had set.
                          * mnc_ctx_set_layer_conventions ignores it. */
} mnc_layer_conventions;
MNC_API int mnc_ctx_set_layer_conventions(mnc_ctx* ctx, const mnc_layer_conventions* conv);   /* NULL: back to the SPEC */
/* Override one of the launchers' own choices on this context (a tile shape, a kernel variant, a plan switch): name as in
 * csrc/mnc_internal.h MNC_TUNE_KEYS, e.g. "FC_TILE" / "5", "CONV1X1_TILE" / "2,4"; value NULL or "" = the library's choice again.
 * The environment variable MNC_<NAME> sets the same value when the context is created -- launch paths never read the
 * environment.  For tests (every variant reachable at a small shape) and A/B measurements; results never change beyond the
 * summation grouping of K splits. */
MNC_API int mnc_ctx_set_tuning(mnc_ctx* ctx, const char* name, const char* value);
MNC_API int mnc_ctx_get_layer_conventions(const mnc_ctx* ctx, mnc_layer_conventions* conv);

/* Launch-sequence capture for hosts that drive the per-layer entry points themselves (the caffe-shaped Python engine does, for
 * any prototxt): everything the library enqueues on the context's stream between capture_begin and capture_end -- kernels,
 * mnc_h2d_async / mnc_d2h_async / mnc_d2d copies -- becomes one HIP graph; mnc_graph_launch replays it with one call.  Inside a
 * capture nothing may synchronise or allocate (mnc_h2d, mnc_d2h, mnc_ctx_sync, mnc_dev_alloc / _free, a growing internal
 * arena): such a call is refused with MNC_ERR_STATE BEFORE it touches the stream (the capture stays intact: end it, discard the
 * graph, run the sequence eagerly once so that every buffer has its size, capture again).  mnc_ctx_capture_begin itself returns
 * MNC_ERR_STATE while per-launch profiling is on (mnc_prof_enable): event pairs cannot be captured.  The graph holds raw device addresses: mnc_graph_launch returns MNC_ERR_STATE when an internal arena of
 * the context has been re-allocated since the capture (mnc_ctx_arena_generation) -- capture again.  The caller keeps its own
 * buffers in place.  mnc_forward_image uses the same mechanism internally. */
typedef struct mnc_graph mnc_graph;
MNC_API int mnc_ctx_capture_begin(mnc_ctx* ctx);
MNC_API int mnc_ctx_capture_end(mnc_ctx* ctx, mnc_graph** out);     /* *out = NULL and an error status when the capture failed */
MNC_API int mnc_graph_launch(mnc_ctx* ctx, mnc_graph* graph);        /* asynchronous on the context's stream */
MNC_API int mnc_graph_destroy(mnc_graph* graph);
/* Device address of the row count the last mnc_proposal left on the device (valid until the proposal state is re-allocated):
 * lets a captured sequence copy it down with its results instead of calling mnc_proposal_count (which synchronises). */
MNC_API int mnc_proposal_count_ptr(mnc_ctx* ctx, void** d_count);

/* Device memory for the host-side executor (the caffe-shaped Net keeps its blobs here). */
MNC_API int mnc_dev_alloc(mnc_ctx* ctx, size_t bytes, void** d_ptr);
MNC_API int mnc_dev_free(mnc_ctx* ctx, void* d_ptr);
MNC_API int mnc_h2d(mnc_ctx* ctx, void* d_dst, const void* src_host, size_t bytes);   /* stream-ordered + sync */
MNC_API int mnc_d2h(mnc_ctx* ctx, void* dst_host, const void* d_src, size_t bytes);   /* stream-ordered + sync */
MNC_API int mnc_d2d(mnc_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);      /* stream-ordered, async */
MNC_API int mnc_dev_zero(mnc_ctx* ctx, void* d_ptr, size_t bytes);
/* Page-locked host memory for the image that goes up and the instance records that come down, and the stream-ordered copies
 * that do NOT synchronise (from / to pinned memory they are truly asynchronous; the caller synchronises with mnc_ctx_sync). */
MNC_API int mnc_host_alloc(mnc_ctx* ctx, size_t bytes, void** host_ptr);
MNC_API int mnc_host_free(mnc_ctx* ctx, void* host_ptr);
MNC_API int mnc_h2d_async(mnc_ctx* ctx, void* d_dst, const void* src_host, size_t bytes);
MNC_API int mnc_d2h_async(mnc_ctx* ctx, void* dst_host, const void* d_src, size_t bytes);

/* Per-kernel timing with HIP events on the context's stream (bench.py's `roofline` numbers come from here).
 * enable=1 records a start/stop event pair around every kernel launched through the context; enable=2 only around the
 * launches that carry >= 1 GFLOP of algorithmic work (the MFMA kernels), which keeps the timed region almost undisturbed. */
MNC_API int mnc_prof_enable(mnc_ctx* ctx, int enable);
MNC_API int mnc_prof_reset(mnc_ctx* ctx);
MNC_API int mnc_prof_count(mnc_ctx* ctx, int* n_records);                 /* synchronises the stream */
MNC_API int mnc_prof_get(mnc_ctx* ctx, int index, char* name_buf, int name_cap, float* ms, double* flops,
                         double* bytes);

/* ---------------------------------------------------------------------------------------------------------------
 * Layout conversion and weight packing (device -> device, asynchronous on the context's stream).
 * ------------------------------------------------------------------------------------------------------------- */
MNC_API int mnc_nchw_to_c8(mnc_ctx* ctx, const float* d_nchw, float* d_c8, int C, int H, int W);  /* C%8==0 */
MNC_API int mnc_c8_to_nchw(mnc_ctx* ctx, const float* d_c8, float* d_nchw, int C, int H, int W);
/* [R][C][PH][PW] (Caffe) <-> [R][PH][PW][C] (engine) */
MNC_API int mnc_rchw_to_rhwc(mnc_ctx* ctx, const float* d_in, float* d_out, int R, int C, int PH, int PW);
MNC_API int mnc_rhwc_to_rchw(mnc_ctx* ctx, const float* d_in, float* d_out, int R, int C, int PH, int PW);
/* Caffe conv weight [Cout][Cin][3][3] -> packed [Cin/8][Cout][76].  Cin%8==0, Cout%32==0.  Elements: Cin/8*Cout*76 */
MNC_API int mnc_pack_conv3x3_weights(mnc_ctx* ctx, const float* d_oihw, float* d_packed, int Cout, int Cin);
/* Caffe InnerProduct weight [N][C*PH*PW] (columns in (c,h,w) order) -> [N][PH*PW*C] ((h,w,c) order). */
MNC_API int mnc_pack_fc_weights(mnc_ctx* ctx, const float* d_nchw_cols, float* d_hwc_cols, int N, int C, int PH, int PW);

/* ---------------------------------------------------------------------------------------------------------------
 * Graph ops -- one per layer type of models/VGG16/mnc_5stage/test.prototxt.  All asynchronous on the
 * context's stream; all tensors fp32.
 * ------------------------------------------------------------------------------------------------------------- */
/* conv1_1 (test.prototxt:19-40): 3x3 pad 1, Cin = 3, reads the NCHW input blob, + bias + ReLU -> c8.  HBM-bound. */
MNC_API int mnc_conv3x3_c3(mnc_ctx* ctx, const float* d_in_nchw, const float* d_w_oihw, const float* d_bias,
                           float* d_out_c8, int H, int W, int Cout, int relu);
/* Convolution 3x3 pad 1 stride 1 + bias (+ ReLU) (test.prototxt:41-412), c8 -> c8, fp32 MFMA implicit GEMM. */
MNC_API int mnc_conv3x3(mnc_ctx* ctx, const float* d_in_c8, const float* d_w_packed, const float* d_bias,
                        float* d_out_c8, int H, int W, int Cin, int Cout, int relu);
/* The same convolution on the bf16 matrix pipe with fp32-class accuracy ("bf16x3", see mnc_fc_bf16x3 and
 * mnc_amd/csrc/conv_sw.hip; BASELINE.json configs[2] "bf16 convs via MFMA").  Activations fp32 c8 in and out at this entry point
 * (packed forms: "Reduced-precision 3x3 convolutions" below); d_w_packed comes from mnc_pack_conv3x3_bf16x3 =
 * mnc_pack_conv3x3_lowp(mode 0), mnc_conv3x3_lowp_weight_bytes(0, Cout, Cin) bytes.  Cin%8==0, Cout%32==0. */
MNC_API int mnc_pack_conv3x3_bf16x3(mnc_ctx* ctx, const float* d_oihw, void* d_packed, int Cout, int Cin);
MNC_API int mnc_conv3x3_bf16x3(mnc_ctx* ctx, const float* d_in_c8, const void* d_w_packed, const float* d_bias,
                               float* d_out_c8, int H, int W, int Cin, int Cout, int relu);
/* The same convolution (fp32 in, fp32 out, fp32 MFMA) by Winograd's minimal filtering F(2x2, 3x3): 16 instead of 36 multiplies
 * per (input channel, output channel, 2x2 output tile) -- 2.25x fewer matrix-pipe cycles (mnc_amd/csrc/conv_wino.hip).  All
 * transform coefficients are 0, +-1, +-1/2: input / output transforms are exact fp32 additions, the filter transform is evaluated
 * in double and rounded once; results agree with mnc_conv3x3 to fp32 rounding (not bit for bit: different summation order).
 * d_w_packed from mnc_pack_conv3x3_wino: Caffe [Cout][Cin][3][3] -> [Cin/8][Cout/32][2][32][68] floats (Cin*Cout*17 floats). */
MNC_API int mnc_pack_conv3x3_wino(mnc_ctx* ctx, const float* d_oihw, float* d_packed, int Cout, int Cin);
MNC_API int mnc_conv3x3_wino(mnc_ctx* ctx, const float* d_in_c8, const float* d_w_packed, const float* d_bias, float* d_out_c8,
                             int H, int W, int Cin, int Cout, int relu);
/* The same followed by the Pooling MAX 2x2 stride 2 of the trunk (test.prototxt:69-79, 130-140, 216-226, 302-312) in the kernel's
 * epilogue: a 2x2 Winograd output tile IS a pooling window, so the pooled value is the maximum of a lane's own outputs and the
 * full-resolution tensor never reaches HBM.  d_out_pooled_c8: [Cout/8][ceil(H/2)][ceil(W/2)][8] (Caffe's ceil output size). */
MNC_API int mnc_conv3x3_wino_pool(mnc_ctx* ctx, const float* d_in_c8, const float* d_w_packed, const float* d_bias,
                                  float* d_out_pooled_c8, int H, int W, int Cin, int Cout, int relu);
/* The same convolution by Winograd's F(4x4, 3x3) (round 4; mnc_amd/csrc/conv_wino4.hip): 36 multiplies per (input channel, output
 * channel, 4x4 output tile) = 2.25 per output against F(2x2)'s 4 and the direct form's 9.  Fused: input transform, the 36 channel
 * contractions (v_mfma_f32_16x16x4_f32) and the output transform run in one kernel; four-wave workgroups (32 channels x 8 x 64
 * pixels) with half of a CU's LDS each, two per CU; the two waves of a tile row split the 36 positions (half of the packed-fp32
 * input transform each) and exchange partial output sums through LDS in the epilogue.  The transforms carry the coefficients 2, 4, 5, 8 and 1/6, 1/12, 1/24 (filter side, evaluated in double,
 * rounded once): rounding error ~1e-5 of the output range at 512 input channels (F(2x2): ~1e-6; both inside the kernels' 1e-4
 * bar).  d_w_packed from mnc_pack_conv3x3_wino4: Caffe [Cout][Cin][3][3] -> [Cin/8][Cout/32][2][2][64][36] floats (Cin*Cout*36 floats).
 * Cin%8==0, Cout%32==0; the input tensor and the packed weights each below 2 GB (32-bit buffer offsets; beyond that mnc_conv3x3_wino).  _pool: the following Pooling MAX 2x2/2 in the epilogue (a 4x4 tile is four windows). */
MNC_API int mnc_pack_conv3x3_wino4(mnc_ctx* ctx, const float* d_oihw, float* d_packed, int Cout, int Cin);
MNC_API int mnc_conv3x3_wino4(mnc_ctx* ctx, const float* d_in_c8, const float* d_w_packed, const float* d_bias, float* d_out_c8,
                              int H, int W, int Cin, int Cout, int relu);
MNC_API int mnc_conv3x3_wino4_pool(mnc_ctx* ctx, const float* d_in_c8, const float* d_w_packed, const float* d_bias,
                                   float* d_out_pooled_c8, int H, int W, int Cin, int Cout, int relu);
/* F(4x4, 3x3) unfused (mnc_amd/csrc/conv_wino4_split.hip): input transform c8 -> V[36][tiles][Cin], the 36 transform positions as one
 * batched InnerProduct launch (mnc_fc_batch's kernel: tile = row, output channel = column, K = Cin) -> M[36][tiles][Cout], output
 * transform + bias (+ ReLU, _pool: + the following Pooling MAX 2x2/2) -> c8.  For the small 512-channel maps, which the fused kernel
 * has to cut into K ranges.  Same arithmetic as mnc_conv3x3_wino4 up to the order of the channel sum.  V and M (36/16 floats per
 * input and output value) live in d_ws, mnc_conv3x3_wino4_split_ws_bytes(H, W, Cin, Cout) bytes of the caller's.  d_w_split from
 * mnc_pack_conv3x3_wino4_split: Caffe [Cout][Cin][3][3] -> [36][Cout][Cin] floats (G g G^T in double, rounded once).
 * Cin%32==0, Cout%32==0 (_ws_bytes: 0 for a shape the split form does not take).  _selected: 1 where the context's tuning value
 * WINO_SPLIT moves this layer of a net to the split form (0 never, 1 the throughput plan's choice, 2 every supported layer) -- every
 * executor of a graph asks it, so that all of them run the same kernels. */
MNC_API int mnc_pack_conv3x3_wino4_split(mnc_ctx* ctx, const float* d_oihw, float* d_packed, int Cout, int Cin);
MNC_API size_t mnc_conv3x3_wino4_split_ws_bytes(int H, int W, int Cin, int Cout);
MNC_API int mnc_conv3x3_wino4_split_selected(mnc_ctx* ctx, int H, int W, int Cin, int Cout);
MNC_API int mnc_conv3x3_wino4_split(mnc_ctx* ctx, const float* d_in_c8, const float* d_w_split, const float* d_bias, float* d_out_c8,
                                    void* d_ws, int H, int W, int Cin, int Cout, int relu);
MNC_API int mnc_conv3x3_wino4_split_pool(mnc_ctx* ctx, const float* d_in_c8, const float* d_w_split, const float* d_bias,
                                         float* d_out_pooled_c8, void* d_ws, int H, int W, int Cin, int Cout, int relu);
/* Pooling MAX 2x2 stride 2 with Caffe's ceil output size (test.prototxt:69-79,...): c8 [C/8][H][W][8] ->
 * [C/8][OH][OW][8], OH = ceil((H-2)/2)+1. */
MNC_API int mnc_maxpool2_c8(mnc_ctx* ctx, const float* d_in, float* d_out, int C, int H, int W);
/* rpn_cls_score / rpn_bbox_pred (test.prototxt:413-439): 1x1 conv c8 -> NCHW [Cout][H][W], weight [Cout][Cin]. */
MNC_API int mnc_conv1x1_to_nchw(mnc_ctx* ctx, const float* d_in_c8, const float* d_w, const float* d_bias,
                                float* d_out_nchw, int H, int W, int Cin, int Cout);
/* Reshape(0,2,-1,0) -> Softmax(axis 1) -> Reshape(0,18,-1,0) (test.prototxt:440-462): pairs channel a with A+a. */
MNC_API int mnc_rpn_softmax(mnc_ctx* ctx, const float* d_score_nchw, float* d_prob_nchw, int A, int H, int W);
/* rpn_cls_score + rpn_bbox_pred + the softmax above in ONE launch (test.prototxt:413-462): d_w = [2A cls rows | 4A bbox rows] x
 * [Cin] (the two layers' weights concatenated, biases likewise), d_score = the 6A score planes (NCHW: the first 2A are
 * rpn_cls_score, the last 4A rpn_bbox_pred), d_prob = the 2A probability planes.  The same bits as mnc_conv1x1_to_nchw on the
 * concatenated weights followed by mnc_rpn_softmax(A). */
MNC_API int mnc_rpn_heads(mnc_ctx* ctx, const float* d_in_c8, const float* d_w, const float* d_bias, float* d_score_nchw,
                          float* d_prob_nchw, int H, int W, int Cin, int A);
/* ROIWarping (test.prototxt:479-492, 809-820) per oracle/SPEC.md section 1, c8 feature -> [R][PH][PW][C].
 * pool2 != 0 fuses the following Pooling MAX 2x2/2 (test.prototxt:494-505): the warp is evaluated at
 * 2PH x 2PW and max-reduced, so the 28x28 "premax" tensor never reaches HBM. */
MNC_API int mnc_roi_warp(mnc_ctx* ctx, const float* d_feat_c8, int C, int H, int W, const float* d_rois, int R,
                         int PH, int PW, float spatial_scale, int pool2, float* d_out_rhwc);
/* ---- general convolution / pooling / residual ops (graphs beyond VGG-16, e.g. a ResNet-50 trunk;
 * BASELINE.json configs[4]).  Public BVLC Caffe semantics (convolution_param / pooling_param / eltwise_param); there is no
 * such model in the reference repository. ---- */
/* Caffe conv weight [Cout][Cin][KH][KW] -> [KH*KW][Cin/8][Cout][8] for mnc_conv2d.  Cin%8==0, Cout%8==0; same element count. */
MNC_API int mnc_pack_conv_weights(mnc_ctx* ctx, const float* d_oihw, float* d_packed, int Cout, int Cin, int KH, int KW);
/* Convolution, any kernel / stride / pad, c8 -> c8 ([Cout/8][OH][OW][8], OH = (H + 2 pad - KH)/stride + 1), fp32 MFMA implicit
 * GEMM: out = conv(in) + bias (+ d_residual, same layout as out, may be NULL) (+ ReLU).  A BatchNorm + Scale pair behind the
 * convolution is folded into the weights and bias by the caller. */
MNC_API int mnc_conv2d(mnc_ctx* ctx, const float* d_in_c8, const float* d_w_packed, const float* d_bias,
                       const float* d_residual_c8, float* d_out_c8, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                       int pad, int relu);
/* "f16" math mode of mnc_conv2d: activations rounded to fp16 while staged, weights from mnc_pack_conv_weights_f16
 * ([KH*KW][ceil(Cin/32)][Cout][32] halves, channel groups zero-padded: ceil(Cin/32)*32*Cout*KH*KW*2 bytes), fp32 accumulate,
 * same epilogue. */
MNC_API int mnc_pack_conv_weights_f16(mnc_ctx* ctx, const float* d_oihw, void* d_packed, int Cout, int Cin, int KH, int KW);
MNC_API int mnc_conv2d_f16(mnc_ctx* ctx, const float* d_in_c8, const void* d_w_packed, const float* d_bias,
                           const float* d_residual_c8, float* d_out_c8, int H, int W, int Cin, int Cout, int KH, int KW,
                           int stride, int pad, int relu);
/* 1x1 convolution, stride 1 or 2, no padding, as a plain GEMM (csrc/conv1x1.hip): the c8 layout is already the MFMA B
 * fragment order, so both operands go global -> registers -> matrix pipe with no LDS staging.  Same epilogue as mnc_conv2d
 * (+ bias, + residual, ReLU).  Weights from mnc_pack_conv1x1: Caffe [Cout][Cin] fp32 -> A-fragment order
 * [K-steps][ceil(Cout/32)][64 lanes] x 16 bytes (f16 != 0: halves, K-step 16, Cin%16==0; else fp32, K-step 8):
 * Cin * ceil(Cout/32)*32 * (f16 ? 2 : 4) bytes.
 * mnc_conv1x1: fp32 c8 in / residual / out on the fp32 matrix pipe.
 * mnc_conv1x1_f16_pk ("f16" math mode): d_in is the packed fp16 c8 tensor ([C/8][H][W][8] halves, see "2-byte activation
 * tensors" below); d_out packed fp16 (out_packed != 0; nearest-even rounding of the fp32 result) or fp32 c8; d_residual
 * (may be NULL) packed fp16 (res_packed != 0) or fp32 c8; fp32 accumulate. */
MNC_API int mnc_pack_conv1x1(mnc_ctx* ctx, const float* d_w, void* d_packed, int Cout, int Cin, int f16);
MNC_API int mnc_conv1x1(mnc_ctx* ctx, const float* d_in_c8, const void* d_w_packed, const float* d_bias,
                        const float* d_residual_c8, float* d_out_c8, int H, int W, int Cin, int Cout, int stride, int relu);
MNC_API int mnc_conv1x1_f16_pk(mnc_ctx* ctx, const void* d_in_pk, const void* d_w_packed, const float* d_bias,
                               const void* d_residual, void* d_out, int H, int W, int Cin, int Cout, int stride, int relu,
                               int res_packed, int out_packed);
/* First convolution of a 3-channel NCHW input blob (ResNet conv1 7x7/2 pad 3): weights [Cout][3][K][K] as in Caffe,
 * + bias (+ ReLU) -> c8.  Cout%16==0.  mnc_conv_stem_c3_fmt: out_packed != 0 writes the packed fp16 c8 tensor instead. */
MNC_API int mnc_conv_stem_c3(mnc_ctx* ctx, const float* d_in_nchw, const float* d_w_oihw, const float* d_bias, float* d_out_c8,
                             int H, int W, int Cout, int K, int stride, int pad, int relu);
MNC_API int mnc_conv_stem_c3_fmt(mnc_ctx* ctx, const float* d_in_nchw, const float* d_w_oihw, const float* d_bias, void* d_out,
                                 int H, int W, int Cout, int K, int stride, int pad, int relu, int out_packed);
/* "f16" math mode of the stem: the same convolution on the fp16 matrix pipe (csrc/conv_gen.hip: the kernel rows padded to 8 taps,
 * so a lane's 8 K-values are 8 consecutive input pixels read straight from the NCHW blob; weights in registers).  Input rounded
 * to fp16 in registers, weights once by mnc_pack_conv_stem_f16 ([ceil(3K/2)][Cout/32][64] x 16 bytes), fp32 accumulate; output
 * fp32 c8 or packed fp16 c8.  K = 3, 5 or 7; Cout%32==0. */
MNC_API int mnc_pack_conv_stem_f16(mnc_ctx* ctx, const float* d_w_oihw, void* d_packed, int Cout, int K);
MNC_API int mnc_conv_stem_f16(mnc_ctx* ctx, const float* d_in_nchw, const void* d_w_packed, const float* d_bias, void* d_out, int H,
                              int W, int Cout, int K, int stride, int pad, int relu, int out_packed);
/* Pooling MAX with any kernel / stride / pad on a c8 map; Caffe's ceil output size, windows clipped to the image.
 * mnc_maxpool_c8_f16: the same on the packed fp16 c8 tensor (max commutes with the rounding: bit for bit the fp16 form of
 * the fp32 result). */
MNC_API int mnc_maxpool_c8(mnc_ctx* ctx, const float* d_in, float* d_out, int C, int H, int W, int K, int stride, int pad);
MNC_API int mnc_maxpool_c8_f16(mnc_ctx* ctx, const void* d_in, void* d_out, int C, int H, int W, int K, int stride, int pad);
/* Eltwise SUM of two tensors of the same layout (+ ReLU): d_out[i] = d_a[i] + d_b[i]. */
MNC_API int mnc_add(mnc_ctx* ctx, const float* d_a, const float* d_b, float* d_out, size_t n, int relu);
/* prep_im_for_blob (lib/utils/blob.py:36-50) and one level of prep_im_for_blob_cfm (:53-85) on the device: a uint8 BGR image
 * [H][W][3] -> float32 planes [3][PH][PW] holding (pixel - mean) resized with cv2.resize's INTER_LINEAR rule to OH x OW and
 * zero-padded to the blob's PH x PW (im_list_to_blob, :17-33).  `means` = 3 host doubles (cfg.PIXEL_MEANS).  The resize
 * taps come from the caller (the host function that the numpy path uses): d_x0[OW] / d_y0[OH] first source index,
 * d_ax[OW] / d_ay[OH] fraction of the next one; the second index is min(first + 1, size - 1).  Bit-identical to the host
 * path (tests/test_gpu_ops.py). */
MNC_API int mnc_prep_image(mnc_ctx* ctx, const unsigned char* d_bgr_hwc, int H, int W, const double* means_host,
                           const int* d_x0, const float* d_ax, int OW, const int* d_y0, const float* d_ay, int OH,
                           float* d_out_chw, int PH, int PW);
/* ROIPooling (models/VGG16/cfm/test.prototxt:397-407 7x7, :446-456 14x14; the Fast R-CNN layer of the absent caffe-mnc
 * submodule, restated in oracle/SPEC.md section 4): max over the integer bins of round(roi * spatial_scale).  The feature
 * is a batch of N c8 images [N][C/8][H][W][8] (CFM feeds an image pyramid, lib/caffeWrapper/TesterWrapper.py:371-399);
 * rois are [R][5] = (batch index, x1, y1, x2, y2); output [R][PH][PW][C].  Empty bins give 0. */
MNC_API int mnc_roi_pool(mnc_ctx* ctx, const float* d_feat_c8, int N, int C, int H, int W, const float* d_rois, int R,
                         int PH, int PW, float spatial_scale, float* d_out_rhwc);
/* Pooling MAX 2x2/2 on per-RoI features [R][PH][PW][C] -> [R][PH/2][PW/2][C] (test.prototxt:571-582,...). */
MNC_API int mnc_maxpool2_rhwc(mnc_ctx* ctx, const float* d_in, float* d_out, int R, int PH, int PW, int C);
/* MaskResize (test.prototxt:558-567) per SPEC.md section 2: [R][IH][IW] -> [R][OH][OW]. */
MNC_API int mnc_mask_resize(mnc_ctx* ctx, const float* d_in, float* d_out, int R, int IH, int IW, int OH, int OW);
/* MaskPooling (test.prototxt:631-637) per SPEC.md section 3: feat[R][PH][PW][C] * mask[R][PH][PW].
 * pool2 != 0 fuses the following Pooling MAX 2x2/2 (test.prototxt:639-650). */
MNC_API int mnc_mask_pool(mnc_ctx* ctx, const float* d_feat, const float* d_mask, float* d_out, int R, int PH,
                          int PW, int C, int pool2);
/* InnerProduct (+ReLU / +Sigmoid): out[M][N] = act(A[M][K] . W[N][K]^T + bias[N]).  fp32 MFMA, split-K chosen
 * internally; d_out may be a column slice of a wider matrix (ldc >= N) so Concat (test.prototxt:700-709) is free.
 * act: 0 none, 1 ReLU, 2 sigmoid. */
MNC_API int mnc_fc(mnc_ctx* ctx, const float* d_a, const float* d_w, const float* d_bias, float* d_out, int M,
                   int N, int K, int ldc, int act);
/* Two InnerProducts of ONE shape in one launch: out_i = act(a_i . w_i^T + bias_i), i = 0, 1 (the box and the mask branch of a head
 * stage: fc6 + fc6_mask, fc7 + fc7_mask, test.prototxt:584-627 / :652-696).  Twice the column tiles fill the chip with half as
 * many K ranges: longer ranges per workgroup, half the partial sums.  Shapes mnc_fc would not give to its 320-row kernel in one
 * launch run as two mnc_fc calls.  The paired launch groups the partial sums differently from mnc_fc (results differ in the last
 * bits): every executor of a graph pairs the same layers. */
MNC_API int mnc_fc_pair(mnc_ctx* ctx, const float* d_a0, const float* d_w0, const float* d_bias0, float* d_out0, const float* d_a1,
                        const float* d_w1, const float* d_bias1, float* d_out1, int M, int N, int K, int ldc, int act);
/* B InnerProducts of ONE shape at constant strides in one launch: out_b[M][N] = a_b . w_b^T with a_b = d_a + b * stride_a floats (and
 * d_w, d_out alike), b = 0 .. B-1; no bias, no activation, K never cut.  Always the eight-wave fp32 LDS-DMA kernel, whatever the
 * size of one product (the 36 transform positions of mnc_conv3x3_wino4_split).  K%32==0, operands and strides 16-byte aligned.
 * Every output's K order is that kernel's: the same bits as B calls with B = 1. */
MNC_API int mnc_fc_batch(mnc_ctx* ctx, const float* d_a, long stride_a, const float* d_w, long stride_w, float* d_out,
                         long stride_out, int B, int M, int N, int K, int ldc);
/* InnerProduct on the bf16 matrix pipe with fp32-class accuracy ("bf16x3": every operand split into hi + lo bf16, product =
 * a_lo*b_hi + a_hi*b_lo + a_hi*b_hi, fp32 accumulate; relative error ~1e-5 per product, see mnc_amd/csrc/gemm_x3.hip).
 * d_w_packed comes from mnc_pack_fc_bf16x3: fp32 [N][K] -> stage-major tiles [ceil(N/128)][K/32][128][(hi x8 | lo x8) x 4] bf16,
 * ceil(N/128)*128*K*4 bytes (rows past N are zero), K%32==0 -- the weight panel a workgroup needs for one K stage is one
 * contiguous 16 KB.  Activations are fp32 at the interface (split per call into the context's scratch arena).
 * Same contract as mnc_fc otherwise. */
MNC_API int mnc_pack_fc_bf16x3(mnc_ctx* ctx, const float* d_w, void* d_packed, int N, int K);
MNC_API int mnc_fc_bf16x3(mnc_ctx* ctx, const float* d_a, const void* d_w_packed, const float* d_bias, float* d_out, int M,
                          int N, int K, int ldc, int act);
/* Reduced-precision 3x3 convolutions (round 6: csrc/conv_sw.hip -- sliding-window implicit GEMM on 2-byte activation planes, every
 * operand by LDS-DMA, K ranges summed inside the workgroup; models/VGG16/mnc_5stage/test.prototxt:41-412).  mode: 0 = bf16x3 (split
 * precision, above), 1 = f16 (one fp16 product per term on v_mfma_f32_32x32x16_f16, operands rounded to nearest even, fp32
 * accumulation), 2 = bf16 (the same with bf16: BASELINE configs[2] "bf16 convs via MFMA" as written; ~4e-3 of a layer's range per
 * layer, measured and recorded, outside the 1e-3 bar -- bf16x3 is the bf16-pipe mode that keeps it).
 * Packed weights: mnc_pack_conv3x3_lowp (and the per-mode names of rounds 1-5, which call it) writes
 *   [ceil(Cin/16)][Cout/32][planes][9 taps][32 channels] x 16 B (8 two-byte values)
 * planes = the two 8-channel halves of the 16-channel block (f16 / bf16), or hi of each half then lo of each half (bf16x3: hi =
 * rne(w), lo = rne(w - hi)); channels past Cin are zero.  mnc_conv3x3_lowp_weight_bytes(mode, Cout, Cin) is the buffer's size:
 * ceil(Cin/16) * (Cout/32) * (mode == 0 ? 4 : 2) * 4608 bytes.
 * Packed 2-byte activations between MFMA layers.  A c8 tensor [C/8][H][W][8] is kept as
 *   bf16x3:  [C/8][H][W][hi x8 | lo x8] bf16 -- the split the kernels apply to an fp32 value (hi = truncation, lo = the
 *            remainder rounded half-up), two 2-byte planes interleaved per pixel, 32 B per pixel and channel block;
 *   f16:     [C/8][H][W][8] fp16 (round to nearest even), 16 B per pixel and channel block;
 *   bf16:    [C/8][H][W][8] bf16 (round to nearest even), 16 B (round 6).
 * The convolution multiplies PACKED inputs; an fp32 c8 input (in_packed = 0, and the fp32-tensor entry points) is packed into the
 * context's scratch arena first.  A producer's epilogue applies exactly that packing to its fp32 result, so a packed chain gives bit
 * for bit the results of the fp32-tensor chain (test.prototxt:41-412 is such a chain: conv1_1 .. conv5_3 with four MAX 2x2/2 pools).
 * mnc_conv3x3_lowp writes d_out_packed and / or d_out_c8 (fp32 c8); a null one is not written (conv5_3 feeds the RPN convolution
 * packed and the RoI warps in fp32: test.prototxt:395-424, 479-492).  The *_pk forms select one format per side.
 * mnc_maxpool2_c8_{bf16x3,f16,bf16}: Pooling MAX 2x2/2 (ceil output size) on the packed form; mnc_act_pack / mnc_act_unpack:
 * fp32 c8 <-> packed, n = element count (multiple of 8), f16 = the mode number (0 bf16x3, 1 f16, 2 bf16). */
MNC_API size_t mnc_conv3x3_lowp_weight_bytes(int mode, int Cout, int Cin);
MNC_API int mnc_pack_conv3x3_lowp(mnc_ctx* ctx, int mode, const float* d_oihw, void* d_packed, int Cout, int Cin);
MNC_API int mnc_conv3x3_lowp(mnc_ctx* ctx, int mode, const void* d_in_packed, const void* d_w_packed, const float* d_bias,
                             void* d_out_packed, float* d_out_c8, int H, int W, int Cin, int Cout, int relu);
/* The same convolution with the following Pooling MAX 2x2/2 (Caffe's ceil output size) folded into the epilogue: writes only the
 * pooled tensor [Cout/8][ceil(H/2)][ceil(W/2)] in the packed form -- bit for bit mnc_maxpool2_c8_* of the unpooled packed output
 * (conv1_2 / conv2_2 / conv3_3 / conv4_3 + pool1..4: test.prototxt:61-92, 117-148, 193-232, 277-316).  Cout % 64 == 0. */
MNC_API int mnc_conv3x3_lowp_pool(mnc_ctx* ctx, int mode, const void* d_in_packed, const void* d_w_packed, const float* d_bias,
                                  void* d_out_pooled_packed, int H, int W, int Cin, int Cout, int relu);
MNC_API int mnc_pack_conv3x3_f16(mnc_ctx* ctx, const float* d_oihw, void* d_packed, int Cout, int Cin);
MNC_API int mnc_pack_conv3x3_bf16(mnc_ctx* ctx, const float* d_oihw, void* d_packed, int Cout, int Cin);
MNC_API int mnc_conv3x3_bf16(mnc_ctx* ctx, const float* d_in_c8, const void* d_w_packed, const float* d_bias, float* d_out_c8,
                             int H, int W, int Cin, int Cout, int relu);
MNC_API int mnc_conv3x3_f16(mnc_ctx* ctx, const float* d_in_c8, const void* d_w_packed, const float* d_bias, float* d_out_c8,
                            int H, int W, int Cin, int Cout, int relu);
MNC_API int mnc_conv3x3_bf16x3_pk(mnc_ctx* ctx, const void* d_in, const void* d_w_packed, const float* d_bias, void* d_out,
                                  int H, int W, int Cin, int Cout, int relu, int in_packed, int out_packed);
MNC_API int mnc_conv3x3_f16_pk(mnc_ctx* ctx, const void* d_in, const void* d_w_packed, const float* d_bias, void* d_out,
                               int H, int W, int Cin, int Cout, int relu, int in_packed, int out_packed);
MNC_API int mnc_conv3x3_bf16_pk(mnc_ctx* ctx, const void* d_in, const void* d_w_packed, const float* d_bias, void* d_out,
                                int H, int W, int Cin, int Cout, int relu, int in_packed, int out_packed);
/* conv1_1 (mnc_conv3x3_c3) writing the packed form: out_fmt 0 = fp32 c8, 1 = bf16x3 packed, 2 = fp16 packed, 3 = bf16 packed */
MNC_API int mnc_conv3x3_c3_fmt(mnc_ctx* ctx, const float* d_in_nchw, const float* d_w_oihw, const float* d_bias, void* d_out,
                               int H, int W, int Cout, int relu, int out_fmt);
MNC_API int mnc_maxpool2_c8_bf16x3(mnc_ctx* ctx, const void* d_in, void* d_out, int C, int H, int W);
MNC_API int mnc_maxpool2_c8_f16(mnc_ctx* ctx, const void* d_in, void* d_out, int C, int H, int W);
MNC_API int mnc_maxpool2_c8_bf16(mnc_ctx* ctx, const void* d_in, void* d_out, int C, int H, int W);
MNC_API int mnc_act_pack(mnc_ctx* ctx, const float* d_c8, void* d_packed, size_t n, int f16);
MNC_API int mnc_act_unpack(mnc_ctx* ctx, const void* d_packed, float* d_c8, size_t n, int f16);
/* "f16" math mode (BASELINE.json configs[4] names fp16): InnerProduct with both operands rounded to IEEE fp16 (nearest even)
 * and fp32 accumulation on v_mfma_f32_32x32x16_f16 -- one product per term, 2 bytes per value streamed instead of 4.
 * mnc_pack_fc_f16: Caffe weight [N][K] -> [ceil(N/128)][K/64][128][64] halves (bytes: ceil(N/128)*128*K*2), once at load.
 * mnc_fc_f16: same interface as mnc_fc (fp32 activations in, fp32 out); K%64==0.  Relative error vs fp32 ~3e-4 per layer. */
MNC_API int mnc_pack_fc_f16(mnc_ctx* ctx, const float* d_w, void* d_packed, int N, int K);
/* The same InnerProduct in plain bf16 (nearest even, one product per term; the "bf16" math mode): mnc_fc_f16's layout and interface. */
MNC_API int mnc_pack_fc_bf16(mnc_ctx* ctx, const float* d_w, void* d_packed, int N, int K);
MNC_API int mnc_fc_bf16(mnc_ctx* ctx, const float* d_a, const void* d_w_packed, const float* d_bias, float* d_out, int M, int N,
                        int K, int ldc, int act);
MNC_API int mnc_fc_f16(mnc_ctx* ctx, const float* d_a, const void* d_w_packed, const float* d_bias, float* d_out, int M, int N,
                       int K, int ldc, int act);
/* Two reduced-precision InnerProducts of one shape as ONE launch (round 6; mode 1 = fp16, 2 = plain bf16): the box and the mask
 * branch of a head stage (fc6 + fc6_mask, fc7 + fc7_mask; test.prototxt:584-627, 652-696) -- mnc_fc_pair's idea on the 256-column
 * LDS-DMA kernel: twice the column tiles fill the chip with half the K ranges (half the partial sums: 2 x 39 MB instead of 2 x 79 at
 * fc6 / 300 RoIs).  Per product exactly the arguments of mnc_fc_f16_ex (one of d_a / d_a_sm; m_stride rows per stage of the
 * stage-major inputs; an optional second output in the next InnerProduct's form).  mode 0 (split bf16) and shapes the paired kernel
 * does not take (it needs 160 < M <= 320, N % 256 == 0, >= 8 stages per K range) run as the two single calls.  The paired launch
 * groups the partial sums differently from two single calls: every executor of a graph pairs the same layers. */
MNC_API int mnc_fc_lowp_pair(mnc_ctx* ctx, int mode, const float* d_a0, const void* d_a_sm0, const float* d_a1, const void* d_a_sm1,
                             int m_stride, const void* d_w0, const void* d_w1, const float* d_bias0, const float* d_bias1,
                             float* d_out0, float* d_out1, int M, int N, int K, int ldc, int act, void* d_out_sm0, void* d_out_sm1,
                             int out_sm_fmt);
/* ---- InnerProduct activations already in the reduced-precision kernels' own form ----
 * mnc_fc_bf16x3 / mnc_fc_f16 multiply the activations from a stage-major 2-byte tensor, which they otherwise make from the fp32
 * rows on every call (an elementwise pass over M x K: 0.2 ms per image at 300 RoIs, 0.75 ms at 1000 RoIs x 1024 channels):
 *   fmt 1 (f16)    [K/64][M][64] halves (nearest even of the fp32 value),                 M*K*2 bytes
 *   fmt 2 (bf16x3) [K/32][M][4 x (hi x8 | lo x8)] bf16 (x = hi + lo, both nearest even), M*K*4 bytes
 * with row r of the fp32 tensor [M][K] at row r of every stage.  The producers of the per-RoI tensors write this form next to the
 * fp32 tensor in their epilogue (the *_sm entry points below: d_sm may be NULL / sm_fmt 0 = no second output; values are bit for
 * bit what mnc_fc_pack_act makes of the fp32 output), and mnc_fc_{bf16x3,f16}_pre take it: m_stride = rows of the stage-major
 * tensor (>= M: a call may multiply its first M rows), everything else as mnc_fc_*.
 *   mnc_roi_warp_sm        = mnc_roi_warp        (+ d_sm of d_out_rhwc as [R][PH*PW*C])
 *   mnc_maxpool2_rhwc_sm   = mnc_maxpool2_rhwc   (+ d_sm of d_out)
 *   mnc_mask_pool_sm       = mnc_mask_pool       (+ d_sm of d_out)
 * C%64==0 (fmt 1) / C%32==0 (fmt 2) so that an 8-channel group never straddles a stage. */
MNC_API int mnc_fc_pack_act(mnc_ctx* ctx, const float* d_a, void* d_a_sm, int M, int K, int f16);
/* Round 6.  The inverse: fp32 rows [M][K] out of a stage-major tensor (fmt 1 = fp16: the rounded values; fmt 2 = split bf16: hi + lo)
 * -- for a consumer, or the host, that needs the rows of a tensor whose producer wrote the stage-major form ONLY
 * (mnc_roi_warp_sm / mnc_box_mask_pool_ex with null fp32 outputs; mnc_amd/engine.py materialises such blobs on demand). */
MNC_API int mnc_fc_unpack_act(mnc_ctx* ctx, const void* d_a_sm, float* d_a, int M, int K, int fmt);
/* *ok = 1 when mnc_roi_warp_sm on this context (its layer conventions, its kernel choice for C channels / pool2) accepts
 * d_out_rhwc = NULL next to a stage-major output. */
MNC_API int mnc_roi_warp_sm_only_ok(mnc_ctx* ctx, int C, int pool2, int* ok);
MNC_API int mnc_fc_f16_pre(mnc_ctx* ctx, const void* d_a_sm, int m_stride, const void* d_w_packed, const float* d_bias,
                           float* d_out, int M, int N, int K, int ldc, int act);
MNC_API int mnc_fc_bf16x3_pre(mnc_ctx* ctx, const void* d_a_sm, int m_stride, const void* d_w_packed, const float* d_bias,
                              float* d_out, int M, int N, int K, int ldc, int act);
/* The general form of the two: activations as fp32 rows (d_a) or stage-major (d_a_sm, m_stride) -- exactly one non-NULL -- and,
 * optionally (d_out_sm != NULL), the result rows written a second time in the stage-major form of the NEXT reduced-precision
 * InnerProduct (out_sm_fmt 1: [N/64][M][64] halves, N%64==0; 2: split bf16, N%32==0) by the K-split reduction: fc6 -> fc7 without a
 * conversion pass.  Bit for bit mnc_fc_pack_act of d_out. */
MNC_API int mnc_fc_f16_ex(mnc_ctx* ctx, const float* d_a, const void* d_a_sm, int m_stride, const void* d_w_packed,
                          const float* d_bias, float* d_out, int M, int N, int K, int ldc, int act, void* d_out_sm, int out_sm_fmt);
MNC_API int mnc_fc_bf16x3_ex(mnc_ctx* ctx, const float* d_a, const void* d_a_sm, int m_stride, const void* d_w_packed,
                             const float* d_bias, float* d_out, int M, int N, int K, int ldc, int act, void* d_out_sm,
                             int out_sm_fmt);
/* Round 6: the plain bf16 mode's stage-major form, FORMAT 3 = format 1's layout ([K/64][M][64] 2-byte values) with the values
 * rounded to bf16 (nearest even) instead of fp16.  Written by the same producers (sm_fmt = 3: mnc_roi_warp_sm, mnc_maxpool2_rhwc_sm,
 * mnc_mask_pool_sm, mnc_box_mask_pool[_ex] -- whose stage-major input may be format 3 too, with format-3 outputs -- and the K-split
 * reduction of an InnerProduct, out_sm_fmt = 3), by mnc_fc_pack_act(.., f16 = 2), read by mnc_fc_bf16_ex / mnc_fc_lowp_pair(mode 2)
 * and mnc_fc_unpack_act(.., fmt = 3). */
MNC_API int mnc_fc_bf16_ex(mnc_ctx* ctx, const float* d_a, const void* d_a_sm, int m_stride, const void* d_w_packed,
                           const float* d_bias, float* d_out, int M, int N, int K, int ldc, int act, void* d_out_sm, int out_sm_fmt);
/* ---- "f8" math mode: InnerProduct on OCP e4m3fn operands (csrc/gemm_f8.hip) ----
 * Both operands as e4m3fn codes (NOT gfx942's e4m3fnuz) with ONE power-of-two scale 2^e per row, fp32 accumulation on
 * v_mfma_scale_f32_32x32x64_f8f6f4 with both hardware block scales at 1.0, the row exponents applied after all K ranges are summed:
 *   out[m][n] = act(ldexp(sum_k dec(qa[m][k]) * dec(qw[n][k]), ea[m] + ew[n]) + bias[n]).
 * Row rule: amax = f * 2^p (f in [0.5, 1)), e = p - 9 when f <= 0.875, else p - 8, clamped to [-64, 64], 0 for a zero row; codes =
 * e4m3(x * 2^-e), nearest even, saturating at +-448.  amax is taken over the row's finite values: an infinity saturates at +-448, a
 * NaN stays NaN (0x7F | sign).  mnc_amd/f8.py states all of it in numpy; the kernels follow it bit for bit
 * except for the fp32 summation order, which is fixed (the same bits from run to run).  Like "bf16" the mode claims no parity bar.
 * Products over fewer than four stages (K < 512; none in a net) decode the codes to fp16, exactly, and multiply on the fp16 MFMA: the
 * scaled instruction drops products 2^16 below the largest of their K group, which an fp32 summation of so few terms would not.
 * K%128==0 everywhere; anything else, a null operand and the like are refused with MNC_ERR_INVALID before any launch.
 *   mnc_pack_fc_f8      Caffe weight [N][K] fp32 -> codes [ceil(N/256)][K/128][256][128] (mnc_pack_fc_f8_bytes(N, K) bytes; rows
 *                       past N are zero codes) and d_wexp, ceil(N/256)*256 int32 row exponents.  Once at load.
 *   mnc_fc_pack_act_f8  the activation quantiser: M rows from fp32 rows [M][K] (d_a) OR from the fp16 stage-major format-1 panel
 *                       [K/64][m_stride][64] (d_a_sm) -- exactly one non-NULL -- -> codes [K/128][M][128] (M*K bytes), d_aexp M int32.
 *   mnc_fc_f8           mnc_fc's interface: quantises the fp32 rows in the context's scratch and multiplies.
 *   mnc_fc_f8_ex        activations in either form (as mnc_fc_f16_ex); optionally the result rows a second time as fp16 in the
 *                       stage-major format 1 (out_sm_fmt == 1, N%64==0) the next InnerProduct reads; bit for bit
 *                       mnc_fc_pack_act(d_out, f16 = 1) (dense rows, ldc == N, for that comparison; any ldc is accepted).
 *   mnc_fc_f8_pre       activations already quantised by mnc_fc_pack_act_f8 (m_stride = rows per stage of d_q). */
MNC_API size_t mnc_pack_fc_f8_bytes(int N, int K);
MNC_API int mnc_pack_fc_f8(mnc_ctx* ctx, const float* d_w, void* d_packed, int* d_wexp, int N, int K);
MNC_API int mnc_fc_pack_act_f8(mnc_ctx* ctx, const float* d_a, const void* d_a_sm, int m_stride, void* d_q, int* d_aexp, int M, int K);
MNC_API int mnc_fc_f8(mnc_ctx* ctx, const float* d_a, const void* d_w_packed, const int* d_wexp, const float* d_bias, float* d_out,
                      int M, int N, int K, int ldc, int act);
MNC_API int mnc_fc_f8_ex(mnc_ctx* ctx, const float* d_a, const void* d_a_sm, int m_stride, const void* d_w_packed, const int* d_wexp,
                         const float* d_bias, float* d_out, int M, int N, int K, int ldc, int act, void* d_out_sm, int out_sm_fmt);
MNC_API int mnc_fc_f8_pre(mnc_ctx* ctx, const void* d_q, const int* d_aexp, int m_stride, const void* d_w_packed, const int* d_wexp,
                          const float* d_bias, float* d_out, int M, int N, int K, int ldc, int act);
MNC_API int mnc_roi_warp_sm(mnc_ctx* ctx, const float* d_feat_c8, int C, int H, int W, const float* d_rois, int R, int PH, int PW,
                            float spatial_scale, int pool2, float* d_out_rhwc, void* d_sm, int sm_fmt);
MNC_API int mnc_maxpool2_rhwc_sm(mnc_ctx* ctx, const float* d_in, float* d_out, int R, int PH, int PW, int C, void* d_sm,
                                 int sm_fmt);
MNC_API int mnc_mask_pool_sm(mnc_ctx* ctx, const float* d_feat, const float* d_mask, float* d_out, int R, int PH, int PW, int C,
                             int pool2, void* d_sm, int sm_fmt);
/* The box-feature Pooling (MAX 2x2/2 of the per-RoI tensor, test.prototxt:571-582) and MaskPooling + its Pooling (:631-650) of
 * the SAME tensor in one pass: d_box_out = mnc_maxpool2_rhwc(d_feat), d_mask_out = mnc_mask_pool(d_feat, d_mask, pool2 = 1), bit
 * for bit; d_feat is read once instead of twice.  d_box_sm / d_mask_sm: their stage-major second outputs (both or neither). */
MNC_API int mnc_box_mask_pool(mnc_ctx* ctx, const float* d_feat, const float* d_mask, float* d_box_out, float* d_mask_out, int R,
                              int PH, int PW, int C, void* d_box_sm, void* d_mask_sm, int sm_fmt);
/* Round 6.  The same pass with (a) the fp32 outputs optional -- both null when only the stage-major ones are consumed (60 of 210 MB
 * per call at 300 RoIs x 512 channels) -- and (b) the 14x14 tensor read from its stage-major fp16 form d_feat_sm (feat_sm_fmt = 1:
 * [PH*PW*C/64][R][64] halves, what mnc_roi_warp_sm wrote for fc6_maskest) when stage-major outputs are written: 60 instead of 120 MB
 * read, and the producer need not write the fp32 tensor (mnc_roi_warp_sm accepts d_out_rhwc = NULL with a stage-major output on the
 * SPEC's convention and the launcher's own kernel choice).  d_box_sm is then the same bits as from the fp32 tensor (rounding is monotonic); d_mask_sm
 * multiplies the ROUNDED features by the mask and differs in the last fp16 bit -- every executor of a graph must pass the same
 * inputs (csrc/pipeline.hip and engine.py both pass d_feat_sm whenever the producer wrote it).  feat_sm_fmt = 2: the split-bf16 form
 * ([PH*PW*C/32][R][4][hi x8 | lo x8]; a value is hi + lo, 16 significant bits -- the box pool too may then differ in the last fp16
 * bit).  feat_sm_fmt 0, or no stage-major outputs: d_feat is read as in mnc_box_mask_pool. */
MNC_API int mnc_box_mask_pool_ex(mnc_ctx* ctx, const float* d_feat, const void* d_feat_sm, int feat_sm_fmt, const float* d_mask,
                                 float* d_box_out, float* d_mask_out, int R, int PH, int PW, int C, void* d_box_sm, void* d_mask_sm,
                                 int sm_fmt);
/* Softmax over the last axis of [M][N] (test.prototxt cls_prob / seg_cls_prob). */
MNC_API int mnc_softmax_rows(mnc_ctx* ctx, const float* d_in, float* d_out, int M, int N);
/* Same with a row stride on the input (the input may be a column slice of a merged-GEMM output). */
MNC_API int mnc_softmax_rows_ld(mnc_ctx* ctx, const float* d_in, int ld_in, float* d_out, int M, int N);
/* Stand-alone ReLU (op 1) / Sigmoid (op 2) for graphs where the activation is not fused into its producer
 * (test.prototxt:540-545 `mask_output` when run unfused).  In-place allowed. */
MNC_API int mnc_eltwise(mnc_ctx* ctx, const float* d_in, float* d_out, size_t count, int op);
/* Strided 2-D device copy of float rows (Concat, test.prototxt:700-709, when the producers could not write in place). */
MNC_API int mnc_copy2d(mnc_ctx* ctx, float* d_dst, int dst_ld, const float* d_src, int src_ld, int rows, int cols);

/* ---------------------------------------------------------------------------------------------------------------
 * Device-resident forms of the three inference-time Python layers (the Python classes in mnc_amd/lib/pylayer remain the
 * API and the path for user-defined layers; the engine substitutes these for the stock classes).
 * ------------------------------------------------------------------------------------------------------------- */
/* ProposalLayer.forward (lib/pylayer/proposal_layer.py:52-175): d_cls_prob [2A][H][W], d_bbox_pred [4A][H][W] (NCHW,
 * batch 1), anchors_host [A][4] (transform.anchors.generate_anchors as float32), im_info = (im_h, im_w, im_scale).
 * Writes d_rois [post_nms_topn][5] (rows >= the row count are zero) and returns the row count in *num_rois_host (one 4-byte
 * D2H + stream sync).  num_rois_host == NULL: fully asynchronous, the count stays on the device until mnc_proposal_count
 * (the engine launches the heads on all post_nms_topn rows meanwhile and checks the count with the outputs).
 * Candidate order is score descending by value, anchor index ascending (the reference leaves tie order to numpy's sort); +0.0
 * and -0.0 are one value and tie.  pre_nms_topn <= 0 keeps every box that passes the size filter; more than 16384 after the
 * clamp to the anchor count is MNC_ERR_INVALID.  A NaN score cannot be seen from the host: it is ordered by its bit pattern
 * (memory-safe) and the result is then unspecified. */
MNC_API int mnc_proposal(mnc_ctx* ctx, const float* d_cls_prob, const float* d_bbox_pred, int A, int H, int W,
                         const float* anchors_host, int feat_stride, float im_h, float im_w, float im_scale,
                         int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size, float* d_rois,
                         int* num_rois_host);
/* gpu_mask_voting (mnc_mask_voting above) with the inputs already on the device -- the engine's own outputs, produced on ctx's stream (no host round trip
 * between net.forward and the voting): d_boxes [n][4], d_masks [n][S][S], d_scores [n][num_classes]; outputs are host
 * arrays as above.  The library orders each class itself (order = NULL semantics). */
MNC_API int mnc_mask_voting_dev(mnc_ctx* ctx, const float* d_boxes, const float* d_masks, const float* d_scores, int n,
                                int num_classes, int mask_size, int max_per_image, float nms_thresh, float iou_thresh,
                                int image_height, int image_width, float* out_mask, int* out_box, float* out_score,
                                int* class_count, int* result_num);
/* gpu_mask_voting with inputs AND outputs on the device, fully asynchronous on ctx's stream (no host decision, no
 * synchronisation): the whole-image path's last stage, and the block the multi-GPU path gathers.
 *   d_records [record_cap][6 + S*S] float32: (x1, y1, x2, y2, score, class id 1..num_classes-1, S*S mask values) of the
 *             result rows in the reference's order (class-major, keep order); rows past the result count are zero (class 0).
 *   d_counts  [num_classes] int32: [0] = R, the number of result rows (> max_per_image only when scores tie at the global
 *             threshold; rows >= record_cap are not written), [c] = rows of class c.
 * The global threshold and the result rows (mask_transform.py:242-258) are chosen by a kernel (np.sort()[::-1] order, NaN
 * first).  Limits: n <= 4096, (num_classes-1) * min(max_per_image, n) <= 8192.  Records are bit-identical to mnc_mask_voting. */
MNC_API int mnc_vote_instances(mnc_ctx* ctx, const float* d_boxes, const float* d_masks, const float* d_scores, int n,
                               int num_classes, int mask_size, int max_per_image, float nms_thresh, float iou_thresh,
                               int image_height, int image_width, float* d_records, int record_cap, int* d_counts);
/* Voting rules of mnc_vote_instances_ex / mnc_net_set_voting: gpu_mask_voting (the default) or cpu_mask_voting
 * (cfg.TEST.USE_GPU_MASK_MERGE = False; mnc_mask_voting_image). */
#define MNC_VOTE_MV 0
#define MNC_VOTE_IMAGE 1
/* mnc_vote_instances with the voting rule chosen by `mode`: MNC_VOTE_MV is mnc_vote_instances itself (binarize_thresh unused:
 * the rule's 0.4 is compiled in, as in the reference kernel), MNC_VOTE_IMAGE is cpu_mask_voting, records bit-identical to
 * mnc_mask_voting_image.  Same record layout, counts and limits; rounded boxes with x2 < x1 or y2 < y1 (which clipped boxes
 * never give) cover no pixel. */
MNC_API int mnc_vote_instances_ex(mnc_ctx* ctx, int mode, const float* d_boxes, const float* d_masks, const float* d_scores,
                                  int n, int num_classes, int mask_size, int max_per_image, float nms_thresh, float iou_thresh,
                                  double binarize_thresh, int image_height, int image_width, float* d_records, int record_cap,
                                  int* d_counts);
/* The visualisation tail of the records of mnc_vote_instances (tools/demo.py:get_vis_dict + _convert_pred_to_image + the colour
 * map + Image.blend), everything on the device, asynchronous on ctx's stream, no host read-back.  The rows [0, min(d_counts[0],
 * record_cap)) of d_records [record_cap][6 + S*S] with (double)score >= vis_thresh are painted in record order (class-major, keep
 * order: the order get_vis_dict / _prepare_dict build) by the rule of mnc_render_instances, the class being the record's class id.
 * Unlike there, a rounded, clipped box with x2 < x1 or y2 < y1 is not an error: it covers no pixel and draws no outline, but still
 * consumes its instance id (the convention of mnc_vote_instances_ex).  Every output is optional (NULL):
 *   d_inst, d_cls            [H][W] int32 label maps
 *   d_inst_rgb, d_cls_rgb    [H][W][3] uint8, _get_voc_color_map()[label] (computed from the label's bits, no table)
 *   d_overlay_rgb            [H][W][3] uint8, PIL.Image.blend(photograph as RGB, cls_rgb, alpha): (uint8)((int)a + alpha *
 *                            ((int)b - (int)a)) in float32 with truncation, 0 <= alpha <= 1; d_bgr_hwc is the uint8 [H][W][3] BGR
 *                            photograph (NULL: a black one)
 *   d_kept                   int32, the number of rows painted
 * The colour map has 256 entries: the colour of an instance label is that of label & 255, which differs from the reference (an
 * IndexError there) only when more than 255 instances are kept -- out of reach with max_per_image <= 255 and no score ties at
 * the voting threshold (the default is 100).  Limits: mask_size <= 32, num_classes <= 256, H and W in [2, 32768]. */
MNC_API int mnc_render_records(mnc_ctx* ctx, const float* d_records, const int* d_counts, int record_cap, int num_classes,
                               int mask_size, double vis_thresh, double binarize_thresh, int H, int W,
                               const unsigned char* d_bgr_hwc, float alpha, int* d_inst, int* d_cls, unsigned char* d_inst_rgb,
                               unsigned char* d_cls_rgb, unsigned char* d_overlay_rgb, int* d_kept);
/* mnc_instance_masks of the records of mnc_vote_instances, everything on the device, asynchronous on ctx's stream, no host
 * read-back: exactly the rows mnc_render_records keeps at vis_thresh = score_thresh -- the rows [0, min(d_counts[0], record_cap))
 * of d_records with (double)score >= score_thresh -- in record order, always with clip = 1.  A first kernel (one workgroup) derives
 * the bounds, the byte sizes and their exclusive prefix; the pack kernel follows it.  As there, a rounded, clipped box with
 * x2 < x1 or y2 < y1 is not an error: it keeps its place and has no rows (area 0).
 *   *d_info   device address of [mnc_mask_head | mnc_mask_info[record_cap]], kept entries valid: ONE copy of 256 + 64 * rows bytes
 *             brings the count, bounds, offsets, areas, classes and scores down
 *   *d_bits   device address of the masks, head.bits_bytes bytes (a second copy).  d_bits == NULL: sizes only -- the first kernel
 *             alone runs, every area is 0
 * Both live in an arena of the context (in no captured graph) that holds record_cap * H * 8 * ceil(W / 64) bytes of bits, which
 * always suffice for clipped boxes, and stay valid until the next call on this context.  Limits: mask_size <= 32,
 * num_classes <= 256, H and W in [1, 32768]. */
MNC_API int mnc_mask_records(mnc_ctx* ctx, const float* d_records, const int* d_counts, int record_cap, int num_classes,
                             int mask_size, double score_thresh, double binarize_thresh, int H, int W, void** d_info,
                             void** d_bits);
/* n6 on the device: mnc_mask_overlaps with A the result of mnc_mask_records on this context -- d_info, d_bits and rows_cap
 * (= its record_cap) as that call returned them; the instance count (head.kept) is read on the device, the host does not read it
 * back.  B is a host set as in mnc_mask_overlaps, uploaded stream-ordered into an arena of the context, or b_bits == NULL for A
 * against itself (nb is then rows_cap).  *d_inter (long long) and *d_iou (double) receive device addresses of [rows_cap][nb]
 * matrices, row-major with leading dimension nb; rows and columns past the sets' counts hold 0 / 0.0.  Asynchronous on ctx's
 * stream, in no captured graph; the matrices live in an arena of their own (never the one of mnc_mask_records: the masks stay
 * as they are) and stay valid until the next mnc_mask_overlaps_dev / mnc_mask_nms_dev on this context.  rows_cap == 0 or
 * nb == 0: nothing is launched, both addresses are NULL.  MNC_ERR_INVALID as mnc_mask_overlaps (rows_cap in the place of na). */
MNC_API int mnc_mask_overlaps_dev(mnc_ctx* ctx, const void* d_info, const void* d_bits, int rows_cap, const int* b_bounds,
                                  const long long* b_offsets, const long long* b_areas, const void* b_bits, size_t b_bytes, int nb,
                                  void** d_inter, void** d_iou);
/* mnc_mask_nms of the result of mnc_mask_records (rows_cap <= 2048), scores and classes taken from its instance table, the score
 * order computed on the device as well.  *d_keep receives the device address of [int kept | 252 bytes | int rows[rows_cap]]: the
 * kept instances in score order, ONE copy of 256 + 4 * rows_cap bytes brings the count and the list down.  Asynchronous on
 * ctx's stream, in no captured graph, buffers as mnc_mask_overlaps_dev's.  A NaN thresh is MNC_ERR_INVALID; a NaN score cannot
 * be seen from the host: it is ordered by its bit pattern (memory-safe) and the result is then unspecified. */
MNC_API int mnc_mask_nms_dev(mnc_ctx* ctx, const void* d_info, const void* d_bits, int rows_cap, double thresh, int class_aware,
                             void** d_keep);
/* n7 on the device: mnc_mask_rle of the result of mnc_mask_records on this context (d_info, d_bits, rows_cap = its record_cap,
 * H and W the image it was made for; rows_cap <= 2048); the instance count is read on the device, nothing is read back by the
 * call.  *d_rle receives the device address of
 *   [256-byte head: int kept at byte 0, long long total_runs at byte 8 | long long run_ptr[rows_cap + 1] | unsigned runs[runs_cap]]
 * (run_ptr entries past kept repeat total_runs).  Emission is guarded by slot < runs_cap, total_runs is always the true total:
 * a caller that finds total_runs > runs_cap calls again with room (runs_cap == 0: the counting passes alone).  Two copies bring
 * the result down: head + run_ptr, then the runs; the bits never leave the device.  Asynchronous on ctx's stream, in no captured
 * graph; the result lives in an arena of its own (never the one of mnc_mask_records: the masks stay as they are) and stays valid
 * until the next mnc_mask_rle_dev on this context.  rows_cap == 0: nothing is launched, the head is zero. */
MNC_API int mnc_mask_rle_dev(mnc_ctx* ctx, const void* d_info, const void* d_bits, int rows_cap, int H, int W, size_t runs_cap,
                             void** d_rle);
/* n8 on the device: mnc_mask_match with the detections the result of mnc_mask_records on this context (d_info, d_bits, rows_cap
 * = its record_cap <= 2048; classes, scores and areas from its instance table, the count read on the device); the ground truths
 * and the parameters are host arrays as in mnc_mask_match, uploaded stream-ordered.  The outputs are device addresses of tables
 * with rows_cap in the place of nd (leading dimension rows_cap; entries past the count hold -1 / 0 / 0.0): *d_rank,
 * *d_dt_match, *d_dt_ignore, *d_gt_match, *d_gt_ignore, and with want_iou = 1 *d_iou (else NULL).  Only those tables need to come
 * back; the bits never leave the device.  Asynchronous on ctx's stream, in no captured graph; everything lives in an arena of
 * its own (never the one of mnc_mask_records or of mnc_mask_overlaps_dev) and stays valid until the next mnc_mask_match_dev on
 * this context.  The ranks and the size rule need the device's table, so ng == 0 still launches the list and matching passes;
 * rows_cap == 0 and ng == 0 launches nothing.  A NaN score cannot be seen from the host: it is ordered by its bit pattern
 * (memory-safe) and the result is then unspecified.  MNC_ERR_INVALID otherwise as mnc_mask_match. */
MNC_API int mnc_mask_match_dev(mnc_ctx* ctx, const void* d_info, const void* d_bits, int rows_cap, const int* gt_bounds,
                               const long long* gt_offsets, const long long* gt_areas, const void* gt_bits, size_t gt_bytes, int ng,
                               const int* gt_classes, const unsigned char* gt_crowd, const unsigned char* gt_ignore_in,
                               const double* gt_eval_area, const double* iou_thrs, int T, const double* area_rngs, int A,
                               int max_det, int want_iou, void** d_rank, void** d_dt_match, void** d_dt_ignore, void** d_gt_match,
                               void** d_gt_ignore, void** d_iou);
/* The tail of im_detect on the device (tools/demo.py:84-100, lib/caffeWrapper/TesterWrapper.py:240-260): d_boxes
 * [R1+R2][4] = clip(rois[:, 1:5] / scale, image) of stage-1 rois followed by stage-2 rois (float32 division, clamp to
 * [0, W-1] x [0, H-1] as transform/bbox_transform.py:clip_boxes). */
MNC_API int mnc_detect_tail(mnc_ctx* ctx, const float* d_rois1, int R1, const float* d_rois2, int R2, float scale,
                            int image_height, int image_width, float* d_boxes);

/* Row count of the last mnc_proposal on this context (4-byte D2H + stream sync). */
MNC_API int mnc_proposal_count(mnc_ctx* ctx, int* num_rois_host);
/* The sorted pre-NMS candidates of the last mnc_proposal on this context (parity tests teacher-force the NMS with them):
 * boxes_host [n][4], scores_host [n], *n_host = n.  Pass null arrays to query n only. */
MNC_API int mnc_proposal_candidates(mnc_ctx* ctx, float* boxes_host, float* scores_host, int capacity, int* n_host);
/* StageBridgeLayer.forward_test (lib/pylayer/stage_bridge_layer.py:237-255): per RoI the box regressor of the arg-max
 * class of d_probs (first maximum, background included) is applied and clipped to (im_h, im_w).  d_bbox_pred / d_probs
 * may be column slices (row strides ld_bbox / ld_probs). */
MNC_API int mnc_stage_bridge(mnc_ctx* ctx, const float* d_rois, const float* d_bbox_pred, int ld_bbox, const float* d_probs,
                             int ld_probs, int R, int K, float im_h, float im_w, float* d_rois_ext);

/* ---------------------------------------------------------------------------------------------------------------
 * The whole image in ONE call (mnc_load_weights / mnc_forward_image): what tools/demo.py does per image
 * (prepare_mnc_args :54-76, net.forward :79-83, the tail of im_detect :84-100, gpu_mask_voting :147) for the graph
 * models/VGG16/mnc_5stage/test.prototxt, as a native object -- no Python, no prototxt parser: the layer sequence of that file
 * (13 conv3x3 + 4 pools, RPN head + ProposalLayer, two head stages with the shared parameters, StageBridge) is fixed in
 * csrc/pipeline.hip with the fused plan the Python engine derives from the prototxt (warp+pool, FC+activation, Concat-free
 * column slices, merged sibling heads), the widths are configuration.  The launch sequence of an image size is captured in a
 * HIP graph on first use and replayed afterwards (use_graph); everything is asynchronous on the context's stream and the
 * call returns after ONE synchronisation, with the final instance records in host memory.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct mnc_net mnc_net;
typedef struct mnc_net_config {
  int trunk_channels[5];   /* conv1_x .. conv5_x widths (64, 128, 256, 512, 512)                      test.prototxt:19-387 */
  int rpn_channels;        /* rpn_conv_3x3 width (512)                                                 :391-412 */
  int num_anchors;         /* 9; anchors[a*4 + k] = transform.anchors.generate_anchors() as float32   lib/transform/anchors.py:38-49 */
  float anchors[64];
  int feat_stride;         /* 16 */
  int pre_nms_topn, post_nms_topn;      /* 6000, 300                              lib/mnc_config.py TEST.RPN_{PRE,POST}_NMS_TOP_N */
  float rpn_nms_thresh, rpn_min_size;   /* 0.7, 16 */
  int mask_fc, mask_size;  /* fc6_maskest width 256, mask side 21 (mask_pred = mask_size^2 outputs)   :509-545 */
  int fc_dim;              /* fc6 / fc7 / fc6_mask / fc7_mask width 4096                               :584-696 */
  int num_classes;         /* 21 */
  int roi_size;            /* 14: ROIWarping 28x28 + MAX 2x2 in stage 2, 14x14 direct in stage 4      :479-505, 809-820 */
  float spatial_scale;     /* 0.0625 */
  int target_size, max_size;            /* 600, 1000: TEST.SCALES[0], TRAIN.MAX_SIZE (tools/demo.py:59) */
  double pixel_means[3];   /* cfg.PIXEL_MEANS, BGR */
  int max_per_image;       /* 100 */
  float vote_nms_thresh, vote_iou_thresh;   /* TEST.MASK_MERGE_NMS_THRESH 0.3, TEST.MASK_MERGE_IOU_THRESH 0.5 */
  int math;                /* 0 fp32, 1 bf16x3, 2 f16, 3 mixed = convolutions bf16x3 (fp32-class) + large InnerProducts fp16: the
                            * reduced-precision mode that keeps the 1e-3 bar; 4 bf16 = plain bf16, one product per term (BASELINE
                            * configs[2] as written; measured, outside the 1e-3 bar) (the engine's math modes) */
  int use_graph;           /* 1: replay a captured HIP graph per image size; 0: launch every kernel every time */
  int winograd;            /* fp32 math, the 3x3 convolutions: 4 = Winograd F(4x4,3x3) (mnc_conv3x3_wino4; default), 2 (or 1) =
                            * F(2x2,3x3) (mnc_conv3x3_wino), 0 = direct implicit GEMM */
  mnc_layer_conventions conventions;   /* ROIWarping / MaskResize / MaskPooling conventions.  The RoI kernels read them from the
                                        * CONTEXT: with conventions.inherit == 1 (mnc_net_default_config) mnc_net_create leaves the
                                        * context's alone (the SPEC on a fresh context, or what the host set with
                                        * mnc_ctx_set_layer_conventions); with inherit == 0 it applies this member to `ctx` (all
                                        * other fields zero = oracle/SPEC.md) -- for every net on that context */
} mnc_net_config;

/* The reference's values for every field (VGG-16 widths, lib/mnc_config.py defaults). */
MNC_API int mnc_net_default_config(mnc_net_config* cfg);
MNC_API int mnc_net_create(mnc_ctx* ctx, const mnc_net_config* cfg, mnc_net** out);
/* A second net over the SAME device weights as `parent` (its configuration too): own context `ctx` (same device: own stream,
 * scratch arenas, activation buffers, HIP graph), no weights of its own -- the reference shares parameters by `param { name }`
 * inside one net (test.prototxt:514-515 <-> :829-834); several images in flight on one GPU share them across nets the same
 * way (one 1.13 GB set instead of one per image in flight).  Packs `parent`'s weights first if that has not happened yet (its
 * parameters must all be set).  `parent` must outlive the nets that share with it: mnc_net_destroy(parent) fails with
 * MNC_ERR_STATE while one exists. */
MNC_API int mnc_net_create_shared(mnc_ctx* ctx, mnc_net* parent, mnc_net** out);
/* One parameter blob of one layer, in Caffe's own layout (what net.params[layer][index].data holds: Convolution
 * [Cout][Cin][3][3], InnerProduct [N][K] with K in (c,h,w) order, bias [N]).  Layers: conv1_1 .. conv5_3, rpn_conv_3x3,
 * rpn_cls_score, rpn_bbox_pred, fc6_maskest, mask_pred, fc6, fc7, fc6_mask, fc7_mask, cls_score, seg_cls_score, bbox_pred
 * (the *_ext layers share these by `param { name }`, test.prototxt:514-515 <-> :829-834).  index 0 = weights, 1 = bias. */
MNC_API int mnc_net_set_param(mnc_net* net, const char* layer, int index, const float* data_host, size_t count);
/* mnc_load_weights: every blob from a flat little-endian file written by mnc_amd.caffemodel.save_flat / tools/convert_weights.py:
 * "MNCW0001", uint32 n, then n x { uint16 name_len, name, uint8 blob index, uint8 ndim, uint32 dims[ndim], float32 data }.
 * Entries with a blob index > 1 (a third blob of a layer, e.g. BatchNorm's moving-average factor) are read over and ignored. */
MNC_API int mnc_net_load_file(mnc_net* net, const char* path);
/* The voting rule of the net's last stage: MNC_VOTE_MV (gpu_mask_voting, what every net starts with) or MNC_VOTE_IMAGE
 * (cpu_mask_voting, cfg.TEST.USE_GPU_MASK_MERGE = False; binarize_thresh = cfg.BINARIZE_THRESH, unused by MNC_VOTE_MV) -- see
 * mnc_vote_instances_ex.  A per-net setting (a net made by mnc_net_create_shared starts with MNC_VOTE_MV), not a field of
 * mnc_net_config.  A change drops the net's captured graph (the next image of a size runs direct and re-captures); an image in
 * flight is waited for first. */
MNC_API int mnc_net_set_voting(mnc_net* net, int mode, double binarize_thresh);
/* One image.  bgr_host: uint8 [H][W][3] (BGR, as cv2.imread gives the reference).  records_host: [record_cap][6 + S*S] float32
 * = (x1, y1, x2, y2, score, class id, mask) of the voted instances, rows past the count zero; counts_host [num_classes]:
 * [0] = number of instances, [c] = instances of class c.  record_cap <= (num_classes-1) * max_per_image. */
MNC_API int mnc_forward_image(mnc_net* net, const unsigned char* bgr_host, int H, int W, float* records_host, int record_cap,
                              int* counts_host);
/* The two halves of mnc_forward_image, for hosts that keep several images in flight (one mnc_net + context + stream per image
 * in flight; independent images overlap on the GPU, so the latency-bound stretches of one -- proposal top-k, NMS scan, voting --
 * run beside the next one's convolutions):
 *   mnc_forward_image_async  stages the image and enqueues everything (graph replay or direct launches); no synchronisation.
 *                            *d_records / *d_counts (may be NULL) are the device-resident block mnc_gather_instances sends.
 *   mnc_net_fetch            waits for that image and hands out its records exactly as mnc_forward_image does. */
MNC_API int mnc_forward_image_async(mnc_net* net, const unsigned char* bgr_host, int H, int W, float** d_records, int** d_counts);
MNC_API int mnc_net_fetch(mnc_net* net, float* records_host, int record_cap, int* counts_host);
/* mnc_render_records of the LAST image of the net -- its own record block, its own staged photograph -- into host memory: waits
 * for the image, renders on the net's stream behind it (never inside the captured graph, which stays as it is, as does a following
 * mnc_net_fetch), waits again and copies out what was asked for.  inst_host / cls_host [H][W] int32, inst_rgb_host / cls_rgb_host /
 * overlay_rgb_host [H][W][3] uint8, kept_host one int; each may be NULL.  H, W are those of the image given to mnc_forward_image.
 * MNC_ERR_STATE when no image has been forwarded on this net. */
MNC_API int mnc_net_render(mnc_net* net, double vis_thresh, double binarize_thresh, float alpha, int* inst_host, int* cls_host,
                           unsigned char* inst_rgb_host, unsigned char* cls_rgb_host, unsigned char* overlay_rgb_host,
                           int* kept_host);
/* mnc_mask_records of the LAST image of the net into host memory, beside mnc_net_render: waits for the image, packs on the net's
 * stream behind it (never inside the captured graph, which stays as it is, as does a following mnc_net_fetch), waits again and
 * copies out.  The image's row count is known on the host by then, so the context's arena is sized for those rows only.
 * info_host receives [mnc_mask_head | mnc_mask_info[kept]] (256 + 64 * info_cap bytes of room; info_cap below the image's rows is
 * MNC_ERR_INVALID -- (num_classes - 1) * max_per_image always suffices), bits_host the head.bits_bytes bytes of the masks,
 * *bits_bytes (may be NULL) that number.  bits_host == NULL: sizes only (mnc_mask_records without d_bits); bits_cap below the
 * bytes needed is MNC_ERR_INVALID.  MNC_ERR_STATE when no image has been forwarded on this net. */
MNC_API int mnc_net_masks(mnc_net* net, double score_thresh, double binarize_thresh, void* info_host, int info_cap,
                          void* bits_host, size_t bits_cap, size_t* bits_bytes);
/* Device address and Caffe-order shape of an intermediate blob of the LAST image, for parity tests: "conv5_3" (c8),
 * "rpn_cls_prob_reshape", "rpn_bbox_pred", "rois", "rois_ext", "mask_proposal" [2R][S][S] (both stages stacked),
 * "seg_cls_prob" [2R][num_classes], "boxes" [2R][4], "head_scores" [2R][6*num_classes] = [cls_score | seg_cls_score | bbox_pred]
 * of both stages, "data" (the prepared network input), "records" (the instance block of mnc_forward_image_async).  dims
 * receives up to 4 ints, *ndim their number. */
MNC_API int mnc_net_blob(mnc_net* net, const char* name, void** d_ptr, int* dims, int* ndim);
MNC_API int mnc_net_destroy(mnc_net* net);

/* ---------------------------------------------------------------------------------------------------------------
 * Multi-GPU (the reference is single-GPU: batch is 1 per forward, lib/pylayer/proposal_layer.py:65).  Images are
 * sharded one per rank, one process and one context per GPU, weights replicated, no data-path collective.  The only exchange
 * is the all-gather of every rank's instance records (mnc_vote_instances' d_records, [100][447] float32 by default) issued as
 * ncclAllGather ON THE CONTEXT'S STREAM, device pointer to device pointer.  librccl is loaded at run time.
 *   mnc_comm_unique_id  rank 0 creates the 128-byte ncclUniqueId; the host program carries it to the other ranks.
 *   mnc_comm_init       ncclCommInitRank for this context's device (collective: every rank calls it).
 *   mnc_gather_instances d_recv [nranks][floats_per_rank] <- every rank's d_send [floats_per_rank]; asynchronous.
 * ------------------------------------------------------------------------------------------------------------- */
MNC_API int mnc_comm_unique_id(void* id_out, int capacity_bytes);
MNC_API int mnc_comm_init(mnc_ctx* ctx, const void* id, int nranks, int rank);
MNC_API int mnc_comm_info(mnc_ctx* ctx, int* nranks, int* rank, int* rccl_version);
MNC_API int mnc_gather_instances(mnc_ctx* ctx, const float* d_send, float* d_recv, size_t floats_per_rank);
MNC_API int mnc_comm_destroy(mnc_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MNC_HIP_H_ */
