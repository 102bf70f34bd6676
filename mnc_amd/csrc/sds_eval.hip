// The pixel counting of the SDS mAP^r evaluation for gfx950 -- utils/voc_eval.py:voc_eval_sds (reference: lib/utils/voc_eval.py:
// 195-283, lib/transform/mask_transform.py:16-46 mask_overlap).  Per prediction p, everything that does not depend on the overlap
// threshold:
//   area_p           pixels of the rounded box where the S x S mask resized to it (cv2 INTER_LINEAR, cv_resize.h) is
//                    >= float32(binarize_thresh)
//   for each GT g of p's (class, image), in list order:
//     inter_pg       pixels of the intersection rectangle where the prediction and the GT bit are both set
//     union_pg       area_g + area_p - inter_pg
//     ov             inter / union in float64 (0 when the rectangles do not meet or union < 1)
//   best_gt[p]       the first g with a strictly greater ov, starting from -1000 (-1: no GT), and its inter / union.
// Matching (the only threshold-dependent, order-dependent part) runs on the host from these.
//
// sds_best_overlap_kernel: one workgroup (256 lanes) per prediction.  The mask goes to LDS as float32; lanes walk the box (then
// each intersection rectangle) pixel by pixel, count in registers, and one wave-shuffle + LDS reduction per rectangle gives the
// count to lane 0, which keeps the arg-max.  The GTs of p are walked sequentially, so ties resolve in list order.  Bound: pixel
// work, sum over p of (box area + sum of intersection areas), ~20 VALU operations each (two taps with one float64 multiply).
//
// Compiled with -ffp-contract=off: the resize is evaluated in the reference's operation order and the quotients are correctly
// rounded float64 divisions, as Python's float(inter) / float(union).
#include <cmath>

#include "cv_resize.h"
#include "mnc_internal.h"

namespace mnc {

constexpr int kSdsThreads = 256;
constexpr int kSdsMaxMask = 32;               // S <= 32 (cfg.MASK_SIZE is 21)
constexpr double kSdsMaxCoord = 1 << 24;      // |rounded coordinate| limit: widths and heights fit an int
constexpr long long kSdsMaxArea = 1LL << 26;  // pixels of one rounded prediction box (or GT bound): counts fit an int

__device__ __forceinline__ int sds_block_sum(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kSdsThreads / 64; ++k) t += red[k];
  __syncthreads();                            // red[] may be written again
  return t;                                   // (lane 0 of the block only)
}

// boxes [P][4] float64, masks [P][S*S] bytes (taken as float32), gt_begin / gt_end [P] into the GT arrays: bounds [G][4] (x1, y1,
// x2, y2), byte offsets [G] of bit rows of ceil(w / 8) bytes (bit x of a row is bit x % 8 of byte x / 8), areas [G].
__global__ __launch_bounds__(kSdsThreads) void sds_best_overlap_kernel(
    const double* __restrict__ boxes, const unsigned char* __restrict__ masks, int S, const int* __restrict__ gt_begin,
    const int* __restrict__ gt_end, const int* __restrict__ gt_bounds, const long long* __restrict__ gt_offsets,
    const unsigned char* __restrict__ gt_bits, const long long* __restrict__ gt_areas, float mthr, int* __restrict__ best_gt,
    long long* __restrict__ best_inter, long long* __restrict__ best_union) {
  __shared__ float mk[kSdsMaxMask * kSdsMaxMask];
  __shared__ int red[kSdsThreads / 64];
  const long p = blockIdx.x;
  const unsigned char* m = masks + p * S * S;
  for (int i = threadIdx.x; i < S * S; i += kSdsThreads) mk[i] = (float)m[i];
  __syncthreads();
  // np.round(new_boxes[i, :4]).astype(int): half to even in float64 (the host checked the range)
  const double* b = boxes + p * 4;
  const int x0 = (int)rint(b[0]), y0 = (int)rint(b[1]), x1 = (int)rint(b[2]), y1 = (int)rint(b[3]);
  const int w = x1 - x0 + 1, h = y1 - y0 + 1;
  const double ifx = cv_inv(w, S), ify = cv_inv(h, S);

  int cnt = 0;
  for (int i = threadIdx.x; i < w * h; i += kSdsThreads) {
    const int dy = i / w, dx = i - dy * w;
    cnt += cv_px(mk, S, dy, dx, ifx, ify) >= mthr;
  }
  const long long area_p = sds_block_sum(cnt, red);

  double best_ov = -1000.0;
  int bg = -1;
  long long bi = 0, bu = 0;
  const int g0 = gt_begin[p], g1 = gt_end[p];
  for (int g = g0; g < g1; ++g) {
    const int gx0 = gt_bounds[4 * g], gy0 = gt_bounds[4 * g + 1], gx1 = gt_bounds[4 * g + 2], gy1 = gt_bounds[4 * g + 3];
    const int ix0 = max(gx0, x0), iy0 = max(gy0, y0), ix1 = min(gx1, x1), iy1 = min(gy1, y1);
    const bool meet = ix0 <= ix1 && iy0 <= iy1;
    int inter = 0;
    if (meet) {                               // uniform over the block
      const int iw = ix1 - ix0 + 1, ih = iy1 - iy0 + 1;
      const long rowbytes = (gx1 - gx0 + 1 + 7) >> 3;
      const unsigned char* gb = gt_bits + gt_offsets[g];
      int c = 0;
      for (int i = threadIdx.x; i < iw * ih; i += kSdsThreads) {
        const int ry = i / iw, y = iy0 + ry, x = ix0 + (i - ry * iw);
        const int gx = x - gx0;
        if ((gb[(long)(y - gy0) * rowbytes + (gx >> 3)] >> (gx & 7)) & 1)
          c += cv_px(mk, S, y - y0, x - x0, ifx, ify) >= mthr;
      }
      inter = sds_block_sum(c, red);
    }
    if (threadIdx.x == 0) {
      const long long uni = gt_areas[g] + area_p - inter;
      const double ov = meet && uni >= 1 ? (double)inter / (double)uni : 0.0;
      if (ov > best_ov) { best_ov = ov; bg = g; bi = inter; bu = uni; }
    }
  }
  if (threadIdx.x == 0) { best_gt[p] = bg; best_inter[p] = bi; best_union[p] = bu; }
}

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_sds_best_overlap(const double* boxes, const unsigned char* masks, int P, int mask_size, const int* gt_begin,
                         const int* gt_end, int G, const int* gt_bounds, const long long* gt_offsets, const unsigned char* gt_bits,
                         size_t gt_bytes, const long long* gt_areas, double binarize_thresh, int* best_gt, long long* best_inter,
                         long long* best_union, int device_id) {
  MNC_REQUIRE(P >= 0 && G >= 0, "mnc_sds_best_overlap: P=%d, G=%d must be >= 0", P, G);
  MNC_REQUIRE(mask_size >= 1 && mask_size <= kSdsMaxMask, "mnc_sds_best_overlap: mask_size %d not in [1, %d]", mask_size,
              kSdsMaxMask);
  if (P == 0) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(boxes && masks && gt_begin && gt_end && best_gt && best_inter && best_union, "mnc_sds_best_overlap: null pointer");
  MNC_REQUIRE(G == 0 || (gt_bounds && gt_offsets && gt_areas), "mnc_sds_best_overlap: null GT pointer");
  MNC_REQUIRE(gt_bytes == 0 || gt_bits, "mnc_sds_best_overlap: null gt_bits");
  for (int g = 0; g < G; ++g) {
    const int* q = gt_bounds + 4 * (size_t)g;
    MNC_REQUIRE(q[0] <= q[2] && q[1] <= q[3] && q[0] > -kSdsMaxCoord && q[2] < kSdsMaxCoord && q[1] > -kSdsMaxCoord &&
                    q[3] < kSdsMaxCoord,
                "mnc_sds_best_overlap: GT %d bound (%d, %d, %d, %d) is empty or out of range", g, q[0], q[1], q[2], q[3]);
    const long long w = (long long)q[2] - q[0] + 1, h = (long long)q[3] - q[1] + 1;
    MNC_REQUIRE(w * h <= kSdsMaxArea, "mnc_sds_best_overlap: GT %d bound %lld x %lld exceeds %lld pixels", g, w, h, kSdsMaxArea);
    MNC_REQUIRE(gt_areas[g] >= 0 && gt_areas[g] <= w * h, "mnc_sds_best_overlap: GT %d area %lld not in [0, %lld]", g,
                gt_areas[g], w * h);
    MNC_REQUIRE(gt_offsets[g] >= 0 && (unsigned long long)gt_offsets[g] + (unsigned long long)(h * ((w + 7) / 8)) <= gt_bytes,
                "mnc_sds_best_overlap: GT %d bit rows [%lld, +%lld) outside the %zu bytes", g, gt_offsets[g], h * ((w + 7) / 8),
                gt_bytes);
  }
  // every rounded box non-empty (the reference's cv2.resize raises otherwise), checked before anything is launched
  for (int p = 0; p < P; ++p) {
    const double* b = boxes + 4 * (size_t)p;
    double r[4];
    for (int k = 0; k < 4; ++k) {
      r[k] = std::rint(b[k]);
      MNC_REQUIRE(std::fabs(r[k]) < kSdsMaxCoord, "mnc_sds_best_overlap: box %d coordinate %g out of range", p, b[k]);
    }
    MNC_REQUIRE(r[0] <= r[2] && r[1] <= r[3],
                "mnc_sds_best_overlap: box %d (%g, %g, %g, %g) is empty once rounded (cv2.resize would raise)", p, b[0], b[1],
                b[2], b[3]);
    const double area = (r[2] - r[0] + 1) * (r[3] - r[1] + 1);
    MNC_REQUIRE(area <= (double)kSdsMaxArea, "mnc_sds_best_overlap: box %d covers %.0f pixels (limit %lld)", p, area,
                kSdsMaxArea);
    MNC_REQUIRE(gt_begin[p] >= 0 && gt_begin[p] <= gt_end[p] && gt_end[p] <= G,
                "mnc_sds_best_overlap: GT range [%d, %d) of box %d not inside [0, %d)", gt_begin[p], gt_end[p], p, G);
  }
  const int S = mask_size;
  const size_t nP = (size_t)P, nG = (size_t)G;
  double* d_boxes; unsigned char *d_masks, *d_bits; int *d_begin, *d_end, *d_bounds, *d_bg; long long *d_offs, *d_areas, *d_bi, *d_bu;
  auto layout = [&](WsLayout l) {
    d_boxes = l.take<double>(nP * 4);
    d_masks = l.take<unsigned char>(nP * S * S);
    d_begin = l.take<int>(nP);
    d_end = l.take<int>(nP);
    d_bounds = l.take<int>(nG * 4);
    d_offs = l.take<long long>(nG);
    d_areas = l.take<long long>(nG);
    d_bits = l.take<unsigned char>(gt_bytes);
    d_bg = l.take<int>(nP);
    d_bi = l.take<long long>(nP);
    d_bu = l.take<long long>(nP);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, 0);                   // the device's stream (and device check)
  if (rc) return rc;
  CallBuf buf;     // this call's own: a whole-dataset call needs ~0.5 KB per prediction, too much to keep in the workspace
  rc = buf.alloc("mnc_sds_best_overlap", layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(buf.p));
  MNC_HIP_TRY(hs.up(d_boxes, boxes, nP * 32));
  MNC_HIP_TRY(hs.up(d_masks, masks, nP * S * S));
  MNC_HIP_TRY(hs.up(d_begin, gt_begin, nP * 4));
  MNC_HIP_TRY(hs.up(d_end, gt_end, nP * 4));
  MNC_HIP_TRY(hs.up(d_bounds, gt_bounds, nG * 16));
  MNC_HIP_TRY(hs.up(d_offs, gt_offsets, nG * 8));
  MNC_HIP_TRY(hs.up(d_areas, gt_areas, nG * 8));
  MNC_HIP_TRY(hs.up(d_bits, gt_bits, gt_bytes));
  // a numpy float32 mask is compared with the Python float threshold in float32
  hipLaunchKernelGGL(sds_best_overlap_kernel, dim3(P), dim3(kSdsThreads), 0, hs.stream, d_boxes, d_masks, S, d_begin, d_end, d_bounds,
                     d_offs, d_bits, d_areas, (float)binarize_thresh, d_bg, d_bi, d_bu);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(best_gt, d_bg, nP * 4));
  MNC_HIP_TRY(hs.down(best_inter, d_bi, nP * 8));
  MNC_HIP_TRY(hs.down(best_union, d_bu, nP * 8));
  MNC_HIP_TRY(hs.sync());
  clear_error();
  return MNC_OK;
}
