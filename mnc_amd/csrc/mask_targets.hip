// Training targets on packed ground-truth masks for gfx950 (include/mnc_hip.h n23): the two per-RoI loops of the reference's
// training step, on the PackedMasks layout of inst_masks.hip (n5).
//
//   mask_targets_kernel        the reference's intersect_mask (lib/transform/mask_transform.py:49-80) for K (box, ground truth)
//                              rows: the S x S mask regression target of a box e is cv2.resize(C, (S, S)) >= float32(thresh), C the
//                              float32 canvas of e's size that holds the ground-truth mask on e & g and zeros elsewhere.  The canvas
//                              is never made: one lane per output cell evaluates the four taps of cv_tap (cv_resize.h), each a bit
//                              look-up in the instance's words, and combines them in cv_px's order.  A box that does not meet the
//                              instance's bounds, or an instance without rows, gives zeros.  One byte stored per lane, no atomics.
//   mask_pred_overlaps_kernel  what MaskLayer.forward_train counts (lib/pylayer/mask_layer.py:68-83): a predicted S x S mask resized
//                              to its rounded, unclipped box and binarised -- inst_masks_pack_kernel's pixels, in its work items
//                              (one box, 32 * fold rows) and its lane layout -- but no word is stored: the ballot of a wave step is
//                              counted (the area) and so is the ballot of the lanes whose pixel is also set in the ground-truth
//                              instance of the row, read as the 64 bits of that instance from the strip's first column on (mask_read:
//                              funnel-shifted from two words, 0 outside its bounds, one address per row of the step).  The waves'
//                              counts meet in LDS; one 64-bit integer atomic per workgroup, item and figure.  A row with ground truth
//                              -1 has no items.
// Integer counts only: two calls give the same bytes.  No scratch memory, no float atomics.
//
// Compiled with -ffp-contract=off: the resize is evaluated in the reference's operation order.
#include <cmath>
#include <vector>

#include "cv_resize.h"
#include "mask_set.h"

namespace mnc {

constexpr int kTgThreads = 256;
constexpr int kTgWaves = kTgThreads / 64;
constexpr int kTgSteps = 8;                   // row steps a wave walks down one strip
constexpr int kTgChunk = 32;                  // row steps of one work item (x fold rows each)
constexpr int kTgMaxMask = 32;                // S <= 32 (cfg.MASK_SIZE is 21)
constexpr int kTgMaxRows = 65536;             // K
constexpr int kTgMaxCoord = 1 << 24;          // |coordinate| limit: widths, heights and column differences fit an int
constexpr long long kTgMaxArea = 1LL << 26;   // pixels of one box
constexpr int kTgMaxGrid = 2048;              // workgroups of the overlap launch: 8 per CU, items beyond are taken grid-stride

CallTimer g_tg_timer;                         // mnc_mask_targets_timing's

// One row of mnc_mask_pred_overlaps: the rounded box, its ground-truth instance (-1: none) and its first work item.
struct PredRow {
  int x1, y1, x2, y2;
  int gt;
  int pad;
  long long work;
};

// Lanes one row of a w-column box takes in a wave step, and the items of a box: inst_masks.hip's mask_wpad / mask_items.
__host__ __device__ inline int tg_wpad(int w) {
  if (w > 32) return 64;
  int p = 1;
  while (p < w) p <<= 1;
  return p;
}
__host__ __device__ inline long long tg_items(int w, int h) {
  const int rows = kTgChunk * (64 / tg_wpad(w));
  return ((long long)h + rows - 1) / rows;
}

// Pixel (x, y), image coordinates, of the canvas of a box: the instance's bit inside (ix1, iy1, ix2, iy2) = box & bounds, else 0.
__device__ __forceinline__ float canvas_px(const u64* __restrict__ rows, int strips, int gx1, int gy1, int ix1, int iy1, int ix2,
                                           int iy2, int x, int y) {
  if (x < ix1 || x > ix2 || y < iy1 || y > iy2) return 0.0f;
  const int c = x - gx1;
  return (float)((rows[(long long)(y - gy1) * strips + (c >> 6)] >> (c & 63)) & 1ull);
}

// grid ceil(K * S * S / 256), block 256.  boxes [K][4] int (x1, y1, x2, y2 inclusive), gt_index [K] in [0, count of G), out
// [K][S][S] bytes: every byte is stored once.
__global__ __launch_bounds__(kTgThreads) void mask_targets_kernel(MaskSet G, const int* __restrict__ boxes,
                                                                  const int* __restrict__ gt_index, int K, int S, float thr,
                                                                  unsigned char* __restrict__ out) {
  const long long cell = (long long)blockIdx.x * kTgThreads + threadIdx.x;
  if (cell >= (long long)K * S * S) return;
  const int k = (int)(cell / (S * S)), r = (int)(cell - (long long)k * S * S);
  const int dy = r / S, dx = r - dy * S;
  const int ex1 = boxes[4 * k], ey1 = boxes[4 * k + 1], ex2 = boxes[4 * k + 2], ey2 = boxes[4 * k + 3];
  const mnc_mask_info g = G.info[gt_index[k]];
  const int ix1 = max(ex1, g.x1), iy1 = max(ey1, g.y1), ix2 = min(ex2, g.x2), iy2 = min(ey2, g.y2);
  unsigned char v = 0;
  // (an instance without rows has x2 < x1 or y2 < y1: its intersection with anything is empty)
  if (ix1 <= ix2 && iy1 <= iy2) {
    const int ew = ex2 - ex1 + 1, eh = ey2 - ey1 + 1, strips = mask_strips(g.x2 - g.x1 + 1);
    const u64* rows = G.bits + g.offset / 8;
    const CvTap tx = cv_tap(dx, cv_inv(S, ew), ew), ty = cv_tap(dy, cv_inv(S, eh), eh);
    const int xa = ex1 + tx.i0, xb = ex1 + tx.i1, ya = ey1 + ty.i0, yb = ey1 + ty.i1;
    // cv_px's expressions: the horizontal pass of both rows, then the vertical, in float32
    const float bx = 1.0f - tx.a, by = 1.0f - ty.a;
    const float h0 = canvas_px(rows, strips, g.x1, g.y1, ix1, iy1, ix2, iy2, xa, ya) * bx +
                     canvas_px(rows, strips, g.x1, g.y1, ix1, iy1, ix2, iy2, xb, ya) * tx.a;
    const float h1 = canvas_px(rows, strips, g.x1, g.y1, ix1, iy1, ix2, iy2, xa, yb) * bx +
                     canvas_px(rows, strips, g.x1, g.y1, ix1, iy1, ix2, iy2, xb, yb) * tx.a;
    v = (h0 * by + h1 * ty.a) >= thr ? 1 : 0;
  }
  out[cell] = v;
}

// grid <= kTgMaxGrid, block 256.  rows [K] with the items' prefix filled in (rows without ground truth have none), preds
// [K][S * S] float32, counts [K][2] = (inter, area of the prediction), zero before the launch.
__global__ __launch_bounds__(kTgThreads) void mask_pred_overlaps_kernel(MaskSet G, const PredRow* __restrict__ rows, int K,
                                                                        long long items, const float* __restrict__ preds, int S,
                                                                        float mthr, unsigned long long* __restrict__ counts) {
  __shared__ float mk[kTgMaxMask * kTgMaxMask];
  __shared__ int wave_area[kTgWaves], wave_inter[kTgWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    // the last row whose first item is <= it (rows without items share their successor's value and come before it)
    int lo = 0, hi = K - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (rows[mid].work <= it) lo = mid; else hi = mid - 1;
    }
    const PredRow r = rows[lo];
    const mnc_mask_info g = G.info[r.gt];
    const int w = r.x2 - r.x1 + 1, h = r.y2 - r.y1 + 1;
    __syncthreads();                      // the previous item's mask and counts have been read
    for (int i = threadIdx.x; i < S * S; i += kTgThreads) mk[i] = preds[(long long)lo * S * S + i];
    __syncthreads();
    const int wpad = tg_wpad(w), fold = 64 / wpad, strips = mask_strips(w);
    const int row_lo = (int)(it - r.work) * (kTgChunk * fold), row_hi = min(h, row_lo + kTgChunk * fold);
    const double ifx = cv_inv(w, S), ify = cv_inv(h, S);
    const int sub = lane / wpad, cx = lane & (wpad - 1);           // this lane's row within a wave step, column within the strip
    int area = 0, inter = 0;
    // units of the item: (strip, group of kTgSteps row steps), dealt to the waves
    for (int u = wave; u < strips * (kTgChunk / kTgSteps); u += kTgWaves) {
      const int strip = u % strips, dx = strip * 64 + cx;
      const int r0 = row_lo + (u / strips) * (kTgSteps * fold);
      for (int k = 0; k < kTgSteps; ++k) {
        const int rbase = r0 + k * fold;
        if (rbase >= row_hi) break;                                 // uniform over the wave
        const int dy = rbase + sub;
        // (the taps clamp to the mask, so a lane past the box reads inside LDS; its bit is cleared here)
        const bool on = dx < w && dy < row_hi && cv_px(mk, S, dy, dx, ifx, ify) >= mthr;
        // the instance's 64 bits from the strip's first column on, in this lane's image row: 0 outside its bounds
        const u64 gw = mask_read(g, G.bits, r.x1 + strip * 64, r.y1 + dy);
        area += __popcll(__ballot(on));
        inter += __popcll(__ballot(on && ((gw >> cx) & 1ull)));
      }
    }
    if (lane == 0) { wave_area[wave] = area; wave_inter[wave] = inter; }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long a = 0, b = 0;
      for (int k = 0; k < kTgWaves; ++k) { a += (unsigned long long)wave_area[k]; b += (unsigned long long)wave_inter[k]; }
      if (b) atomicAdd(&counts[2 * (long long)lo], b);
      if (a) atomicAdd(&counts[2 * (long long)lo + 1], a);
    }
  }
}

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_targets(const int* gt_bounds, const long long* gt_offsets, const long long* gt_areas, const void* gt_bits,
                     size_t gt_bytes, int G, const int* ex_boxes, const int* gt_index, int K, int mask_size, double thresh,
                     unsigned char* out, int device_id) {
  const int S = mask_size;
  MNC_REQUIRE(K >= 0 && K <= kTgMaxRows, "mnc_mask_targets: K=%d not in [0, %d]", K, kTgMaxRows);
  MNC_REQUIRE(G >= 0, "mnc_mask_targets: G=%d must be >= 0", G);
  MNC_REQUIRE(S >= 1 && S <= kTgMaxMask, "mnc_mask_targets: mask_size %d not in [1, %d]", S, kTgMaxMask);
  MNC_REQUIRE(!std::isnan(thresh), "mnc_mask_targets: thresh is NaN");
  HostMaskSet gt;
  int rc = gt.check("mnc_mask_targets", "gt", gt_bounds, gt_offsets, gt_areas, gt_bits, gt_bytes, G, nullptr, nullptr);
  if (rc) return rc;
  MNC_REQUIRE(K == 0 || (ex_boxes && gt_index && out), "mnc_mask_targets: null pointer");
  for (int k = 0; k < K; ++k) {
    const int* q = ex_boxes + 4 * (size_t)k;
    for (int c = 0; c < 4; ++c)
      MNC_REQUIRE(q[c] > -kTgMaxCoord && q[c] < kTgMaxCoord, "mnc_mask_targets: box %d coordinate %d out of range", k, q[c]);
    MNC_REQUIRE(q[0] <= q[2] && q[1] <= q[3], "mnc_mask_targets: box %d (%d, %d, %d, %d) is empty (cv2.resize would raise)", k, q[0],
                q[1], q[2], q[3]);
    const long long px = (long long)(q[2] - q[0] + 1) * (q[3] - q[1] + 1);
    MNC_REQUIRE(px <= kTgMaxArea, "mnc_mask_targets: box %d covers %lld pixels (limit %lld)", k, px, kTgMaxArea);
    MNC_REQUIRE(gt_index[k] >= 0 && gt_index[k] < G, "mnc_mask_targets: gt_index[%d] = %d not in [0, %d)", k, gt_index[k], G);
  }
  if (K == 0) { clear_error(); return MNC_OK; }
  const size_t cells = (size_t)K * S * S;
  int *d_boxes, *d_index; unsigned char* d_out;
  auto layout = [&](WsLayout l) {
    gt.take(l);
    d_boxes = l.take<int>(4 * (size_t)K);
    d_index = l.take<int>(K);
    d_out = l.take<unsigned char>(cells);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(gt.upload(hs));
  MNC_HIP_TRY(hs.up(d_boxes, ex_boxes, 16 * (size_t)K));
  MNC_HIP_TRY(hs.up(d_index, gt_index, 4 * (size_t)K));
  TimedSpan span(g_tg_timer);
  span.begin(hs.stream);
  // a numpy float32 canvas is compared with the threshold in float32
  hipLaunchKernelGGL(mask_targets_kernel, dim3((unsigned)((cells + kTgThreads - 1) / kTgThreads)), dim3(kTgThreads), 0, hs.stream,
                     gt.view(), d_boxes, d_index, K, S, (float)thresh, d_out);
  MNC_HIP_TRY(hipGetLastError());
  span.end(hs.stream);
  MNC_HIP_TRY(hs.down(out, d_out, cells));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_pred_overlaps(const int* gt_bounds, const long long* gt_offsets, const long long* gt_areas, const void* gt_bits,
                           size_t gt_bytes, int G, const double* boxes, const float* preds, const int* gt_index, int K,
                           int mask_size, double thresh, long long* inter, long long* area_pred, int device_id) {
  const int S = mask_size;
  MNC_REQUIRE(K >= 0 && K <= kTgMaxRows, "mnc_mask_pred_overlaps: K=%d not in [0, %d]", K, kTgMaxRows);
  MNC_REQUIRE(G >= 0, "mnc_mask_pred_overlaps: G=%d must be >= 0", G);
  MNC_REQUIRE(S >= 1 && S <= kTgMaxMask, "mnc_mask_pred_overlaps: mask_size %d not in [1, %d]", S, kTgMaxMask);
  HostMaskSet gt;
  int rc = gt.check("mnc_mask_pred_overlaps", "gt", gt_bounds, gt_offsets, gt_areas, gt_bits, gt_bytes, G, nullptr, nullptr);
  if (rc) return rc;
  MNC_REQUIRE(K == 0 || (boxes && preds && gt_index && inter && area_pred), "mnc_mask_pred_overlaps: null pointer");
  std::vector<PredRow> rows((size_t)K);
  long long items = 0;
  for (int k = 0; k < K; ++k) {
    const double* b = boxes + 4 * (size_t)k;
    int q[4];
    for (int c = 0; c < 4; ++c) {
      const double r = std::rint(b[c]);                // np.round: half to even
      MNC_REQUIRE(std::fabs(r) < (double)kTgMaxCoord, "mnc_mask_pred_overlaps: box %d coordinate %g out of range", k, b[c]);
      q[c] = (int)r;
    }
    MNC_REQUIRE(q[0] <= q[2] && q[1] <= q[3],
                "mnc_mask_pred_overlaps: box %d (%g, %g, %g, %g) is empty once rounded (cv2.resize would raise)", k, b[0], b[1], b[2],
                b[3]);
    const int w = q[2] - q[0] + 1, h = q[3] - q[1] + 1;
    MNC_REQUIRE((long long)w * h <= kTgMaxArea, "mnc_mask_pred_overlaps: box %d covers %lld pixels (limit %lld)", k, (long long)w * h,
                kTgMaxArea);
    MNC_REQUIRE(gt_index[k] >= -1 && gt_index[k] < G, "mnc_mask_pred_overlaps: gt_index[%d] = %d not in [-1, %d)", k, gt_index[k], G);
    PredRow& r = rows[k];
    r.x1 = q[0]; r.y1 = q[1]; r.x2 = q[2]; r.y2 = q[3];
    r.gt = gt_index[k];
    r.pad = 0;
    r.work = items;
    if (r.gt >= 0) items += tg_items(w, h);
  }
  for (int k = 0; k < K; ++k) { inter[k] = 0; area_pred[k] = 0; }
  if (K == 0 || items == 0) { clear_error(); return MNC_OK; }
  std::vector<unsigned long long> counts(2 * (size_t)K);
  PredRow* d_rows; float* d_preds; unsigned long long* d_counts;
  auto layout = [&](WsLayout l) {
    gt.take(l);
    d_rows = l.take<PredRow>(K);
    d_preds = l.take<float>((size_t)K * S * S);
    d_counts = l.take<unsigned long long>(2 * (size_t)K);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(gt.upload(hs));
  MNC_HIP_TRY(hs.up(d_rows, rows.data(), (size_t)K * sizeof(PredRow)));
  MNC_HIP_TRY(hs.up(d_preds, preds, (size_t)K * S * S * 4));
  TimedSpan span(g_tg_timer);
  span.begin(hs.stream);
  MNC_HIP_TRY(hipMemsetAsync(d_counts, 0, 16 * (size_t)K, hs.stream));
  // a numpy float32 mask is compared with the Python float threshold in float32
  hipLaunchKernelGGL(mask_pred_overlaps_kernel, dim3((unsigned)(items < kTgMaxGrid ? items : kTgMaxGrid)), dim3(kTgThreads), 0,
                     hs.stream, gt.view(), d_rows, K, items, d_preds, S, (float)thresh, d_counts);
  MNC_HIP_TRY(hipGetLastError());
  span.end(hs.stream);
  MNC_HIP_TRY(hs.down(counts.data(), d_counts, 16 * (size_t)K));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  for (int k = 0; k < K; ++k) { inter[k] = (long long)counts[2 * (size_t)k]; area_pred[k] = (long long)counts[2 * (size_t)k + 1]; }
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_targets_timing(int on, double* last_ms) { return g_tg_timer.set(on, last_ms); }
