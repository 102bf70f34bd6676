// Per-instance binary masks at image resolution for gfx950, packed one bit per pixel -- the rule every consumer of a voted
// instance applies first (reference: lib/utils/vis_seg.py:101-130 _convert_pred_to_image, lib/utils/voc_eval.py:197-199): round
// the box half to even, clip it to the image (clip = 1, the visualisation's rule) or not (clip = 0, the evaluation's), resize the
// S x S mask to the box with cv2's INTER_LINEAR rule (cv_resize.h) and binarise with >= float32(binarize_thresh).  mnc_render_*
// paints these masks over one another and mnc_sds_best_overlap counts them; here each instance keeps its own.
//
// Output of instance i: h rows of ceil(w / 64) little-endian 64-bit words at byte offset[i]; bit dx % 64 of word dx / 64 of a row
// is pixel dx, padding bits are 0 -- utils.voc_eval.pack_sds_gt's bit order with the row stride rounded up to 8 bytes, so that one
// wave's __ballot is one stored word.  area[i] = its set bits.
//
//   inst_masks_select_kernel  one workgroup: the records with score >= score_thresh in record order (render_select_kernel's rows),
//                             their rounded clipped bounds, byte sizes and work items, and the exclusive prefix of both (ballot
//                             count for the order, shuffle scan for the sums).  No host read-back.  The host-array entry computes
//                             the same table on the host: there it follows from the boxes alone.
//   inst_masks_pack_kernel    a workgroup takes work items (one instance, 32 * fold rows) grid-stride; the instance of an item is
//                             found by bisection of the items' prefix.  The S x S mask goes to LDS; a wave owns a 64-column strip
//                             and walks 8 row steps down it: every lane evaluates its pixel (its column tap does not change down
//                             the strip), the comparison goes through __ballot and lanes [0, fold) store one 8-byte word each.  A
//                             box of w <= 32 columns folds fold = 64 / pow2(w) rows into one wave step, so a 7-wide box still uses 56
//                             of the 64 lanes.  __popcll of the ballots is summed per wave and item and added to the area with one
//                             64-bit integer atomic (exact in any order).
// Write bound: every word of the output is stored once (8 bytes per 64 pixels), the mask is read once per item from L2; ~30 VALU
// operations per pixel (two taps with one float64 multiply each).
//
// Compiled with -ffp-contract=off: the resize is evaluated in the reference's operation order.
#include <cmath>
#include <vector>

#include "cv_resize.h"
#include "mask_set.h"
#include "scan.h"

namespace mnc {

constexpr int kMaskThreads = 256;
constexpr int kMaskWaves = kMaskThreads / 64;
constexpr int kMaskSteps = 8;                  // row steps a wave walks down one strip
constexpr int kMaskChunk = 32;                 // row steps of one work item (x fold rows each)
constexpr int kMaskMaxMask = 32;               // S <= 32 (cfg.MASK_SIZE is 21)
constexpr double kMaskMaxCoord = 1 << 24;      // |rounded coordinate| limit: widths and heights fit an int
constexpr long long kMaskMaxArea = 1LL << 26;  // pixels of one box
constexpr int kMaskMaxSide = 32768;            // H, W limit with clip = 1
constexpr int kMaskMaxGrid = 2048;             // workgroups of the pack launch: 8 per CU, items beyond are taken grid-stride

static_assert(sizeof(mnc_mask_info) == 64 && sizeof(mnc_mask_head) == 256, "the layout include/mnc_hip.h documents");

// Lanes one row of a w-column box takes in a wave step: 64 above 32 columns (one strip per step), else the power of two >= w.
__host__ __device__ inline int mask_wpad(int w) {
  if (w > 32) return 64;
  int p = 1;
  while (p < w) p <<= 1;
  return p;
}
__host__ __device__ inline long long mask_items(int w, int h) {
  if (w < 1 || h < 1) return 0;
  const int rows = kMaskChunk * (64 / mask_wpad(w));
  return ((long long)h + rows - 1) / rows;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// block 256.  d_records [record_cap][6 + S*S], rows [0, min(d_counts[0], record_cap)); info [record_cap]; head: kept rows, total
// bytes and work items.  A rounded, clipped box with x2 < x1 or y2 < y1 keeps its place and has no bytes and no items.
__global__ __launch_bounds__(kMaskThreads) void inst_masks_select_kernel(const float* __restrict__ records,
                                                                         const int* __restrict__ counts, int record_cap, int S,
                                                                         double score_thresh, int H, int W,
                                                                         mnc_mask_head* __restrict__ head,
                                                                         mnc_mask_info* __restrict__ info) {
  __shared__ int wave_cnt[kMaskWaves];
  __shared__ long long wave_bytes[kMaskWaves], wave_items[kMaskWaves];
  const int D = 6 + S * S;
  const int n = min(max(counts[0], 0), record_cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  long long base_bytes = 0, base_items = 0;
  for (int r0 = 0; r0 < n; r0 += kMaskThreads) {
    const int r = r0 + threadIdx.x;
    const float* rec = records + (long)(r < n ? r : 0) * D;
    // det[:, -1] >= thresh on the reference's float64 boxes: the float32 score widened (render_select_kernel's rows)
    const bool keep = r < n && (double)rec[4] >= score_thresh;
    mnc_mask_info d = {};
    long long bytes = 0, items = 0;
    if (keep) {
      // np.round(box).astype(int), half to even (the record holds integral float32 coordinates), then the clip
      d.x1 = clampi((int)rintf(rec[0]), 0, W - 1); d.y1 = clampi((int)rintf(rec[1]), 0, H - 1);
      d.x2 = clampi((int)rintf(rec[2]), 0, W - 1); d.y2 = clampi((int)rintf(rec[3]), 0, H - 1);
      d.score = rec[4];
      d.cls = (int)rec[5];
      d.row = r;
      bytes = mask_bytes(d.x2 - d.x1 + 1, d.y2 - d.y1 + 1);
      items = mask_items(d.x2 - d.x1 + 1, d.y2 - d.y1 + 1);
    }
    const unsigned long long b = __ballot(keep);
    const long long incl_bytes = wave_incl_scan(bytes, lane), incl_items = wave_incl_scan(items, lane);
    if (lane == 63) { wave_bytes[wave] = incl_bytes; wave_items[wave] = incl_items; }
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int off = base, total = 0;
    long long off_bytes = base_bytes, off_items = base_items, total_bytes = 0, total_items = 0;
    for (int k = 0; k < kMaskWaves; ++k) {
      if (k < wave) { off += wave_cnt[k]; off_bytes += wave_bytes[k]; off_items += wave_items[k]; }
      total += wave_cnt[k]; total_bytes += wave_bytes[k]; total_items += wave_items[k];
    }
    if (keep) {
      d.offset = off_bytes + incl_bytes - bytes;
      d.work = off_items + incl_items - items;
      info[off + __popcll(b & ((1ull << lane) - 1ull))] = d;
    }
    base += total; base_bytes += total_bytes; base_items += total_items;
    __syncthreads();                      // the wave_* arrays are written again
  }
  if (threadIdx.x == 0) {
    mnc_mask_head h = {};
    h.kept = base; h.bits_bytes = base_bytes; h.items = base_items;
    *head = h;
  }
}

// grid <= kMaskMaxGrid, block 256.  info [head->kept] with the prefixes filled in, area zero; mask of an instance: masks +
// info.row * mask_stride, S * S float32; bits: the words of all instances.  Every word of every instance is stored exactly once.
__global__ __launch_bounds__(kMaskThreads) void inst_masks_pack_kernel(const mnc_mask_head* __restrict__ head,
                                                                       mnc_mask_info* __restrict__ info,
                                                                       const float* __restrict__ masks, long mask_stride, int S,
                                                                       float mthr, unsigned long long* __restrict__ bits) {
  __shared__ float mk[kMaskMaxMask * kMaskMaxMask];
  const int n = head->kept;
  const long long items = head->items;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    // the last instance whose first item is <= it (instances without items share their successor's value and come before it)
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (info[mid].work <= it) lo = mid; else hi = mid - 1;
    }
    const int x1 = info[lo].x1, y1 = info[lo].y1, x2 = info[lo].x2, y2 = info[lo].y2, row = info[lo].row;
    const long long first = info[lo].work, offset = info[lo].offset;
    const int w = x2 - x1 + 1, h = y2 - y1 + 1;
    __syncthreads();                      // the previous item's mask has been read
    for (int i = threadIdx.x; i < S * S; i += kMaskThreads) mk[i] = masks[(long)row * mask_stride + i];
    __syncthreads();
    const int wpad = mask_wpad(w), fold = 64 / wpad, strips = mask_strips(w);
    const int row_lo = (int)(it - first) * (kMaskChunk * fold), row_hi = min(h, row_lo + kMaskChunk * fold);
    const double ifx = cv_inv(w, S), ify = cv_inv(h, S);
    unsigned long long* out = bits + offset / 8;
    const int sub = lane / wpad, cx = lane & (wpad - 1);           // this lane's row within a wave step, column within the strip
    const unsigned long long row_mask = wpad == 64 ? ~0ull : (1ull << wpad) - 1ull;
    int cnt = 0;
    // units of the item: (strip, group of kMaskSteps row steps), dealt to the waves
    for (int u = wave; u < strips * (kMaskChunk / kMaskSteps); u += kMaskWaves) {
      const int strip = u % strips, dx = strip * 64 + cx;
      const int r0 = row_lo + (u / strips) * (kMaskSteps * fold);
      for (int k = 0; k < kMaskSteps; ++k) {
        const int rbase = r0 + k * fold;
        if (rbase >= row_hi) break;                                 // uniform over the wave
        const int dy = rbase + sub;
        // (the taps clamp to the mask, so a lane past the box reads inside LDS; its bit is cleared here: padding bits are 0)
        const bool on = dx < w && dy < row_hi && cv_px(mk, S, dy, dx, ifx, ify) >= mthr;
        const unsigned long long b = __ballot(on);
        cnt += __popcll(b);
        if (lane < fold && rbase + lane < row_hi) out[(long long)(rbase + lane) * strips + strip] = (b >> (lane * wpad)) & row_mask;
      }
    }
    if (lane == 0 && cnt) atomicAdd((unsigned long long*)&info[lo].area, (unsigned long long)cnt);
  }
}

namespace {

void pack_launch(hipStream_t s, long long items_bound, const mnc_mask_head* d_head, mnc_mask_info* d_info, const float* d_masks,
                 long mask_stride, int S, double binarize_thresh, unsigned long long* d_bits) {
  const int grid = (int)(items_bound < kMaskMaxGrid ? items_bound : kMaskMaxGrid);
  // a numpy float32 mask is compared with the Python float threshold in float32
  hipLaunchKernelGGL(inst_masks_pack_kernel, dim3(grid), dim3(kMaskThreads), 0, s, d_head, d_info, d_masks, mask_stride, S,
                     (float)binarize_thresh, d_bits);
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_instance_masks(const double* boxes, const float* masks, int n, int mask_size, double binarize_thresh, int image_height,
                       int image_width, int clip, int* bounds, long long* offsets, long long* areas, void* bits, size_t bits_cap,
                       size_t* bits_bytes, int device_id) {
  const int H = image_height, W = image_width, S = mask_size;
  MNC_REQUIRE(n >= 0, "mnc_instance_masks: n=%d must be >= 0", n);
  MNC_REQUIRE(S >= 1 && S <= kMaskMaxMask, "mnc_instance_masks: mask_size %d not in [1, %d]", S, kMaskMaxMask);
  MNC_REQUIRE(clip == 0 || clip == 1, "mnc_instance_masks: clip=%d is not 0 / 1", clip);
  MNC_REQUIRE(!clip || (H >= 1 && W >= 1 && H <= kMaskMaxSide && W <= kMaskMaxSide),
              "mnc_instance_masks: image %d x %d not in [1, %d]", H, W, kMaskMaxSide);
  MNC_REQUIRE(bits_bytes, "mnc_instance_masks: null bits_bytes");
  if (n == 0) { *bits_bytes = 0; clear_error(); return MNC_OK; }
  MNC_REQUIRE(boxes && bounds && offsets, "mnc_instance_masks: null pointer");
  std::vector<mnc_mask_info> info((size_t)n);
  mnc_mask_head head = {};
  head.kept = n;
  for (int i = 0; i < n; ++i) {
    const double* b = boxes + 4 * (size_t)i;
    int q[4];
    for (int k = 0; k < 4; ++k) {
      const double r = std::rint(b[k]);                // np.round: half to even
      MNC_REQUIRE(std::fabs(r) < kMaskMaxCoord, "mnc_instance_masks: box %d coordinate %g out of range", i, b[k]);
      const int hi = (k & 1) ? H - 1 : W - 1;
      const int v = (int)r;
      q[k] = !clip ? v : v < 0 ? 0 : v > hi ? hi : v;
    }
    MNC_REQUIRE(q[0] <= q[2] && q[1] <= q[3],
                "mnc_instance_masks: box %d (%g, %g, %g, %g) is empty once rounded%s (cv2.resize would raise)", i, b[0], b[1], b[2],
                b[3], clip ? " and clipped" : "");
    const int w = q[2] - q[0] + 1, h = q[3] - q[1] + 1;
    MNC_REQUIRE((long long)w * h <= kMaskMaxArea, "mnc_instance_masks: box %d covers %lld pixels (limit %lld)", i, (long long)w * h,
                kMaskMaxArea);
    mnc_mask_info& d = info[i];
    d = mnc_mask_info();
    d.x1 = q[0]; d.y1 = q[1]; d.x2 = q[2]; d.y2 = q[3];
    d.row = i;
    d.offset = head.bits_bytes;
    d.work = head.items;
    head.bits_bytes += mask_bytes(w, h);
    head.items += mask_items(w, h);
  }
  for (int i = 0; i < n; ++i) {
    bounds[4 * (size_t)i] = info[i].x1; bounds[4 * (size_t)i + 1] = info[i].y1;
    bounds[4 * (size_t)i + 2] = info[i].x2; bounds[4 * (size_t)i + 3] = info[i].y2;
    offsets[i] = info[i].offset;
  }
  const size_t total = (size_t)head.bits_bytes;
  *bits_bytes = total;
  if (!bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(masks && areas, "mnc_instance_masks: null pointer");
  MNC_REQUIRE(bits_cap >= total, "mnc_instance_masks: bits_cap %zu is below the %zu bytes of the masks", bits_cap, total);
  mnc_mask_head* d_head; mnc_mask_info* d_info; float* d_masks; unsigned long long* d_bits;
  auto layout = [&](WsLayout l) {
    d_head = l.take<mnc_mask_head>(1);
    d_info = l.take<mnc_mask_info>(n);
    d_masks = l.take<float>((size_t)n * S * S);
    d_bits = l.take<unsigned long long>(total / 8);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(hs.up(d_head, &head, sizeof(head)));
  MNC_HIP_TRY(hs.up(d_info, info.data(), (size_t)n * sizeof(mnc_mask_info)));
  MNC_HIP_TRY(hs.up(d_masks, masks, (size_t)n * S * S * 4));
  pack_launch(hs.stream, head.items, d_head, d_info, d_masks, (long)S * S, S, binarize_thresh, d_bits);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(info.data(), d_info, (size_t)n * sizeof(mnc_mask_info)));
  MNC_HIP_TRY(hs.down(bits, d_bits, total));
  MNC_HIP_TRY(hs.sync());
  for (int i = 0; i < n; ++i) areas[i] = info[i].area;
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_records(mnc_ctx* ctx, const float* d_records, const int* d_counts, int record_cap, int num_classes, int mask_size,
                     double score_thresh, double binarize_thresh, int H, int W, void** d_info, void** d_bits) {
  MNC_REQUIRE(ctx && d_records && d_counts && d_info, "mnc_mask_records: null pointer");
  MNC_REQUIRE(record_cap >= 0 && num_classes >= 1 && num_classes <= 256, "mnc_mask_records: record_cap=%d, num_classes=%d",
              record_cap, num_classes);
  MNC_REQUIRE(mask_size >= 1 && mask_size <= kMaskMaxMask, "mnc_mask_records: mask_size %d not in [1, %d]", mask_size,
              kMaskMaxMask);
  MNC_REQUIRE(H >= 1 && W >= 1 && H <= kMaskMaxSide && W <= kMaskMaxSide, "mnc_mask_records: image %d x %d not in [1, %d]", H, W,
              kMaskMaxSide);
  // clipped boxes: no instance has more than H rows of ceil(W / 64) words
  const size_t words = d_bits ? (size_t)record_cap * H * mask_strips(W) : 0;
  mnc_mask_head* head; mnc_mask_info* info; unsigned long long* bits;
  auto layout = [&](WsLayout l) {
    head = l.take<mnc_mask_head>(1);
    info = l.take<mnc_mask_info>(record_cap);       // (directly behind the 256-byte head: one copy brings both down)
    bits = l.take<unsigned long long>(words);
    return l.bytes();
  };
  // in no captured graph, so growing it does not touch mnc_ctx::arena_gen
  int rc = arena_ensure(&ctx->mask_ws, layout(WsLayout()), 0, "instance-mask buffers", ctx->stream, ctx);
  if (rc) return rc;
  layout(WsLayout(ctx->mask_ws.p));
  const int S = mask_size;
  LaunchScope ls(ctx, "inst_masks");
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(inst_masks_select_kernel, dim3(1), dim3(kMaskThreads), 0, s, d_records, d_counts, record_cap, S, score_thresh,
                     H, W, head, info);
  if (d_bits && record_cap > 0)
    pack_launch(s, (long long)record_cap * ((H + kMaskChunk - 1) / kMaskChunk), head, info, d_records + 6, 6 + (long)S * S, S,
                binarize_thresh, bits);
  rc = ls.finish("inst_masks");
  if (rc) return rc;
  *d_info = head;
  if (d_bits) *d_bits = bits;
  clear_error();
  return MNC_OK;
}
