// Mask IoU between packed instance masks, and the greedy mask NMS built on it, for gfx950 -- the rule of the reference's
// mask_overlap (lib/transform/mask_transform.py:16-46) on the PackedMasks layout of inst_masks.hip (include/mnc_hip.h n5), for
// every pair of two sets at once: intersect the two bounds, count the pixels of that rectangle set in both masks, union =
// area_a + area_b - inter, iou = union < 1 ? 0.0 : (double)inter / (double)union.  Integer counts and one float64 division: no
// atomics, no float sums, nothing depends on order.
//
//   mask_overlaps_kernel    one wave per pair (four pairs per workgroup).  A wave whose rectangles do not meet stores 0 / 0.0 and
//                           leaves: that is most pairs.  Otherwise its lanes stride over the (row, word) items of the
//                           intersection in A's word grid: word k of a row of A covers columns ax1 + 64k ... + 63; the matching
//                           64 bits of B start at bit ax1 + 64k - bx1 of B's row (signed: floor division, non-negative
//                           remainder) and are funnel-shifted together from two neighbouring words of B (shift 0 apart: a 64-bit
//                           shift by 64 is undefined); words before or past B's row read as 0.  The last word of a row of either
//                           operand is masked to its width before use -- padding bits are not trusted -- and the columns outside
//                           the intersection drop out through the AND by themselves.  __popcll into one 64-bit sum per lane, a
//                           shuffle reduction, lane 0 stores inter and iou.
//   mask_order_kernel       the score order of the NMS: rank i = instances with a higher score, or the same score and a lower
//                           index (np.argsort(-scores, kind="stable")); one thread per instance, n <= 2048.
//   mask_nms_words_kernel   the suppression words nms_scan_kernel (nms.hip) reads, in its column-block-major layout: one wave per
//                           (row i, 64 columns) of the set against itself in score order, bit j = j > i && iou > thresh (strict,
//                           nms_kernel.cu:71) && (class blind || same class), through one __ballot.
//   mask_keep_kernel        positions in score order -> instance indices.
// The greedy scan is nms.hip's own (nms_scan_launch / _indirect), unchanged.
//
// Bound: L2 reads.  A pair reads the words of its intersection once from each operand (16 bytes per 64 pixels, B's words twice
// from L1 for the funnel); the work of 100 x 100 instances is spread over 10 000 waves, most of which leave at once.  Staging A's rows
// through LDS for a tile of partners would cut the reads of a large instance.  Not built: measured at 100 x 100 instances of a
// 600 x 1000 image the kernel takes 8.5 us of a 56 us call that is launches and copies (profiles/mask_overlaps_bench.txt).
//
// Compiled with -ffp-contract=off as its siblings are (the lone division has nothing to contract with).
#include <cmath>
#include <vector>

#include "mask_set.h"

namespace mnc {

constexpr int kOvThreads = 256;
constexpr int kOvWaves = kOvThreads / 64;
constexpr long long kOvMaxPairs = 1LL << 22;   // na * nb
constexpr int kOvMaxCoord = 1 << 24;           // |coordinate| limit: widths, heights and column differences fit an int
constexpr long long kOvMaxArea = 1LL << 26;    // pixels of one bound
constexpr int kOvMaxNms = 2048;                // instances of one mask NMS

// grid ceil(rows * cols / 4), block 256.  Pair p = (i, j) of the rows x cols output (row-major, leading dimension cols); rows /
// cols are the capacities the buffers were sized with, pairs past the sets' counts store 0 / 0.0.  order != nullptr: the pair is
// (order[i], order[j]) -- the set against itself in score order -- and with upper_only the pairs j <= i store 0 / 0.0 unread.
__global__ __launch_bounds__(kOvThreads) void mask_overlaps_kernel(MaskSet A, MaskSet B, const int* __restrict__ order, int upper_only,
                                                                   int rows, int cols, long long* __restrict__ inter_out,
                                                                   double* __restrict__ iou_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long p = (long long)blockIdx.x * kOvWaves + wave;
  if (p >= (long long)rows * cols) return;
  const int i = (int)(p / cols), j = (int)(p % cols);
  const int na = mask_count(A, rows), nb = mask_count(B, cols);
  long long inter = 0;
  double iou = 0.0;
  if (i < na && j < nb && !(upper_only && j <= i)) {
    const mnc_mask_info a = A.info[order ? order[i] : i], b = B.info[order ? order[j] : j];
    const int ix1 = max(a.x1, b.x1), iy1 = max(a.y1, b.y1), ix2 = min(a.x2, b.x2), iy2 = min(a.y2, b.y2);
    // (an instance without rows has x2 < x1 or y2 < y1: its intersection with anything is empty)
    if (ix1 <= ix2 && iy1 <= iy2) {
      const int wa = a.x2 - a.x1 + 1, wb = b.x2 - b.x1 + 1;
      const int sa = mask_strips(wa), sb = mask_strips(wb);
      const int k_lo = (ix1 - a.x1) >> 6, k_hi = (ix2 - a.x1) >> 6;
      const int nwords = k_hi - k_lo + 1, nrows = iy2 - iy1 + 1;
      const u64* rows_a = A.bits + a.offset / 8 + (long long)(iy1 - a.y1) * sa;
      const u64* rows_b = B.bits + b.offset / 8 + (long long)(iy1 - b.y1) * sb;
      const int items = nrows * nwords;                  // <= 2^26 / 64 words of A
      long long cnt = 0;
      for (int t = lane; t < items; t += 64) {
        const int r = t / nwords, k = k_lo + (t - r * nwords);
        const u64 wa_bits = mask_word(rows_a + (long long)r * sa, k, sa, wa);
        const int off = a.x1 + (k << 6) - b.x1;          // bit of B's row under bit 0 of this word, signed
        const u64 wb_bits = mask_word_at(rows_b + (long long)r * sb, off, sb, wb);
        cnt += __popcll(wa_bits & wb_bits);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
      inter = cnt;
      const long long uni = a.area + b.area - inter;
      iou = uni < 1 ? 0.0 : (double)inter / (double)uni;
    }
  }
  if (lane == 0) {
    if (inter_out) inter_out[p] = inter;
    if (iou_out) iou_out[p] = iou;
  }
}

// grid ceil(cap / 256), block 256.  order[rank of i] = i; *n_out = the count, clamped to cap (what the scan reads).
__global__ __launch_bounds__(kOvThreads) void mask_order_kernel(MaskSet A, int cap, int* __restrict__ order, int* __restrict__ n_out) {
  const int n = mask_count(A, cap);
  const int i = blockIdx.x * kOvThreads + threadIdx.x;
  if (i == 0) *n_out = n;
  if (i >= n) return;
  const unsigned mine = mask_score_key(A.info[i].score);
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const unsigned k = mask_score_key(A.info[j].score);
    rank += (k > mine || (k == mine && j < i)) ? 1 : 0;
  }
  order[rank] = i;
}

// grid ceil(cap * cb_cap / 4), block 256; cb_cap = ceil(cap / 64).  iou [cap][cap] in score order (pairs j > i valid).
// mask[c * cap + i] = the word of row i in column tile c: nms_scan_kernel's layout with n_stride = cap.
__global__ __launch_bounds__(kOvThreads) void mask_nms_words_kernel(MaskSet A, const int* __restrict__ order, int cap, int cb_cap,
                                                                    const double* __restrict__ iou, double thresh, int class_aware,
                                                                    u64* __restrict__ mask) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long g = (long long)blockIdx.x * kOvWaves + wave;
  if (g >= (long long)cap * cb_cap) return;
  const int n = mask_count(A, cap);
  const int i = (int)(g / cb_cap), c = (int)(g % cb_cap);
  if (i >= n || c * 64 >= n) return;                     // (the scan reads neither)
  const int col = c * 64 + lane;
  bool hit = col < n && col > i;
  if (hit) hit = iou[(long long)i * cap + col] > thresh;
  if (hit && class_aware) hit = A.info[order[i]].cls == A.info[order[col]].cls;
  const u64 word = __ballot(hit);
  if (lane == 0) mask[(long long)c * cap + i] = word;
}

// grid ceil(cap / 256), block 256.  out: [int kept | int instances | pad to 256 bytes | int rows[cap]]; out[0] was written by the
// scan, out[1] by mask_order_kernel.
__global__ __launch_bounds__(kOvThreads) void mask_keep_kernel(const int* __restrict__ order, const int* __restrict__ keep, int cap,
                                                               int* __restrict__ out) {
  const int r = blockIdx.x * kOvThreads + threadIdx.x;
  if (r < min(out[0], cap)) out[64 + r] = order[keep[r]];
}

// The instance table of a host set, checked: MNC_ERR_INVALID before anything is launched.  (Declared in mask_set.h: every host
// entry of the mask files checks its sets here.)
int HostMaskSet::check(const char* who, const char* set, const int* bounds, const long long* offsets, const void* bits_in,
                       size_t bytes, int n, const int* classes, const float* scores) {
  MNC_REQUIRE(n == 0 || (bounds && offsets), "%s: null pointer in set %s", who, set);
  info.assign((size_t)n, mnc_mask_info());
  bits = bits_in;
  used = 0;
  for (int i = 0; i < n; ++i) {
    const int* q = bounds + 4 * (size_t)i;
    for (int k = 0; k < 4; ++k)
      MNC_REQUIRE(q[k] > -kOvMaxCoord && q[k] < kOvMaxCoord, "%s: %s[%d] coordinate %d out of range", who, set, i, q[k]);
    const int w = q[2] - q[0] + 1, h = q[3] - q[1] + 1;
    MNC_REQUIRE(w < 1 || h < 1 || (long long)w * h <= kOvMaxArea, "%s: %s[%d] covers %lld pixels (limit %lld)", who, set, i,
                (long long)w * h, kOvMaxArea);
    MNC_REQUIRE(offsets[i] >= 0 && offsets[i] % 8 == 0, "%s: %s[%d] offset %lld is negative or not a multiple of 8", who, set, i,
                offsets[i]);
    const long long need = mask_bytes(w, h);
    MNC_REQUIRE(need == 0 || ((unsigned long long)offsets[i] <= bytes && bytes - (size_t)offsets[i] >= (size_t)need), "%s: the rows of %s[%d] (%lld bytes at %lld) reach past the %zu bytes given",
                who, set, i, need, offsets[i], bytes);
    if (need && (size_t)(offsets[i] + need) > used) used = (size_t)(offsets[i] + need);
    mnc_mask_info& d = info[i];
    d.x1 = q[0]; d.y1 = q[1]; d.x2 = q[2]; d.y2 = q[3];
    d.cls = classes ? classes[i] : 0;
    d.score = scores ? scores[i] : 0.f;
    d.row = i;
    d.offset = offsets[i];
    d.area = 0;
  }
  MNC_REQUIRE(used == 0 || bits, "%s: null bits in set %s", who, set);
  return MNC_OK;
}

// The same of a set whose areas are given: a null `areas` is refused with the other null pointers.
int HostMaskSet::check(const char* who, const char* set, const int* bounds, const long long* offsets, const long long* areas,
                       const void* bits_in, size_t bytes, int n, const int* classes, const float* scores) {
  MNC_REQUIRE(n == 0 || areas, "%s: null pointer in set %s", who, set);
  const int rc = check(who, set, bounds, offsets, bits_in, bytes, n, classes, scores);
  for (int i = 0; rc == MNC_OK && i < n; ++i) info[i].area = areas[i];
  return rc;
}

// (Declared in mask_set.h: mask_match.hip launches the overlap kernel too.)
void overlaps_launch(hipStream_t s, const MaskSet& A, const MaskSet& B, const int* d_order, int upper_only, int rows, int cols,
                     long long* d_inter, double* d_iou) {
  const long long pairs = (long long)rows * cols;
  if (pairs < 1) return;
  hipLaunchKernelGGL(mask_overlaps_kernel, dim3((unsigned)((pairs + kOvWaves - 1) / kOvWaves)), dim3(kOvThreads), 0, s, A, B, d_order,
                     upper_only, rows, cols, d_inter, d_iou);
}

namespace {

// Buffers of one mask NMS over a set of capacity `cap`, and its launch sequence: order, the upper triangle of the IoU matrix in
// score order, the suppression words, nms.hip's scan, the kept rows.
struct NmsWs {
  int *order, *keep, *out;
  double* iou;
  u64* words;
  void layout(WsLayout& l, int cap) {
    order = l.take<int>(cap);
    keep = l.take<int>(cap);
    out = l.take<int>(64 + (size_t)cap);
    iou = l.take<double>((size_t)cap * cap);
    words = l.take<u64>((size_t)cap * cdiv(cap, 64));
  }
};

void nms_launch(hipStream_t s, const MaskSet& A, int cap, double thresh, int class_aware, const NmsWs& w) {
  const int cb = cdiv(cap, 64);
  hipLaunchKernelGGL(mask_order_kernel, dim3(cdiv(cap, kOvThreads)), dim3(kOvThreads), 0, s, A, cap, w.order, w.out + 1);
  overlaps_launch(s, A, A, w.order, 1, cap, cap, nullptr, w.iou);
  hipLaunchKernelGGL(mask_nms_words_kernel, dim3((unsigned)(((long long)cap * cb + kOvWaves - 1) / kOvWaves)), dim3(kOvThreads), 0, s,
                     A, w.order, cap, cb, w.iou, thresh, class_aware, w.words);
  if (A.n_ptr)
    nms_scan_launch_indirect(s, w.words, w.out + 1, cap, cap, w.keep, w.out);
  else
    nms_scan_launch(s, w.words, A.n, A.n, w.keep, w.out, 1);
  hipLaunchKernelGGL(mask_keep_kernel, dim3(cdiv(cap, kOvThreads)), dim3(kOvThreads), 0, s, w.order, w.keep, cap, w.out);
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_overlaps(const int* a_bounds, const long long* a_offsets, const long long* a_areas, const void* a_bits, size_t a_bytes,
                      int na, const int* b_bounds, const long long* b_offsets, const long long* b_areas, const void* b_bits,
                      size_t b_bytes, int nb, long long* inter, double* iou, int device_id) {
  const bool self = b_bits == nullptr;
  if (self) nb = na;
  MNC_REQUIRE(na >= 0 && nb >= 0, "mnc_mask_overlaps: na=%d, nb=%d must be >= 0", na, nb);
  MNC_REQUIRE((long long)na * nb <= kOvMaxPairs, "mnc_mask_overlaps: %d x %d pairs (limit %lld)", na, nb, kOvMaxPairs);
  MNC_REQUIRE(inter || iou, "mnc_mask_overlaps: both outputs are null");
  HostMaskSet a, b;                                      // (b stays empty when the set meets itself)
  int rc = a.check("mnc_mask_overlaps", "a", a_bounds, a_offsets, a_areas, a_bits, a_bytes, na, nullptr, nullptr);
  if (rc) return rc;
  if (!self) {
    rc = b.check("mnc_mask_overlaps", "b", b_bounds, b_offsets, b_areas, b_bits, b_bytes, nb, nullptr, nullptr);
    if (rc) return rc;
  }
  if (na == 0 || nb == 0) { clear_error(); return MNC_OK; }
  const size_t pairs = (size_t)na * nb;
  long long* d_inter; double* d_iou;
  auto layout = [&](WsLayout l) {
    a.take(l);
    b.take(l);
    d_inter = l.take<long long>(inter ? pairs : 0);
    d_iou = l.take<double>(iou ? pairs : 0);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(a.upload(hs));
  MNC_HIP_TRY(b.upload(hs));
  const MaskSet A = a.view(), B = self ? A : b.view();
  overlaps_launch(hs.stream, A, B, nullptr, 0, na, nb, inter ? d_inter : nullptr, iou ? d_iou : nullptr);
  MNC_HIP_TRY(hipGetLastError());
  if (inter) MNC_HIP_TRY(hs.down(inter, d_inter, pairs * 8));
  if (iou) MNC_HIP_TRY(hs.down(iou, d_iou, pairs * 8));
  MNC_HIP_TRY(hs.sync());
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_overlaps_dev(mnc_ctx* ctx, const void* d_info, const void* d_bits, int rows_cap, const int* b_bounds,
                          const long long* b_offsets, const long long* b_areas, const void* b_bits, size_t b_bytes, int nb,
                          void** d_inter, void** d_iou) {
  MNC_REQUIRE(ctx && d_inter && d_iou, "mnc_mask_overlaps_dev: null pointer");
  const bool self = b_bits == nullptr;
  if (self) nb = rows_cap;
  MNC_REQUIRE(rows_cap >= 0 && nb >= 0, "mnc_mask_overlaps_dev: rows_cap=%d, nb=%d must be >= 0", rows_cap, nb);
  MNC_REQUIRE((long long)rows_cap * nb <= kOvMaxPairs, "mnc_mask_overlaps_dev: %d x %d pairs (limit %lld)", rows_cap, nb, kOvMaxPairs);
  HostMaskSet b;                                         // (stays empty when the set meets itself)
  int rc = MNC_OK;
  if (!self) {
    rc = b.check("mnc_mask_overlaps_dev", "b", b_bounds, b_offsets, b_areas, b_bits, b_bytes, nb, nullptr, nullptr);
    if (rc) return rc;
  }
  *d_inter = nullptr;
  *d_iou = nullptr;
  if (rows_cap == 0 || nb == 0) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(d_info && d_bits, "mnc_mask_overlaps_dev: null device pointer");
  MNC_NO_CAPTURE(ctx, "mnc_mask_overlaps_dev");
  const size_t pairs = (size_t)rows_cap * nb;
  long long* inter; double* iou;
  auto layout = [&](WsLayout l) {
    b.take(l);
    inter = l.take<long long>(pairs);
    iou = l.take<double>(pairs);
    return l.bytes();
  };
  // an arena of its own: mask_ws holds the masks this call reads.  In no captured graph.
  rc = arena_ensure(&ctx->overlap_ws, layout(WsLayout()), 0, "mask-overlap buffers", ctx->stream, ctx);
  if (rc) return rc;
  layout(WsLayout(ctx->overlap_ws.p));
  LaunchScope ls(ctx, "mask_overlaps");
  hipStream_t s = ctx->stream;
  MNC_HIP_TRY(b.upload(s));
  const MaskSet A = MaskSet::of_records(d_info, d_bits, rows_cap), B = self ? A : b.view();
  overlaps_launch(s, A, B, nullptr, 0, rows_cap, nb, inter, iou);
  rc = ls.finish("mask_overlaps");
  if (rc) return rc;
  *d_inter = inter;
  *d_iou = iou;
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_nms(const int* bounds, const long long* offsets, const long long* areas, const void* bits, size_t bytes, int n,
                 const int* classes, const float* scores, double thresh, int class_aware, int* keep_out, int* num_out,
                 int device_id) {
  MNC_REQUIRE(keep_out && num_out, "mnc_mask_nms: null output pointer");
  MNC_REQUIRE(n >= 0 && n <= kOvMaxNms, "mnc_mask_nms: n=%d not in [0, %d]", n, kOvMaxNms);
  MNC_REQUIRE(class_aware == 0 || class_aware == 1, "mnc_mask_nms: class_aware=%d is not 0 / 1", class_aware);
  MNC_REQUIRE(!std::isnan(thresh), "mnc_mask_nms: thresh is NaN");
  MNC_REQUIRE(n == 0 || (scores && (classes || !class_aware)), "mnc_mask_nms: null scores or classes");
  for (int i = 0; i < n; ++i) MNC_REQUIRE(!std::isnan(scores[i]), "mnc_mask_nms: score %d is NaN", i);
  HostMaskSet set;
  int rc = set.check("mnc_mask_nms", "masks", bounds, offsets, areas, bits, bytes, n, classes, scores);
  if (rc) return rc;
  *num_out = 0;
  if (n == 0) { clear_error(); return MNC_OK; }
  NmsWs w;
  auto layout = [&](WsLayout l) {
    set.take(l);
    w.layout(l, n);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(set.upload(hs));
  nms_launch(hs.stream, set.view(), n, thresh, class_aware, w);
  MNC_HIP_TRY(hipGetLastError());
  std::vector<int> out(64 + (size_t)n);
  MNC_HIP_TRY(hs.down(out.data(), w.out, out.size() * 4));       // the count and the kept rows in one copy
  MNC_HIP_TRY(hs.sync());
  *num_out = out[0];
  for (int r = 0; r < out[0]; ++r) keep_out[r] = out[64 + r];
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_nms_dev(mnc_ctx* ctx, const void* d_info, const void* d_bits, int rows_cap, double thresh, int class_aware,
                     void** d_keep) {
  MNC_REQUIRE(ctx && d_keep, "mnc_mask_nms_dev: null pointer");
  MNC_REQUIRE(rows_cap >= 0 && rows_cap <= kOvMaxNms, "mnc_mask_nms_dev: rows_cap=%d not in [0, %d]", rows_cap, kOvMaxNms);
  MNC_REQUIRE(class_aware == 0 || class_aware == 1, "mnc_mask_nms_dev: class_aware=%d is not 0 / 1", class_aware);
  MNC_REQUIRE(!std::isnan(thresh), "mnc_mask_nms_dev: thresh is NaN");
  MNC_REQUIRE(d_info && (d_bits || rows_cap == 0), "mnc_mask_nms_dev: null device pointer");
  MNC_NO_CAPTURE(ctx, "mnc_mask_nms_dev");
  NmsWs w;
  auto layout = [&](WsLayout l) {
    w.layout(l, rows_cap);
    return l.bytes();
  };
  int rc = arena_ensure(&ctx->overlap_ws, layout(WsLayout()), 0, "mask-overlap buffers", ctx->stream, ctx);
  if (rc) return rc;
  layout(WsLayout(ctx->overlap_ws.p));
  LaunchScope ls(ctx, "mask_nms");
  hipStream_t s = ctx->stream;
  if (rows_cap == 0) {
    MNC_HIP_TRY(hipMemsetAsync(w.out, 0, 256, s));
  } else {
    nms_launch(s, MaskSet::of_records(d_info, d_bits, rows_cap), rows_cap, thresh, class_aware, w);
  }
  rc = ls.finish("mask_nms");
  if (rc) return rc;
  *d_keep = w.out;
  clear_error();
  return MNC_OK;
}
