// One set of packed instance masks (include/mnc_hip.h n5), as the mask files share it: inst_masks.hip, mask_overlaps.hip, mask_rle.hip,
// mask_match.hip, mask_boundary.hip, mask_poly.hip, mask_components.hip, mask_contours.hip, mask_distance.hip, mask_shape.hip, mask_algebra.hip, mask_warp.hip, mask_labels.hip, mask_pixels.hip, mask_surface.hip, mask_targets.hip and, through mask_tight.h, mask_tight.hip.  Internal to libmnc_hip.so; nothing else includes it.
#pragma once
#include <vector>

#include "mnc_internal.h"

namespace mnc {

typedef unsigned long long u64;

// Words of one row of w columns, and the bytes of a w x h mask: rows of whole 64-bit words, no bytes without rows.
__host__ __device__ inline int mask_strips(int w) { return (w + 63) >> 6; }
__host__ __device__ inline long long mask_bytes(int w, int h) { return w < 1 || h < 1 ? 0 : (long long)h * mask_strips(w) * 8; }

// An instance has rows: its bounds hold a pixel position.
__host__ __device__ inline bool mask_has_rows(const mnc_mask_info& m) { return m.x2 >= m.x1 && m.y2 >= m.y1; }

// A set on the device -- the instance table, the words, and the count (read from *n_ptr when that is set).
struct MaskSet {
  const mnc_mask_info* info;
  const u64* bits;
  const int* n_ptr;
  int n;
  // The result of mnc_mask_records (inst_masks.hip): the table stands behind the 256-byte head, whose `kept` is the count.  A result
  // without rows (rows_cap == 0) may have no table at all: null info, count 0.
  static MaskSet of_records(const void* d_info, const void* d_bits, int rows_cap) {
    const mnc_mask_head* head = (const mnc_mask_head*)d_info;
    return {rows_cap ? (const mnc_mask_info*)(head + 1) : nullptr, (const u64*)d_bits, rows_cap ? &head->kept : nullptr, 0};
  }
};

// The count of a set whose buffers were sized for `cap` instances.
__device__ __forceinline__ int mask_count(const MaskSet& s, int cap) { return min(max(s.n_ptr ? *s.n_ptr : s.n, 0), cap); }

// Word j of a row of `strips` words holding w columns: 0 outside the row, the padding of the last word cleared (padding bits are
// not trusted).
__device__ __forceinline__ u64 mask_word(const u64* __restrict__ row, int j, int strips, int w) {
  if (j < 0 || j >= strips) return 0ull;
  u64 v = row[j];
  const int valid = w - (j << 6);
  if (valid < 64) v &= (1ull << valid) - 1ull;
  return v;
}

// The 64 bits of that row from bit `bit` on (signed: floor division, non-negative remainder), funnel-shifted together from two
// neighbouring words (shift 0 apart: a 64-bit shift by 64 is undefined); bits before or past the row read 0.
__device__ __forceinline__ u64 mask_word_at(const u64* __restrict__ row, int bit, int strips, int w) {
  const int q = bit >> 6, s = bit & 63;
  u64 v = mask_word(row, q, strips, w);
  if (s) v = (v >> s) | (mask_word(row, q + 1, strips, w) << (64 - s));
  return v;
}

// The 64 bits of instance m from image column x on, in image row y: 0 outside its bounds.
__device__ __forceinline__ u64 mask_read(const mnc_mask_info& m, const u64* __restrict__ bits, int x, int y) {
  const int x1 = m.x1, y1 = m.y1, w = m.x2 - x1 + 1;
  if (w < 1 || y < y1 || y > m.y2) return 0ull;
  const int strips = mask_strips(w);
  return mask_word_at(bits + m.offset / 8 + (long long)(y - y1) * strips, x - x1, strips, w);
}

// Where the words of a set are numbered in raster order, instance after instance, and insts[i].*kFirst is the first word of
// instance i: the last of the n instances whose first word is at or before g -- the one that holds word g (an instance without
// words begins where the next does).  At most 11 turns: the entries that number words this way take n <= 2048.
template <auto kFirst, class Inst>
__device__ __forceinline__ int mask_owner(const Inst* __restrict__ insts, int n, int g) {
  int lo = 0, hi = n - 1;
  for (int turn = 0; turn < 12 && lo < hi; ++turn) {
    const int mid = (lo + hi + 1) >> 1;
    if (insts[mid].*kFirst <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// float32 -> an unsigned key with the floats' order (-0.0 counts as 0.0, as it does for numpy's comparison).  A NaN, which the
// host entries refuse and a device table cannot be asked about without a read-back, gets the place of its bit pattern: the order
// is a permutation whatever the scores hold.
__device__ __forceinline__ unsigned mask_score_key(float s) {
  if (s == 0.f) s = 0.f;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// A set an entry point receives as host arrays (bounds, offsets, areas as include/mnc_hip.h n5 gives them): checked, given its place
// in the call's workspace, uploaded.
struct HostMaskSet {
  std::vector<mnc_mask_info> info;   // the checked instance table (boundary_plan and rle_extent read it)
  const void* bits = nullptr;        // the caller's words
  size_t used = 0;                   // the bytes of them the rows reach
  mnc_mask_info* d_info = nullptr;
  u64* d_bits = nullptr;
  // mask_overlaps.hip: the table, checked against the coordinate, pixel and offset limits of mnc_mask_overlaps -- MNC_ERR_INVALID
  // before anything is launched.  Without `areas`, for a set whose areas are not given, every area is stored as 0.
  int check(const char* who, const char* set, const int* bounds, const long long* offsets, const long long* areas, const void* bits,
            size_t bytes, int n, const int* classes, const float* scores);
  int check(const char* who, const char* set, const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n,
            const int* classes, const float* scores);
  void take(WsLayout& l) {
    d_info = l.take<mnc_mask_info>(info.size());
    d_bits = l.take<u64>(used / 8);
  }
  // asynchronous copies on the stream; nothing is enqueued for zero bytes
  hipError_t upload(hipStream_t s) const {
    const hipError_t e = info.empty() ? hipSuccess
                                      : hipMemcpyAsync(d_info, info.data(), info.size() * sizeof(mnc_mask_info), hipMemcpyHostToDevice, s);
    return e != hipSuccess || !used ? e : hipMemcpyAsync(d_bits, bits, used, hipMemcpyHostToDevice, s);
  }
  hipError_t upload(const HostScope& hs) const { return upload(hs.stream); }
  MaskSet view() const { return {d_info, d_bits, nullptr, (int)info.size()}; }
};

// mask_overlaps.hip: the launch of the overlap kernel over rows x cols pairs of two sets (pairs past the sets' counts store 0 / 0.0;
// d_order != nullptr: the set against itself in that order; either output may be null)
void overlaps_launch(hipStream_t s, const MaskSet& A, const MaskSet& B, const int* d_order, int upper_only, int rows, int cols,
                     long long* d_inter, double* d_iou);
// mask_boundary.hip: the boundary bands (include/mnc_hip.h n11) of one set of packed masks on the device.  boundary_plan makes, on
// the host, the instance table of the result from the input's (bounds clipped to the H x W image, not tightened; (0, 0, -1, -1)
// for an instance without rows or outside the image; offsets in order without gaps; areas 0, which the launch adds to; class,
// score and row carried over) and what the launch needs; boundary_launch writes every word of d_out_bits once and adds the bit
// counts to d_out_info[i].area.  d_out_info holds the uploaded table of boundary_plan, d_scratch plan.planes * plan.bytes bytes.
struct BdPlan {
  int n;                  // instances
  int planes;             // scratch planes of `bytes` each: the row-eroded words, and for a large d their block prefix ANDs
  size_t bytes;           // of the clipped masks = of the result's bits
  long long most_words;   // of one instance
  long long most_scan;    // (word columns x blocks of 2d + 1 rows) of one instance
};
void boundary_plan(const std::vector<mnc_mask_info>& in, int H, int W, int d, std::vector<mnc_mask_info>* out, BdPlan* plan);
void boundary_launch(hipStream_t s, const MaskSet& in, int H, int W, int d, const BdPlan& plan, mnc_mask_info* d_out_info,
                     u64* d_out_bits, u64* d_scratch);
int boundary_check_image(const char* who, int H, int W, int d);   // MNC_ERR_INVALID: H or W outside [1, 32768], d outside [1, 1024]
// mnc_mask_boundary_timing's timer (mask_boundary.hip): mnc_mask_boundary and the boundary part of mnc_mask_match_boundary keep
// the time of their launches in it
extern CallTimer g_bd_timer;

}  // namespace mnc
