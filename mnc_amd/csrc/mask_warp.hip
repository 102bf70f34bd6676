// Geometric transforms of packed instance masks (include/mnc_hip.h n18), for gfx950, on the PackedMasks layout of inst_masks.hip (n5),
// without unpacking a mask: the eight lattice isometries plus a translation (mnc_mask_isometry) and the nearest-neighbour gather
// through an integer affine inverse map (mnc_mask_warp).  The statements of the rules are mnc_amd/warp.py:isometry_numpy and
// warp_numpy; this file computes the same tables and words bit for bit.  All arithmetic is integer.
//
// The two entries are one expression with three forms.  Output instance o is the image of input instance o; it has a LOOSE FRAME
// -- a box that follows from the instance's bounds, the map and the window alone, outside of which its result cannot have a pixel.
// A wave owns a block of 64 rows x 64 columns of a frame, and wp_block leaves in lane l the 64 result bits of the block's row l:
//   rows        isometries that keep rows as rows (codes 0, 2, 4, 6): lane l reads its source row once through mask_word_at at the
//               (mirrored) signed bit position, and reverses the word with __brevll when x is negated.
//   transpose   isometries that turn rows into columns (codes 1, 3, 5, 7): lane l reads the 64 bits of the source row that becomes
//               result column l (reversed when the new y is negated), 64 __ballots of bit k give result row k as one uniform word,
//               and lane k keeps it -- the 64 x 64 bit transpose of mask_rle.hip, without LDS.  Rows and columns outside the source
//               read 0, so partially filled blocks need no case of their own.
//   gather      the affine map: for each of the block's live rows, lane l forms the two int64 numerators of pixel (x0 + l, y), takes
//               the floor of their quotients by den (a 64-bit division corrected towards minus infinity; an arithmetic shift when
//               den is a power of two, which is what affine_map makes), tests the source pixel, and a __ballot is the row's word.
//               Where a quotient does not depend on the row (c1 == 0) or on the column (c3 == 0) -- both for a resize -- it is
//               formed once per lane and, for the rows, handed round by a shuffle: two divisions per lane and block, not 128.
// The frame -- which already is intersected with the window -- is applied as a word and row mask.
//
// The result is tight and its size depends on the data: the protocol, its five launches and its driver are mask_tight.h's.  Here
// the unit of work is a wave per block -- the algebra's passes with a wave, not a lane, as the unit:
//   wp_extent_kernel   a wave per block of the loose frame: wp_block, then tight_join with each lane's row.
//   wp_fill_kernel     a wave per block of the TIGHT frame: wp_block again at the tight position, every word stored once, then
//                      tight_count.
//
// Bound: latency.  100 instances of an image are a few hundred KB of words that sit in L2; an isometry reads at most two words per
// result word; the gather reads one word per pixel and pass, a wave walking the 64 rows of its block eight at a time with their
// loads in flight together (one at a time the chain of L2 latencies was the kernels' time).  Measured at 100 instances of a
// 600 x 1000 image, call with its copies / kernels alone: fliplr 0.16 ms / 18 us, rot90 0.16 ms / 20 us, resize to half 0.17 ms /
// 35 us, to 1.5 times 0.21 ms / 43 us, warp_affine by 30 degrees 0.21 ms / 43 us (profiles/mask_warp_bench.txt).  62 and 63 VGPRs in
// the two block kernels, no LDS and no scratch in any kernel.
#include <algorithm>
#include <climits>
#include <vector>

#include "mask_tight.h"

namespace mnc {

constexpr int kWpThreads = 256;
constexpr int kWpWaves = kWpThreads / 64;
constexpr long long kWpMaxDen = 1ll << 32;
constexpr long long kWpMaxLinear = 1ll << 32;  // |c0|, |c1|, |c3|, |c4|
constexpr long long kWpMaxOffset = 1ll << 60;  // |c2|, |c5|: with the other limits every numerator stays below 2^62

enum WpForm { kWpRows = 0, kWpTranspose = 1, kWpGather = 2 };

// The map of one call.  Isometries: negx / negy say whether the source x / y falls as the result coordinate it depends on rises,
// tx, ty the translation.  Gather: sx = floor((c[0] x + c[1] y + c[2]) / den), sy alike with c[3 .. 5]; shift >= 0: den == 1 << shift.
struct WpMap {
  int form, negx, negy, tx, ty, shift;
  long long c[6], den;
};

// floor(a / d) for d > 0: C++'s quotient rounds towards zero, one too high for a negative a that d does not divide.
__device__ __forceinline__ long long wp_floor_div(long long a, long long d, int shift) {
  if (shift >= 0) return a >> shift;
  const long long q = a / d;
  return (a - q * d) < 0 ? q - 1 : q;
}

// Pixel (sx, sy) of instance m, which has rows; the coordinates as wide as the quotients come.  The load is unconditional -- a
// pixel outside the bounds reads the instance's first word and drops it -- so that the loads of several rows can be in flight.
__device__ __forceinline__ bool wp_pixel(const mnc_mask_info& m, const u64* __restrict__ bits, long long sx, long long sy) {
  const bool inside = sx >= m.x1 && sx <= m.x2 && sy >= m.y1 && sy <= m.y2;
  const int dx = inside ? (int)sx - m.x1 : 0, dy = inside ? (int)sy - m.y1 : 0;
  const u64 word = bits[m.offset / 8 + (long long)dy * mask_strips(m.x2 - m.x1 + 1) + (dx >> 6)];
  return ((word >> (dx & 63)) & (u64)inside) != 0ull;      // (& not &&: no branch for the load to sink into)
}

// The 64 result bits of job j from image column x0 >= j.fx on, in image row y0 + lane; `rows` <= 64 rows of the block are wanted
// (the other lanes' words are not used by the caller).  Every lane of the wave comes here.  Both passes call it.
__device__ __forceinline__ u64 wp_block(const TightFrame& j, const mnc_mask_info& m, const u64* __restrict__ bits, const WpMap& p,
                                        int x0, int y0, int rows, int lane) {
  u64 v = 0ull;
  if (p.form == kWpRows) {
    const int y = y0 + lane - p.ty, sy = p.negy ? -y : y;
    v = p.negx ? __brevll(mask_read(m, bits, p.tx - x0 - 63, sy)) : mask_read(m, bits, x0 - p.tx, sy);
  } else if (p.form == kWpTranspose) {
    // result column x0 + lane is source row sy; its bit k is the result pixel of row y0 + k
    const int x = x0 + lane - p.tx, sy = p.negy ? -x : x;
    const u64 col = p.negx ? __brevll(mask_read(m, bits, p.ty - y0 - 63, sy)) : mask_read(m, bits, y0 - p.ty, sy);
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const u64 b = __ballot((col >> k) & 1ull);
      if (lane == k) v = b;
    }
  } else {
    const long long x = x0 + lane;
    const long long ax = p.c[0] * x + p.c[2], ay = p.c[3] * x + p.c[5];
    // an axis-aligned map (a resize) needs no quotient per pixel: sx does not depend on the row when c1 == 0 and is formed once;
    // sy does not depend on the column when c3 == 0, so lane r forms row r's and a shuffle hands it round.  Same expressions.
    const bool sx_once = p.c[1] == 0, sy_once = p.c[3] == 0;                 // (uniform)
    const long long sx_mine = sx_once ? wp_floor_div(ax, p.den, p.shift) : 0;
    const long long sy_mine = sy_once ? wp_floor_div(p.c[5] + p.c[4] * (long long)(y0 + lane), p.den, p.shift) : 0;
    // eight rows at a time, the quotients (whose division branches) first and the reads after them in straight-line code: the
    // eight loads are in flight together, not one L2 latency after the other
    for (int r0 = 0; r0 < rows; r0 += 8) {                 // (uniform)
      long long sx[8], sy[8];
      bool on[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const long long y = y0 + r0 + k;
        sx[k] = sx_once ? sx_mine : wp_floor_div(ax + p.c[1] * y, p.den, p.shift);
        sy[k] = sy_once ? __shfl(sy_mine, (r0 + k) & 63) : wp_floor_div(ay + p.c[4] * y, p.den, p.shift);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) on[k] = wp_pixel(m, bits, sx[k], sy[k]);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const u64 b = __ballot(on[k]);
        if (lane == r0 + k) v = b;
      }
    }
  }
  const int y = y0 + lane, valid = j.fx + j.fw - x0;       // columns of the frame from x0 on
  if (y < j.fy || y >= j.fy + j.fh || valid < 1) return 0ull;
  if (valid < 64) v &= (1ull << valid) - 1ull;
  return v;
}

// grid (ceil(most loose-frame blocks / 4), jobs), block 256: a wave per 64 x 64 block of the loose frame.
__global__ __launch_bounds__(kWpThreads) void wp_extent_kernel(const TightFrame* __restrict__ jobs, MaskSet A, WpMap p,
                                                               TightBox* __restrict__ ext) {
  const int o = blockIdx.y;
  const TightFrame j = jobs[o];
  if (j.fw < 1 || j.fh < 1) return;
  const int strips = mask_strips(j.fw), lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * kWpWaves + (threadIdx.x >> 6);
  if (w >= (long long)((j.fh + 63) >> 6) * strips) return;  // (the whole wave)
  const int g = (int)(w / strips), c = (int)(w - (long long)g * strips);
  const u64 v = wp_block(j, A.info[o], A.bits, p, j.fx + c * 64, j.fy + g * 64, min(64, j.fh - g * 64), lane);
  tight_join(ext + o, v, c * 64, g * 64 + lane);
}

// grid (ceil(most loose-frame blocks / 4), jobs), block 256: a wave per 64 x 64 block of the tight frame.
__global__ __launch_bounds__(kWpThreads) void wp_fill_kernel(const TightFrame* __restrict__ jobs, MaskSet A, WpMap p,
                                                             const TightBox* __restrict__ box, Scanned first, u64* __restrict__ out,
                                                             u64* __restrict__ area) {
  const int o = blockIdx.y;
  const TightBox b = box[o];
  if (b.x2 < b.x1) return;
  const TightFrame j = jobs[o];
  const int th = b.y2 - b.y1 + 1, strips = mask_strips(b.x2 - b.x1 + 1), lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * kWpWaves + (threadIdx.x >> 6);
  if (w >= (long long)((th + 63) >> 6) * strips) return;   // (the whole wave)
  const int g = (int)(w / strips), c = (int)(w - (long long)g * strips), rows = min(64, th - g * 64);
  const u64 v = wp_block(j, A.info[o], A.bits, p, b.x1 + c * 64, b.y1 + g * 64, rows, lane);
  if (lane < rows) out[(long long)first.at(o) + (long long)(g * 64 + lane) * strips + c] = v;
  tight_count(area + o, lane < rows ? v : 0ull);
}

namespace {

typedef __int128 i128;

inline i128 wp_floor(i128 a, i128 d) {                      // d > 0
  const i128 q = a / d;
  return a - q * d < 0 ? q - 1 : q;
}

// One call (mask_tight.h): the jobs are the frames themselves; beside them the set and the map.
struct WpCall : TightCall<TightFrame> {
  HostMaskSet& A;
  WpMap map;
  explicit WpCall(HostMaskSet& a) : A(a) {}
  void take(WsLayout& l) { A.take(l); }
  hipError_t upload(const HostScope& hs) const { return A.upload(hs); }
  dim3 grid() const { return dim3((unsigned)((most_blocks + kWpWaves - 1) / kWpWaves), (unsigned)jobs.size()); }
  void extent(hipStream_t s, const TightFrame* d_jobs, TightBox* d_ext) const {
    hipLaunchKernelGGL(wp_extent_kernel, grid(), dim3(kWpThreads), 0, s, d_jobs, A.view(), map, d_ext);
  }
  void fill(hipStream_t s, const TightFrame* d_jobs, const TightBox* d_box, Scanned first, u64* d_out, u64* d_area) const {
    hipLaunchKernelGGL(wp_fill_kernel, grid(), dim3(kWpThreads), 0, s, d_jobs, A.view(), map, d_box, first, d_out, d_area);
  }
};

// What both entries refuse about a set, as mnc_mask_combine does.
int wp_check_set(const char* who, HostMaskSet* set, const int* bounds, const long long* offsets, const void* bits, size_t bytes,
                 int n) {
  MNC_REQUIRE(n >= 0 && n <= kTightMaxN, "%s: n=%d not in [0, %d]", who, n, kTightMaxN);
  return set->check(who, "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
}

CallTimer g_wp_timer;

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_isometry(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int code, int tx, int ty,
                      int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits, size_t bits_cap,
                      size_t* bits_bound, size_t* bits_bytes, int device_id) {
  const char* who = "mnc_mask_isometry";
  MNC_REQUIRE(bits_bound, "%s: null bits_bound", who);
  MNC_REQUIRE(code >= 0 && code <= 7, "%s: code=%d not in [0, 7]", who, code);
  MNC_REQUIRE(tx > -kTightMaxCoord && tx < kTightMaxCoord && ty > -kTightMaxCoord && ty < kTightMaxCoord, "%s: translation (%d, %d) out of range",
              who, tx, ty);
  HostMaskSet A;
  int rc = wp_check_set(who, &A, bounds, offsets, bits, bytes, n);
  if (rc) return rc;
  WpCall c(A);
  // a result coordinate depends on the source y (code & 1) or x; the kernels ask the other way round: which sign the source x
  // (the new y for the transposing codes, code & 4; else the new x, code & 2) and the source y take
  c.map = WpMap{(code & 1) ? kWpTranspose : kWpRows, 0, 0, tx, ty, -1, {0, 0, 0, 0, 0, 0}, 1};
  c.map.negx = (code & 1) ? (code >> 2) & 1 : (code >> 1) & 1;
  c.map.negy = (code & 1) ? (code >> 1) & 1 : (code >> 2) & 1;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = A.info[i];
    if (!mask_has_rows(a)) { c.add_empty(); continue; }
    long long u1 = (code & 1) ? a.y1 : a.x1, u2 = (code & 1) ? a.y2 : a.x2, v1 = (code & 1) ? a.x1 : a.y1, v2 = (code & 1) ? a.x2 : a.y2;
    if (code & 2) { const long long t = -u2; u2 = -u1; u1 = t; }
    if (code & 4) { const long long t = -v2; v2 = -v1; v1 = t; }
    u1 += tx; u2 += tx; v1 += ty; v2 += ty;
    MNC_REQUIRE(u1 > -kTightMaxCoord && u2 < kTightMaxCoord && v1 > -kTightMaxCoord && v2 < kTightMaxCoord,
                "%s: the image of instance %d, (%lld, %lld, %lld, %lld), leaves the coordinate range", who, i, u1, v1, u2, v2);
    c.add((int)u1, (int)v1, (int)u2, (int)v2);
  }
  return tight_run(who, c, g_wp_timer, out_bounds, out_offsets, out_areas, out_bits, bits_cap, bits_bound, bits_bytes, device_id);
}

// see include/mnc_hip.h
int mnc_mask_warp(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const long long* coef,
                  long long den, const int* window, int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits,
                  size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id) {
  const char* who = "mnc_mask_warp";
  MNC_REQUIRE(bits_bound, "%s: null bits_bound", who);
  MNC_REQUIRE(coef && window, "%s: null coef or window", who);
  MNC_REQUIRE(den >= 1 && den <= kWpMaxDen, "%s: den=%lld not in [1, 2^32]", who, den);
  for (int k = 0; k < 6; ++k) {
    const long long lim = k % 3 == 2 ? kWpMaxOffset : kWpMaxLinear;
    MNC_REQUIRE(coef[k] >= -lim && coef[k] <= lim, "%s: coef[%d]=%lld exceeds 2^%d in magnitude", who, k, coef[k], k % 3 == 2 ? 60 : 32);
  }
  int rc = tight_check_window(who, window);
  if (rc) return rc;
  i128 det = (i128)coef[0] * coef[4] - (i128)coef[1] * coef[3];
  MNC_REQUIRE(det != 0, "%s: the map is singular (c0 c4 == c1 c3)", who);
  HostMaskSet A;
  rc = wp_check_set(who, &A, bounds, offsets, bits, bytes, n);
  if (rc) return rc;
  WpCall c(A);
  c.map = WpMap{kWpGather, 0, 0, 0, 0, -1, {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]}, den};
  for (int s = 0; s <= 32; ++s)
    if (den == 1ll << s) c.map.shift = s;
  const i128 sign = det < 0 ? -1 : 1;
  det *= sign;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = A.info[i];
    if (!mask_has_rows(a)) { c.add_empty(); continue; }
    // the destination pixels whose source lies in the bounds: P[0] <= c0 x + c1 y <= P[1], Q[0] <= c3 x + c4 y <= Q[1] -- a
    // parallelogram whose corners are rationals over det
    const i128 P[2] = {(i128)a.x1 * den - coef[2], ((i128)a.x2 + 1) * den - 1 - coef[2]};
    const i128 Q[2] = {(i128)a.y1 * den - coef[5], ((i128)a.y2 + 1) * den - 1 - coef[5]};
    i128 x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    for (int k = 0; k < 4; ++k) {
      const i128 p = P[k & 1], q = Q[k >> 1];
      const i128 xn = sign * (coef[4] * p - coef[1] * q), yn = sign * (coef[0] * q - coef[3] * p);
      const i128 xl = wp_floor(xn, det), xh = -wp_floor(-xn, det), yl = wp_floor(yn, det), yh = -wp_floor(-yn, det);
      x1 = k ? std::min(x1, xl) : xl; x2 = k ? std::max(x2, xh) : xh;
      y1 = k ? std::min(y1, yl) : yl; y2 = k ? std::max(y2, yh) : yh;
    }
    x1 = std::max(x1, (i128)window[0]); y1 = std::max(y1, (i128)window[1]);
    x2 = std::min(x2, (i128)window[2]); y2 = std::min(y2, (i128)window[3]);
    if (x2 >= x1 && y2 >= y1) c.add((int)x1, (int)y1, (int)x2, (int)y2);
    else c.add_empty();
  }
  return tight_run(who, c, g_wp_timer, out_bounds, out_offsets, out_areas, out_bits, bits_cap, bits_bound, bits_bytes, device_id);
}

// see include/mnc_hip.h
int mnc_mask_warp_timing(int on, double* last_ms) { return g_wp_timer.set(on, last_ms); }
