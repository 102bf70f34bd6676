// The boundary bands of packed instance masks (include/mnc_hip.h n11), for gfx950 -- the rule of the published mask_to_boundary
// (Boundary IoU, Cheng et al., CVPR 2021: a zero border, cv2.erode with a 3 x 3 kernel of ones d times, the difference) on the
// PackedMasks layout of inst_masks.hip (n5), without unpacking a mask.  With M the mask cropped to the H x W image, E the pixels of
// M whose whole (2d + 1)^2 window lies in the image and in M, the boundary is B = M & ~E.  The statement of the rule is
// mnc_amd/boundary.py:boundary_numpy; this file computes the same words bit for bit.  The window AND is separable: along the row
// (zeros beyond the ends of the row), then down the column (zero rows beyond the box: the clipped box ends where the image does or
// where the mask's bounds do, and the mask is 0 beyond those).
//
//   bd_src_word             the one crop step, at the read of the input words: word j of a row of the clipped box is 64 bits of the
//                           input row from bit max(0, -x1) + 64 j on (mask_word_at: funnel-shifted together from two neighbouring
//                           input words, the input's padding masked before use) and the columns >= the clipped width cleared; a
//                           word outside the row reads 0.
//   boundary_rows_kernel    one thread per output word (instance = blockIdx.y, consecutive lanes = consecutive words of a row).
//                           eroded = ~dilate(~row): in the word itself a log-step shift-OR dilation by min(d, 63); from each of
//                           the ceil(d / 64) words to either side only the zero nearest to this word matters (__clzll / __ffsll):
//                           it reaches the output bits within d of it -- a mask of low resp. high bits, the whole word when the
//                           neighbour lies inside every bit's window.  Words outside the row are all zeros of the mask, and so
//                           are the columns >= w of the last word.  The row-eroded word goes to plane 0 of the scratch buffer.
//   boundary_scan_kernel    (d > kBdPlainMaxD) one thread per (word column, block of 2d + 1 rows): walks its block down, storing
//                           the running prefix AND in plane 1, then up, replacing plane 0 in place by the running suffix AND (its
//                           own block's words only: nobody else reads them in this launch).
//   boundary_final_kernel   one thread per output word: E = suffix[y - d] & prefix[y + d] (the window of 2d + 1 rows meets at most
//                           two blocks) -- two reads whatever d is; for d <= kBdPlainMaxD the 2d + 1 <= 9 row-eroded words
//                           themselves (no scan launch, no plane 1).  E = 0 where y - d or y + d leaves the box.  B = M & ~E with M
//                           read through bd_src_word again, stored once; __popcll, a wave reduction, one integer atomic add per
//                           wave on the instance's area (uploaded as 0 with the instance table).
// Every output word is written exactly once by ordinary vector stores, nothing is zeroed beforehand; the only atomics are integer
// sums: the same bits from run to run.  No floating point in this file.  The intermediate planes live in device memory (a mask may
// be 2^26 pixels), never in LDS.
//
// Bound: latency.  The data of an image's masks is a few hundred KB, read a handful of times from L2; a call is three dependent
// launches per set.  The row pass reads up to 2 ceil(d / 64) + 1 words of its row per output word (33 at d = 1024, 3 at d <= 64),
// the scan reads and writes every word twice, the final pass reads two.  The scan has one thread per word column and block --
// few threads with long walks for a tall narrow mask -- which is what a larger d costs.  Measured at 100 instances of a 600 x 1000
// image, d = 23: the three kernels take 31 us of a 0.14 ms call that is launches and copies (profiles/mask_boundary_bench.txt).
#include <vector>

#include "mask_set.h"

namespace mnc {

constexpr int kBdThreads = 256;
constexpr int kBdMaxN = 2048;                  // instances of one call (mnc_mask_rle's limit)
constexpr int kBdMaxSide = 32768;              // H, W limit
constexpr int kBdMaxD = 1024;
// Up to this d the final pass ANDs the 2d + 1 <= 9 row-eroded words of its column itself (consecutive rows of one plane, L2 hits)
// instead of paying a third launch that reads and writes both planes; above it the reads per output word would grow with d.
constexpr int kBdPlainMaxD = 4;

// The crop: word j of the clipped row (w columns in `strips` words) whose column 0 is bit sx >= 0 of the input row (of `sa` words
// holding `wa` columns).
__device__ __forceinline__ u64 bd_src_word(const u64* __restrict__ row, int j, int strips, int w, int sx, int sa, int wa) {
  if (j < 0 || j >= strips) return 0ull;
  u64 v = mask_word_at(row, sx + (j << 6), sa, wa);
  const int valid = w - (j << 6);
  if (valid < 64) v &= (1ull << valid) - 1ull;
  return v;
}

struct BdBox {
  int w, h, strips, sx, sy, sa, wa;
  long long in_words, out_words;               // first word of the instance in the input bits / in the output bits and the planes
};

__device__ __forceinline__ BdBox bd_box(const mnc_mask_info& a, const mnc_mask_info& o) {
  BdBox b;
  b.w = o.x2 - o.x1 + 1;
  b.h = o.y2 - o.y1 + 1;
  b.strips = mask_strips(b.w);
  b.sx = o.x1 - a.x1;                          // >= 0: the clipped box lies inside the input's bounds
  b.sy = o.y1 - a.y1;
  b.wa = a.x2 - a.x1 + 1;
  b.sa = mask_strips(b.wa);
  b.in_words = a.offset / 8;
  b.out_words = o.offset / 8;
  return b;
}

// grid (ceil(most_words / 256), n), block 256.  plane0[word] = the row-eroded word.
__global__ __launch_bounds__(kBdThreads) void boundary_rows_kernel(MaskSet A, const mnc_mask_info* __restrict__ out, int d,
                                                                   u64* __restrict__ plane0) {
  const int i = blockIdx.y;
  const mnc_mask_info o = out[i];
  if (o.x2 < o.x1 || o.y2 < o.y1) return;
  const BdBox b = bd_box(A.info[i], o);
  const long long t = (long long)blockIdx.x * kBdThreads + threadIdx.x;
  if (t >= (long long)b.h * b.strips) return;
  const int y = (int)(t / b.strips), k = (int)(t - (long long)y * b.strips);
  const u64* row = A.bits + b.in_words + (long long)(b.sy + y) * b.sa;
  // z: the zeros of the mask as ones; dilated by d they are the complement of the eroded row
  u64 z = ~bd_src_word(row, k, b.strips, b.w, b.sx, b.sa, b.wa);
  const int r = d < 63 ? d : 63;
  for (int done = 0, step = 1; done < r; step <<= 1) {
    const int sh = step < r - done ? step : r - done;
    z |= (z << sh) | (z >> sh);
    done += sh;
  }
  const int nb = (d + 63) >> 6;
  for (int jj = 1; jj <= nb && z != ~0ull; ++jj) {
    const u64 left = ~bd_src_word(row, k - jj, b.strips, b.w, b.sx, b.sa, b.wa);
    if (left) {
      // its highest zero stands 64 jj + c - hi columns before bit c of this word
      const int m = d - (jj << 6) + (63 - __clzll((long long)left));
      if (m >= 63) z = ~0ull;
      else if (m >= 0) z |= (2ull << m) - 1ull;
    }
    const u64 right = ~bd_src_word(row, k + jj, b.strips, b.w, b.sx, b.sa, b.wa);
    if (right) {
      // its lowest zero stands 64 jj + lo - c columns after bit c
      const int m = (jj << 6) + (__ffsll((long long)right) - 1) - d;
      if (m <= 0) z = ~0ull;
      else if (m <= 63) z |= ~0ull << m;
    }
  }
  plane0[b.out_words + t] = ~z;
}

// grid (ceil(most_scan / 256), n), block 256.  Thread (block of 2d + 1 rows, word column): plane1 = prefix ANDs of plane0 inside
// the block, then plane0 = suffix ANDs inside the block, in place.
__global__ __launch_bounds__(kBdThreads) void boundary_scan_kernel(const mnc_mask_info* __restrict__ out, int d, u64* __restrict__ plane0,
                                                                   u64* __restrict__ plane1) {
  const mnc_mask_info o = out[blockIdx.y];
  if (o.x2 < o.x1 || o.y2 < o.y1) return;
  const int w = o.x2 - o.x1 + 1, h = o.y2 - o.y1 + 1, strips = mask_strips(w);
  const int len = 2 * d + 1, blocks = (h + len - 1) / len;
  const long long t = (long long)blockIdx.x * kBdThreads + threadIdx.x;
  if (t >= (long long)blocks * strips) return;
  const int blk = (int)(t / strips), k = (int)(t - (long long)blk * strips);
  const int r0 = blk * len, r1 = (r0 + len < h ? r0 + len : h) - 1;
  u64* p0 = plane0 + o.offset / 8 + k;
  u64* p1 = plane1 + o.offset / 8 + k;
  u64 acc = ~0ull;
  for (int r = r0; r <= r1; ++r) {
    acc &= p0[(long long)r * strips];
    p1[(long long)r * strips] = acc;
  }
  acc = ~0ull;
  for (int r = r1; r >= r0; --r) {
    acc &= p0[(long long)r * strips];
    p0[(long long)r * strips] = acc;
  }
}

// grid (ceil(most_words / 256), n), block 256.  bits[word] = M & ~E; out[i].area += the bits set (uploaded as 0).
__global__ __launch_bounds__(kBdThreads) void boundary_final_kernel(MaskSet A, mnc_mask_info* out, int d,
                                                                    const u64* __restrict__ plane0, const u64* __restrict__ plane1,
                                                                    u64* __restrict__ bits) {
  const int i = blockIdx.y;
  const mnc_mask_info o = out[i];
  if (o.x2 < o.x1 || o.y2 < o.y1) return;                // (the whole workgroup: blockIdx.y is the instance)
  const BdBox b = bd_box(A.info[i], o);
  const long long t = (long long)blockIdx.x * kBdThreads + threadIdx.x;
  long long cnt = 0;
  if (t < (long long)b.h * b.strips) {
    const int y = (int)(t / b.strips), k = (int)(t - (long long)y * b.strips);
    u64 e = 0ull;
    if (y >= d && y + d < b.h) {
      const u64* col = plane0 + b.out_words + k;
      if (plane1) {
        e = col[(long long)(y - d) * b.strips] & plane1[b.out_words + k + (long long)(y + d) * b.strips];
      } else {
        e = ~0ull;
        for (int r = y - d; r <= y + d; ++r) e &= col[(long long)r * b.strips];
      }
    }
    const u64 m = bd_src_word(A.bits + b.in_words + (long long)(b.sy + y) * b.sa, k, b.strips, b.w, b.sx, b.sa, b.wa);
    const u64 v = m & ~e;
    bits[b.out_words + t] = v;
    cnt = __popcll(v);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd((u64*)&out[i].area, (u64)cnt);
}

// (Declared in mask_set.h: mask_match.hip plans and launches the two boundary sets of its call.)
void boundary_plan(const std::vector<mnc_mask_info>& in, int H, int W, int d, std::vector<mnc_mask_info>* out, BdPlan* plan) {
  const size_t n = in.size();
  out->assign(n, mnc_mask_info());
  plan->n = (int)n;
  plan->bytes = 0;
  plan->most_words = plan->most_scan = 0;
  plan->planes = d > kBdPlainMaxD ? 2 : 1;
  const long long len = 2LL * d + 1;
  for (size_t i = 0; i < n; ++i) {
    const mnc_mask_info& a = in[i];
    mnc_mask_info& o = (*out)[i];
    o.x1 = 0; o.y1 = 0; o.x2 = -1; o.y2 = -1;
    o.cls = a.cls; o.score = a.score; o.row = a.row;
    o.offset = (long long)plan->bytes;
    o.area = 0;
    if (a.x2 < a.x1 || a.y2 < a.y1) continue;            // no rows
    const int x1 = a.x1 > 0 ? a.x1 : 0, y1 = a.y1 > 0 ? a.y1 : 0;
    const int x2 = a.x2 < W - 1 ? a.x2 : W - 1, y2 = a.y2 < H - 1 ? a.y2 : H - 1;
    if (x2 < x1 || y2 < y1) continue;                    // wholly outside the image
    o.x1 = x1; o.y1 = y1; o.x2 = x2; o.y2 = y2;
    const long long h = y2 - y1 + 1, strips = (x2 - x1 + 64) >> 6;
    const long long words = h * strips, scan = (h + len - 1) / len * strips;
    plan->bytes += (size_t)words * 8;
    if (words > plan->most_words) plan->most_words = words;
    if (scan > plan->most_scan) plan->most_scan = scan;
  }
}

void boundary_launch(hipStream_t s, const MaskSet& in, int H, int W, int d, const BdPlan& plan, mnc_mask_info* d_out_info, u64* d_out_bits,
                     u64* d_scratch) {
  (void)H; (void)W;                                      // (the clipped bounds in d_out_info carry them)
  if (plan.n < 1 || plan.most_words < 1) return;
  u64* plane0 = d_scratch;
  u64* plane1 = plan.planes > 1 ? d_scratch + plan.bytes / 8 : nullptr;
  const dim3 grid((unsigned)((plan.most_words + kBdThreads - 1) / kBdThreads), (unsigned)plan.n);
  hipLaunchKernelGGL(boundary_rows_kernel, grid, dim3(kBdThreads), 0, s, in, d_out_info, d, plane0);
  if (plane1)
    hipLaunchKernelGGL(boundary_scan_kernel, dim3((unsigned)((plan.most_scan + kBdThreads - 1) / kBdThreads), (unsigned)plan.n),
                       dim3(kBdThreads), 0, s, d_out_info, d, plane0, plane1);
  hipLaunchKernelGGL(boundary_final_kernel, grid, dim3(kBdThreads), 0, s, in, d_out_info, d, plane0, plane1, d_out_bits);
}

int boundary_check_image(const char* who, int H, int W, int d) {
  MNC_REQUIRE(H >= 1 && W >= 1 && H <= kBdMaxSide && W <= kBdMaxSide, "%s: image %d x %d not in [1, %d]", who, H, W, kBdMaxSide);
  MNC_REQUIRE(d >= 1 && d <= kBdMaxD, "%s: d=%d not in [1, %d]", who, d, kBdMaxD);
  return MNC_OK;
}

// mnc_mask_boundary_timing: a HIP event pair around the launches of the next calls, the last call's time kept
CallTimer g_bd_timer;

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_boundary(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int H, int W, int d,
                      int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits, size_t bits_cap,
                      size_t* bits_bytes, int device_id) {
  const char* who = "mnc_mask_boundary";
  MNC_REQUIRE(n >= 0 && n <= kBdMaxN, "%s: n=%d not in [0, %d]", who, n, kBdMaxN);
  int rc = boundary_check_image(who, H, W, d);
  if (rc) return rc;
  MNC_REQUIRE(bits_bytes, "%s: null bits_bytes", who);
  MNC_REQUIRE(n == 0 || (out_bounds && out_offsets), "%s: null output pointer", who);
  MNC_REQUIRE(n == 0 || !out_bits || out_areas, "%s: null out_areas", who);
  HostMaskSet set;
  std::vector<mnc_mask_info> out;
  rc = set.check(who, "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
  if (rc) return rc;
  *bits_bytes = 0;
  if (n == 0) { clear_error(); return MNC_OK; }
  BdPlan plan;
  boundary_plan(set.info, H, W, d, &out, &plan);
  for (int i = 0; i < n; ++i) {
    out_bounds[4 * (size_t)i] = out[i].x1; out_bounds[4 * (size_t)i + 1] = out[i].y1;
    out_bounds[4 * (size_t)i + 2] = out[i].x2; out_bounds[4 * (size_t)i + 3] = out[i].y2;
    out_offsets[i] = out[i].offset;
  }
  *bits_bytes = plan.bytes;
  if (!out_bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(bits_cap >= plan.bytes, "%s: bits_cap %zu is below the %zu bytes of the boundaries", who, bits_cap, plan.bytes);
  for (int i = 0; i < n; ++i) out_areas[i] = 0;
  if (plan.bytes == 0) { clear_error(); return MNC_OK; } // no instance meets the image
  mnc_mask_info* d_out; u64 *d_obits, *d_scratch;
  auto layout = [&](WsLayout l) {
    set.take(l);
    d_out = l.take<mnc_mask_info>(n);
    d_obits = l.take<u64>(plan.bytes / 8);
    d_scratch = l.take<u64>(plan.bytes / 8 * plan.planes);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(set.upload(hs));
  MNC_HIP_TRY(hs.up(d_out, out.data(), (size_t)n * sizeof(mnc_mask_info)));
  TimedSpan span(g_bd_timer);
  span.begin(hs.stream);
  boundary_launch(hs.stream, set.view(), H, W, d, plan, d_out, d_obits, d_scratch);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(out.data(), d_out, (size_t)n * sizeof(mnc_mask_info)));
  MNC_HIP_TRY(hs.down(out_bits, d_obits, plan.bytes));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  for (int i = 0; i < n; ++i) out_areas[i] = out[i].area;
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_boundary_timing(int on, double* last_ms) { return g_bd_timer.set(on, last_ms); }
