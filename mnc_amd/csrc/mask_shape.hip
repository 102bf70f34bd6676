// Region descriptors of packed instance masks (include/mnc_hip.h n16), for gfx950, on the PackedMasks layout of inst_masks.hip
// (n5), without unpacking a mask: the moments of order up to two, the convex hull of the pixel squares, and from the hull the
// rectangle of least area and the diameter.  The statements of the rules are mnc_amd/shape.py:moments_numpy, hull_numpy and
// oriented_numpy; this file computes the same integers.  There is no floating point.
//
//   ms_moments_kernel   one lane per 64-bit word of a row.  With c = popc(v), the sums of b and b^2 over the set bit positions b
//                       come from the popcounts of v ANDed with the six bit-plane masks of b and their pairwise ANDs (b = sum of
//                       2^k [bit k of b], b^2 = sum of 4^k [k] + 2 sum over k < l of 2^(k + l) [k][l]): 6 + 15 popcounts and no
//                       loop over bits.  Shifted by the word's column 64 j and multiplied by the row they are the word's six
//                       sums, which a shuffle reduction per wave, LDS per workgroup and one 64-bit integer atomic add per
//                       workgroup and sum bring to the instance.
//   ms_rows_kernel      one lane per lattice row Y = 0 .. h of an instance: the first and last set column of the pixel rows Y - 1
//                       and Y (count-trailing / -leading-zero walks over the row's words) give the two candidates of the row, the
//                       least first column (left chain) and the greatest last column + 1 (right chain); kMsNone where both
//                       rows are empty.  The chains are sorted by Y by construction.
//   ms_flags_kernel     one lane per candidate i.  It is a strict hull vertex exactly when the extreme tangent from it to the
//                       candidates above and the extreme tangent to those below make a strictly convex angle (the first and the
//                       last candidate of a chain always are): one pass over the chain, each lane by itself -- no pointer
//                       chasing, no order dependence.  Coordinates differ by at most 2^15: a cross product is below 2^32.
//                       The chains live in the workspace, whatever their height.
//   scan_launch         numbers the kept candidates (scan.h): per instance the right chain downwards, then the left chain.
//   ms_ptr_kernel       vert_ptr from the scan.
//   ms_place_kernel     one lane per candidate: a kept one writes its vertex -- the top of the left chain first, the right chain
//                       downwards, the rest of the left chain upwards -- in image coordinates.
//   ms_area_kernel      one workgroup per instance: twice the shoelace area.
//   ms_calipers_kernel  one workgroup per instance over its m vertices: a lane takes the edges k = lane, lane + 256, ... and for
//                       each loops over the vertices for tmin, tmax, smax of n16 and for the farthest later vertex; then a wave
//                       and workgroup reduction of (A, D, k) by cross-multiplication in unsigned __int128 (A < 2^64, D < 2^32)
//                       and of (d2, i, j).  A convex lattice polygon in a 32768 box has a few thousand vertices at most: O(m^2).
// 1 launch for the moments, 5 for the sizes of the hulls, 7 for the hulls, 7 for the oriented boxes, whatever the data.  Every
// slot is written once by vector stores; the only atomics are the 64-bit integer adds of the moments: the same bytes on every
// run.
//
// Bound: launch and copy latency.  Measured at 100 instances of a 600 x 1000 image (573 x 10^3 set pixels, 1272 hull vertices),
// kernels alone: the moments 7.8 us of a 0.070 ms call, the hulls 78 us of 0.31 ms (two calls: sizes, then vertices), the oriented
// boxes 82 us of 0.16 ms (profiles/mask_shape_bench.txt).  At most 44 VGPRs, 192 bytes of LDS and no scratch in any kernel.
#include <climits>
#include <vector>

#include "mask_set.h"
#include "scan.h"

namespace mnc {

typedef unsigned __int128 ms_u128;

constexpr int kMsThreads = 256;
constexpr int kMsWaves = kMsThreads / 64;
constexpr int kMsMaxN = 2048;                  // instances of one call (mnc_mask_boundary's limit)
constexpr int kMsMaxExtent = 32768;            // columns or rows of one bound
constexpr int kMsNone = INT_MIN;               // no candidate on this lattice row

// One instance.  One without rows has w = h = 0 and takes no candidates.
struct MsInst {
  long long src_words;        // first word of the rows
  int w, h;
  int x1, y1;
  int cand0;                  // first of its 2 (h + 1) entries in the candidate and flag arrays: the right chain, then the left
  int pad_;
};

__device__ __forceinline__ int ms_cands(const MsInst& a) { return a.h > 0 ? 2 * (a.h + 1) : 0; }

__device__ __forceinline__ u64 ms_wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid (ceil(most words / 256), n), block 256: a lane per word.  out [n][6], zero before the launch.
__global__ __launch_bounds__(kMsThreads) void ms_moments_kernel(const MsInst* __restrict__ insts, const u64* __restrict__ bits,
                                                                u64* __restrict__ out) {
  __shared__ u64 s_part[kMsWaves][6];
  const MsInst a = insts[blockIdx.y];
  const int strips = mask_strips(a.w);
  const long long words = (long long)a.h * strips;
  if ((long long)blockIdx.x * kMsThreads >= words) return;            // (the whole workgroup)
  const long long word = (long long)blockIdx.x * kMsThreads + threadIdx.x;
  u64 s[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  if (word < words) {
    const int y = (int)(word / strips), j = (int)(word - (long long)y * strips);
    const u64 v = mask_word(bits + a.src_words + (long long)y * strips, j, strips, a.w);
    if (v) {
      const u64 plane[6] = {0xaaaaaaaaaaaaaaaaull, 0xccccccccccccccccull, 0xf0f0f0f0f0f0f0f0ull,
                            0xff00ff00ff00ff00ull, 0xffff0000ffff0000ull, 0xffffffff00000000ull};
      const u64 c = (u64)__popcll(v);
      u64 sb = 0ull, sbb = 0ull;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const u64 vk = v & plane[k];
        const u64 ck = (u64)__popcll(vk);
        sb += ck << k;
        sbb += ck << (2 * k);
#pragma unroll
        for (int l = k + 1; l < 6; ++l) sbb += (u64)__popcll(vk & plane[l]) << (k + l + 1);
      }
      const u64 x0 = (u64)j * 64ull, yy = (u64)y;
      const u64 sx = x0 * c + sb;
      s[0] = c;
      s[1] = sx;
      s[2] = yy * c;
      s[3] = x0 * x0 * c + 2ull * x0 * sb + sbb;
      s[4] = yy * sx;
      s[5] = yy * yy * c;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = ms_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s_part[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    u64 t = 0ull;
    for (int wv = 0; wv < kMsWaves; ++wv) t += s_part[wv][threadIdx.x];
    if (t) atomicAdd(&out[(size_t)blockIdx.y * 6 + threadIdx.x], t);
  }
}

// The first and last set column of one row; first = INT_MAX and last = -1 for a row without a set pixel (or outside the rows).
__device__ __forceinline__ void ms_row_extent(const u64* __restrict__ bits, const MsInst& a, int strips, int y, int* first, int* last) {
  *first = INT_MAX;
  *last = -1;
  if (y < 0 || y >= a.h) return;
  const u64* row = bits + a.src_words + (long long)y * strips;
  for (int j = 0; j < strips; ++j) {
    const u64 v = mask_word(row, j, strips, a.w);
    if (v) {
      *first = j * 64 + __ffsll((long long)v) - 1;
      break;
    }
  }
  if (*first == INT_MAX) return;
  for (int j = strips - 1; j >= 0; --j) {
    const u64 v = mask_word(row, j, strips, a.w);
    if (v) {
      *last = j * 64 + 63 - __clzll((long long)v);
      break;
    }
  }
}

// grid (ceil(most (h + 1) / 256), n), block 256: a lane per lattice row.
__global__ __launch_bounds__(kMsThreads) void ms_rows_kernel(const MsInst* __restrict__ insts, const u64* __restrict__ bits,
                                                             int* __restrict__ cand) {
  const MsInst a = insts[blockIdx.y];
  const int Y = blockIdx.x * kMsThreads + threadIdx.x;
  if (a.h < 1 || Y > a.h) return;
  const int strips = mask_strips(a.w);
  int f0, l0, f1, l1;
  ms_row_extent(bits, a, strips, Y - 1, &f0, &l0);
  ms_row_extent(bits, a, strips, Y, &f1, &l1);
  const int first = min(f0, f1), last = max(l0, l1);
  cand[a.cand0 + Y] = last < 0 ? kMsNone : last + 1;
  cand[a.cand0 + (a.h + 1) + Y] = last < 0 ? kMsNone : first;
}

// (a - o) x (b - o) of the chain points (x, row); differences are at most 2^15
__device__ __forceinline__ long long ms_cross(int ox, int oy, int ax, int ay, int bx, int by) {
  return (long long)(ax - ox) * (by - oy) - (long long)(ay - oy) * (bx - ox);
}

// grid (ceil(most 2 (h + 1) / 256), n), block 256: a lane per candidate.
__global__ __launch_bounds__(kMsThreads) void ms_flags_kernel(const MsInst* __restrict__ insts, const int* __restrict__ cand,
                                                              unsigned char* __restrict__ flags) {
  const MsInst a = insts[blockIdx.y];
  const int idx = blockIdx.x * kMsThreads + threadIdx.x;
  if (idx >= ms_cands(a)) return;
  const int rows = a.h + 1, left = idx >= rows, Y = idx - left * rows;
  const int* __restrict__ P = cand + a.cand0 + left * rows;
  const int xi = P[Y];
  unsigned char keep = 0;
  if (xi != kMsNone) {
    const long long sign = left ? -1 : 1;
    int jy = -1, jx = 0, ky = -1, kx = 0;                // the tangent points above and below so far
    for (int t = 0; t < rows; ++t) {
      const int xt = P[t];
      if (xt == kMsNone || t == Y) continue;
      if (t < Y) {
        if (jy < 0 || sign * ms_cross(xi, Y, jx, jy, xt, t) > 0) { jy = t; jx = xt; }
      } else {
        if (ky < 0 || sign * ms_cross(xi, Y, kx, ky, xt, t) < 0) { ky = t; kx = xt; }
      }
    }
    keep = jy < 0 || ky < 0 || sign * ms_cross(jx, jy, xi, Y, kx, ky) > 0;
  }
  flags[a.cand0 + idx] = keep;
}

// grid ceil((n + 1) / 256), block 256.  vert_ptr [n + 1].
__global__ __launch_bounds__(kMsThreads) void ms_ptr_kernel(const MsInst* __restrict__ insts, int n, Scanned kept,
                                                            long long* __restrict__ vert_ptr) {
  const int i = blockIdx.x * kMsThreads + threadIdx.x;
  if (i > n) return;
  vert_ptr[i] = (long long)kept.upto(i < n ? insts[i].cand0 : kept.count);
}

// grid (ceil(most 2 (h + 1) / 256), n), block 256: a lane per candidate.
__global__ __launch_bounds__(kMsThreads) void ms_place_kernel(const MsInst* __restrict__ insts, const int* __restrict__ cand,
                                                              const unsigned char* __restrict__ flags, Scanned kept,
                                                              int2* __restrict__ xy) {
  const MsInst a = insts[blockIdx.y];
  const int idx = blockIdx.x * kMsThreads + threadIdx.x;
  if (idx >= ms_cands(a) || !flags[a.cand0 + idx]) return;
  const int rows = a.h + 1, left = idx >= rows, Y = idx - left * rows;
  const int r0 = kept.upto(a.cand0), r1 = kept.upto(a.cand0 + rows), r2 = kept.upto(a.cand0 + 2 * rows);
  const int nr = r1 - r0, nl = r2 - r1;
  const int rank = kept.at(a.cand0 + idx) - (left ? r1 : r0);
  const int pos = !left ? 1 + rank : rank == 0 ? 0 : 1 + nr + (nl - 1 - rank);
  xy[r0 + pos] = make_int2(a.x1 + cand[a.cand0 + idx], a.y1 + Y);
}

// grid n, block 256.  area2 [n].
__global__ __launch_bounds__(kMsThreads) void ms_area_kernel(const MsInst* __restrict__ insts, const long long* __restrict__ vert_ptr,
                                                             const int2* __restrict__ xy, long long* __restrict__ area2) {
  __shared__ u64 s_part[kMsWaves];
  const int i = blockIdx.x;
  const MsInst a = insts[i];
  const int m = (int)(vert_ptr[i + 1] - vert_ptr[i]);
  const int2* __restrict__ V = xy + vert_ptr[i];
  long long sum = 0;
  for (int k = threadIdx.x; k < m; k += kMsThreads) {
    const int2 p = V[k], q = V[k + 1 < m ? k + 1 : 0];
    sum += (long long)(p.x - a.x1) * (q.y - a.y1) - (long long)(q.x - a.x1) * (p.y - a.y1);
  }
  const u64 w = ms_wave_sum((u64)sum);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0ull;
    for (int wv = 0; wv < kMsWaves; ++wv) t += s_part[wv];
    area2[i] = (long long)t;
  }
}

// Candidates of the least rectangle are (A, D, k): A / D is the area, k the edge; k = INT_MAX: none.  Is b before a -- the smaller
// fraction, the lower k on ties?
__device__ __forceinline__ bool ms_rect_before(u64 bA, u64 bD, int bk, u64 aA, u64 aD, int ak) {
  if (bk == INT_MAX) return false;
  if (ak == INT_MAX) return true;
  const ms_u128 l = (ms_u128)aA * bD, r = (ms_u128)bA * aD;
  return r < l || (r == l && bk < ak);
}
// Candidates of the diameter are (d2, ij): the greater d2, the lower ij = (i << 32) | j on ties; d2 = 0: none.
__device__ __forceinline__ bool ms_far_before(u64 bd2, u64 bij, u64 ad2, u64 aij) { return bd2 > ad2 || (bd2 == ad2 && bij < aij); }

// grid n, block 256.  box [n][8], diameter [n][3].
__global__ __launch_bounds__(kMsThreads) void ms_calipers_kernel(const long long* __restrict__ vert_ptr, const int2* __restrict__ xy,
                                                                 long long* __restrict__ box, long long* __restrict__ diameter) {
  __shared__ u64 s_A[kMsWaves], s_D[kMsWaves], s_d2[kMsWaves], s_ij[kMsWaves];
  __shared__ int s_k[kMsWaves];
  const int i = blockIdx.x;
  const int m = (int)(vert_ptr[i + 1] - vert_ptr[i]);
  long long* __restrict__ ob = box + (size_t)i * 8;
  long long* __restrict__ od = diameter + (size_t)i * 3;
  if (m < 1) {                                                         // (the whole workgroup)
    if (threadIdx.x < 8) ob[threadIdx.x] = 0;
    if (threadIdx.x < 3) od[threadIdx.x] = 0;
    return;
  }
  const int2* __restrict__ V = xy + vert_ptr[i];
  u64 rA = 0ull, rD = 1ull, fd2 = 0ull, fij = ~0ull;
  int rk = INT_MAX;
  long long b_tmin = 0, b_tmax = 0, b_smax = 0;
  for (int k = threadIdx.x; k < m; k += kMsThreads) {
    const int2 a = V[k], b = V[k + 1 < m ? k + 1 : 0];
    const long long ex = b.x - a.x, ey = b.y - a.y;
    long long tmin = 0, tmax = 0, smax = 0;                            // (p = a gives t = s = 0)
    for (int q = 0; q < m; ++q) {
      const int2 p = V[q];
      const long long dx = p.x - a.x, dy = p.y - a.y;
      const long long t = dx * ex + dy * ey, s = ex * dy - ey * dx;
      tmin = t < tmin ? t : tmin;
      tmax = t > tmax ? t : tmax;
      smax = s > smax ? s : smax;
      const u64 d2 = (u64)(dx * dx + dy * dy);
      if (q > k && d2 > fd2) {                                         // (k and q ascend: the lowest pair of this lane's)
        fd2 = d2;
        fij = ((u64)k << 32) | (u64)q;
      }
    }
    const u64 A = (u64)(tmax - tmin) * (u64)smax, D = (u64)(ex * ex + ey * ey);
    if (ms_rect_before(A, D, k, rA, rD, rk)) {
      rA = A; rD = D; rk = k;
      b_tmin = tmin; b_tmax = tmax; b_smax = smax;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 oA = __shfl_xor(rA, o), oD = __shfl_xor(rD, o);
    const int ok = __shfl_xor(rk, o);
    if (ms_rect_before(oA, oD, ok, rA, rD, rk)) { rA = oA; rD = oD; rk = ok; }
    const u64 od2 = __shfl_xor(fd2, o), oij = __shfl_xor(fij, o);
    if (ms_far_before(od2, oij, fd2, fij)) { fd2 = od2; fij = oij; }
  }
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    s_A[wv] = rA; s_D[wv] = rD; s_k[wv] = rk; s_d2[wv] = fd2; s_ij[wv] = fij;
  }
  __syncthreads();
  rA = s_A[0]; rD = s_D[0]; rk = s_k[0]; fd2 = s_d2[0]; fij = s_ij[0];
#pragma unroll
  for (int wv = 1; wv < kMsWaves; ++wv) {
    if (ms_rect_before(s_A[wv], s_D[wv], s_k[wv], rA, rD, rk)) { rA = s_A[wv]; rD = s_D[wv]; rk = s_k[wv]; }
    if (ms_far_before(s_d2[wv], s_ij[wv], fd2, fij)) { fd2 = s_d2[wv]; fij = s_ij[wv]; }
  }
  if (rk % kMsThreads == (int)threadIdx.x) {                           // the lane that took the winning edge still holds its ranges
    const int2 a = V[rk], b = V[rk + 1 < m ? rk + 1 : 0];
    ob[0] = rk; ob[1] = a.x; ob[2] = a.y; ob[3] = b.x - a.x; ob[4] = b.y - a.y;
    ob[5] = b_tmin; ob[6] = b_tmax; ob[7] = b_smax;
  }
  if (threadIdx.x == 0) {
    od[0] = (long long)fd2;
    od[1] = (long long)(fij >> 32);
    od[2] = (long long)(fij & 0xffffffffull);
  }
}

namespace {

// The instance table of a call and what its launches need.
struct MsPlan {
  std::vector<MsInst> inst;
  long long most_words = 0;     // of one instance
  int most_rows = 0;            // lattice rows (h + 1) of the tallest instance
  long long cands = 0;          // entries of the candidate and flag arrays; the vertices have that much room (a hull has at most
                                // two on a lattice row, so no count of kept flags can write past it)
};

// What every entry refuses about its set, and the plan.
int ms_check_set(const char* who, HostMaskSet* set, const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n,
                 MsPlan* plan) {
  MNC_REQUIRE(n >= 0 && n <= kMsMaxN, "%s: n=%d not in [0, %d]", who, n, kMsMaxN);
  const int rc = set->check(who, "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = set->info[i];
    MsInst m = MsInst();
    m.cand0 = (int)plan->cands;
    if (mask_has_rows(a)) {
      m.w = a.x2 - a.x1 + 1;
      m.h = a.y2 - a.y1 + 1;
      MNC_REQUIRE(m.w <= kMsMaxExtent && m.h <= kMsMaxExtent, "%s: masks[%d] is %d x %d (limit %d a side)", who, i, m.w, m.h,
                  kMsMaxExtent);
      m.src_words = a.offset / 8;
      m.x1 = a.x1;
      m.y1 = a.y1;
      const long long words = (long long)m.h * mask_strips(m.w);
      if (words > plan->most_words) plan->most_words = words;
      if (m.h + 1 > plan->most_rows) plan->most_rows = m.h + 1;
      plan->cands += 2 * (m.h + 1);                                   // (2048 instances of 32769 lattice rows: below 2^28)
    }
    plan->inst.push_back(m);
  }
  return MNC_OK;
}

// The device side of the hulls of one call.
struct MsHullWs {
  MsInst* inst;
  int *cand, *in_tile, *tile;
  unsigned char* flags;
  long long* vert_ptr;
  int2* xy;
  void take(WsLayout& l, const MsPlan& p) {
    inst = l.take<MsInst>(p.inst.size());
    cand = l.take<int>((size_t)p.cands);
    in_tile = l.take<int>((size_t)p.cands);
    tile = l.take<int>((size_t)scan_tiles(p.cands) + 1);
    flags = l.take<unsigned char>((size_t)p.cands);
    vert_ptr = l.take<long long>(p.inst.size() + 1);
    xy = l.take<int2>((size_t)p.cands);
  }
};

inline unsigned ms_blocks(long long count) { return (unsigned)((count + kMsThreads - 1) / kMsThreads); }

// vert_ptr, and with `place` the vertices: 5 resp. 6 launches.  p.cands >= 1.
void ms_hull_launch(hipStream_t s, const MsPlan& p, const MsHullWs& w, const u64* d_bits, bool place) {
  const unsigned n = (unsigned)p.inst.size();
  hipLaunchKernelGGL(ms_rows_kernel, dim3(ms_blocks(p.most_rows), n), dim3(kMsThreads), 0, s, w.inst, d_bits, w.cand);
  hipLaunchKernelGGL(ms_flags_kernel, dim3(ms_blocks(2ll * p.most_rows), n), dim3(kMsThreads), 0, s, w.inst, w.cand, w.flags);
  const Scanned kept = scan_launch(s, w.flags, (int)p.cands, w.in_tile, w.tile);
  hipLaunchKernelGGL(ms_ptr_kernel, dim3(ms_blocks(n + 1)), dim3(kMsThreads), 0, s, w.inst, (int)n, kept, w.vert_ptr);
  if (place)
    hipLaunchKernelGGL(ms_place_kernel, dim3(ms_blocks(2ll * p.most_rows), n), dim3(kMsThreads), 0, s, w.inst, w.cand, w.flags, kept,
                       w.xy);
}

CallTimer g_ms_timer;

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_moments(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, long long* moments,
                     int device_id) {
  const char* who = "mnc_mask_moments";
  MNC_REQUIRE(n <= 0 || moments, "%s: null moments", who);
  HostMaskSet set;
  MsPlan plan;
  int rc = ms_check_set(who, &set, bounds, offsets, bits, bytes, n, &plan);
  if (rc) return rc;
  for (size_t k = 0; k < (size_t)n * 6; ++k) moments[k] = 0;
  if (plan.most_words == 0) { clear_error(); return MNC_OK; }
  MsInst* d_inst; u64* d_out;
  auto layout = [&](WsLayout l) {
    set.take(l);
    d_inst = l.take<MsInst>(n);
    d_out = l.take<u64>((size_t)n * 6);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(set.upload(hs));
  MNC_HIP_TRY(hs.up(d_inst, plan.inst.data(), (size_t)n * sizeof(MsInst)));
  MNC_HIP_TRY(hs.up(d_out, moments, (size_t)n * 6 * sizeof(u64)));       // (zeros)
  TimedSpan span(g_ms_timer);
  span.begin(hs.stream);
  hipLaunchKernelGGL(ms_moments_kernel, dim3(ms_blocks(plan.most_words), (unsigned)n), dim3(kMsThreads), 0, hs.stream, d_inst,
                     set.d_bits, d_out);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(moments, d_out, (size_t)n * 6 * sizeof(u64)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_hull(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, long long* vert_ptr, int* xy,
                  long long* area2, size_t vert_cap, size_t* n_verts, int device_id) {
  const char* who = "mnc_mask_hull";
  MNC_REQUIRE(vert_ptr && n_verts, "%s: null vert_ptr or n_verts", who);
  MNC_REQUIRE(!xy || n <= 0 || area2, "%s: null area2", who);
  HostMaskSet set;
  MsPlan plan;
  int rc = ms_check_set(who, &set, bounds, offsets, bits, bytes, n, &plan);
  if (rc) return rc;
  if (plan.cands == 0) {                                   // no instance has a row
    for (int i = 0; i <= n; ++i) vert_ptr[i] = 0;
    *n_verts = 0;
    if (xy) for (int i = 0; i < n; ++i) area2[i] = 0;
    clear_error();
    return MNC_OK;
  }
  MsHullWs w; long long* d_area2;
  auto layout = [&](WsLayout l) {
    set.take(l);
    w.take(l, plan);
    d_area2 = l.take<long long>(n);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(set.upload(hs));
  MNC_HIP_TRY(hs.up(w.inst, plan.inst.data(), (size_t)n * sizeof(MsInst)));
  TimedSpan span(g_ms_timer);
  span.begin(hs.stream);
  ms_hull_launch(hs.stream, plan, w, set.d_bits, xy != nullptr);
  if (xy) hipLaunchKernelGGL(ms_area_kernel, dim3((unsigned)n), dim3(kMsThreads), 0, hs.stream, w.inst, w.vert_ptr, w.xy, d_area2);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(vert_ptr, w.vert_ptr, ((size_t)n + 1) * sizeof(long long)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  const size_t total = (size_t)vert_ptr[n];
  *n_verts = total;
  if (!xy) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(vert_cap >= total, "%s: vert_cap %zu is below the %zu vertices of the hulls", who, vert_cap, total);
  MNC_HIP_TRY(hs.down(xy, w.xy, total * sizeof(int2)));
  MNC_HIP_TRY(hs.down(area2, d_area2, (size_t)n * sizeof(long long)));
  MNC_HIP_TRY(hs.sync());
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_oriented(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, long long* box,
                      long long* diameter, int device_id) {
  const char* who = "mnc_mask_oriented";
  MNC_REQUIRE(n <= 0 || (box && diameter), "%s: null output pointer", who);
  HostMaskSet set;
  MsPlan plan;
  int rc = ms_check_set(who, &set, bounds, offsets, bits, bytes, n, &plan);
  if (rc) return rc;
  if (plan.cands == 0) {
    for (size_t k = 0; k < (size_t)n * 8; ++k) box[k] = 0;
    for (size_t k = 0; k < (size_t)n * 3; ++k) diameter[k] = 0;
    clear_error();
    return MNC_OK;
  }
  MsHullWs w; long long *d_box, *d_diameter;
  auto layout = [&](WsLayout l) {
    set.take(l);
    w.take(l, plan);
    d_box = l.take<long long>((size_t)n * 8);
    d_diameter = l.take<long long>((size_t)n * 3);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(set.upload(hs));
  MNC_HIP_TRY(hs.up(w.inst, plan.inst.data(), (size_t)n * sizeof(MsInst)));
  TimedSpan span(g_ms_timer);
  span.begin(hs.stream);
  ms_hull_launch(hs.stream, plan, w, set.d_bits, true);
  hipLaunchKernelGGL(ms_calipers_kernel, dim3((unsigned)n), dim3(kMsThreads), 0, hs.stream, w.vert_ptr, w.xy, d_box, d_diameter);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(box, d_box, (size_t)n * 8 * sizeof(long long)));
  MNC_HIP_TRY(hs.down(diameter, d_diameter, (size_t)n * 3 * sizeof(long long)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_shape_timing(int on, double* last_ms) { return g_ms_timer.set(on, last_ms); }
