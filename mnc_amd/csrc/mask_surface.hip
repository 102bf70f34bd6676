// Surface distances between packed instance masks (include/mnc_hip.h n22), for gfx950, on the PackedMasks layout of inst_masks.hip
// (n5), without unpacking a mask: the surfaces S(M) = M & ~erode(M, r2 = 1), and for pairs (i, j) of instances of two sets and
// either direction the squared distance from every surface pixel of the one to the nearest surface pixel of the other -- raw, or
// reduced to the count, the maximum with its place, the sum and the counts within up to 8 squared tolerances: what the Hausdorff
// distance, HD95, ASSD, the boundary F-measure and the surface Dice are made of.  The statements of the rules are
// mnc_amd/surface.py:surface_numpy, surface_stats_numpy and surface_distances_numpy; this file computes the same integers.  There
// is no floating point.
//
// The instances of both sets are numbered as one: A's 0 .. n - 1, then B's.  The words of their rows are numbered in that order,
// row-major inside an instance; the surface planes, the popcounts and their prefix sums use this numbering.
//
//   sf_surface_kernel    one lane per word: v & ~(up & down & ((v << 1) | carry from the left) & ((v >> 1) | carry from the
//                        right)), rows and words beyond the bounds reading 0 and padding bits cleared (mask_word), into the
//                        surface plane; the popcount beside it for the raw entry; the wave's popcounts added to the instance's
//                        count by one integer atomic.
//   sf_gap_kernel        for every instance some pair uses as a destination: one lane per pixel of its bounds, a wave per word:
//                        g, the distance along the row to the nearest surface pixel, from the lane's own word below and above its
//                        bit (__clzll / __ffsll) and, while none is found, from the neighbouring words one after the other up to
//                        the row's ends; 0xffff where the row has none.  Stored as uint16 with row stride w -- md_gap_kernel's
//                        walk (mask_distance.hip) on the surface words.
//   sf_query_kernel<R>   a workgroup owns 64 consecutive words of the source of one (pair, direction), a wave 16 of them: lane t
//                        loads word t, the wave visits the words that have a bit, and in a visited word lane b owns bit b.  A lane
//                        with a set bit at (x, y) clamps x into the destination's columns -- every surface pixel of a row lies on
//                        one side of an x outside them, so dx = |x - clamp(x)| + g[row][clamp(x)] -- and walks the destination's
//                        rows outward from clamp(y) while dy^2 < best: the cost of a pixel grows with its distance, not with the
//                        destination's surface, and no lane walks bits.  <1>, raw: best is stored at the slot's base plus the
//                        pixel's rank, the prefix sum of the popcounts before its word plus the popcount below its bit; a slot
//                        whose destination has no surface stores 0xffffffff.  <0>, statistics: the sum, the counts within the
//                        tolerances and the 64-bit key (d2 << 32) | (0xffffffff - raster index) are reduced by shuffles, then LDS,
//                        then one 64-bit atomic add resp. max per workgroup and figure: the greatest d2 at its lowest (y, x).
// The workgroups of the query are listed on the host from the bounds alone (the prefix sum of ceil(words / 64) over the slots), so
// no workgroup is launched for nothing and the launch count is fixed: 3 for the statistics (1 where no pair has a destination with
// rows), 1 for the surfaces, and for the raw entry 1 before its one read-back (the counts, from which the host makes ptr) and the
// scan's 2, the gaps and the query after it.  Every raw entry and every surface word is written once by vector stores; the only
// atomics are integer add and max, which commute: the same input gives the same bytes on every run.  No loop's trip count depends
// on another wave's progress.
//
// Bound: latency and lane occupancy.  A surface word holds a few pixels of an outline, so most lanes of a visiting wave idle while
// the few walk; the g plane is two bytes a pixel and stays in L2.  Measured at 100 instances against 20 ground truths of a
// 600 x 1000 image (92 x 10^3 surface pixels in the 100), kernels alone: the 20 matched pairs 38 us of a 0.17 ms statistics call and
// 47 us of a 0.29 ms raw call (39 x 10^3 distances); all 2000 pairs, most of them far apart, so that a pixel walks every row of the
// other bound, 2.7 ms of 2.9 ms and 2.6 ms of 3.4 ms (3.8 x 10^6 distances).  The loop over full(i, H, W) with scipy's distance
// transform per pair takes 571 ms for the 20 in the same run and, scaled from 40 of them, 28 s for the 2000
// (profiles/surface_dist_bench.txt).
// Registers, LDS and scratch, from the code object: sf_surface_kernel 20 VGPRs, sf_gap_kernel 17, sf_query_kernel<0> 36 and 320
// bytes of LDS, <1> 17; no scratch in any of them.
#include <algorithm>
#include <climits>
#include <vector>

#include "mask_set.h"
#include "scan.h"

namespace mnc {

constexpr int kSfThreads = 256;
constexpr int kSfWaves = kSfThreads / 64;
constexpr int kSfWaveWords = 16;                         // source words of one wave of the query
constexpr int kSfBlockWords = kSfWaves * kSfWaveWords;
constexpr int kSfMaxN = 2048;                            // instances of one set (mnc_mask_boundary's limit)
constexpr int kSfMaxPairs = 65536;
constexpr int kSfMaxTau = 8;
constexpr int kSfMaxSpan = 32768;                        // the hull of all bounds spans fewer pixels than this in either axis
constexpr long long kSfMaxPixels = 1ll << 27;            // pixels of the rows of both sets
constexpr long long kSfMaxEntries = 1ll << 28;           // raw distances of one call
constexpr unsigned kSfNone = 0xffffffffu;                // the distance to an empty surface
constexpr unsigned kSfNoGap = 0xffffu;                   // g of a row without a surface pixel
constexpr int kSfFigures = 2 + kSfMaxTau;                // per slot of the statistics: the sum, the key, the counts within
constexpr long long kSfMaxGrid = 1ll << 22;              // workgroups of one query launch; the rest by a grid stride

// One instance of the joint numbering.  Without rows: w = h = strips = 0.
struct SfInst {
  long long src_words;        // first word of its rows, from the first word of set A on the device
  long long first;            // number of its first word = its place in the surface plane, the popcounts and their prefix sums
  long long g_off;            // first entry of its bounds in the g plane (destinations only)
  int x1, y1, w, h;
  int strips, pad_;
};

// One (pair, direction): the source's surface pixels are measured against the destination's surface.
struct SfSlot {
  long long first_block;      // the workgroups of the slots before it
  long long base;             // first raw entry
  int src, dst;
};

struct SfTau { int t[kSfMaxTau]; };

__device__ __forceinline__ u64 sf_lane_read(u64 v, int t) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, t);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), t);
  return ((u64)hi << 32) | lo;
}

// grid (ceil(most words / 256), instances), block 256.  pc may be null.  count [instances]: zero before.
__global__ __launch_bounds__(kSfThreads) void sf_surface_kernel(const SfInst* __restrict__ insts, const u64* __restrict__ bits,
                                                                u64* __restrict__ surf, int* __restrict__ pc,
                                                                u64* __restrict__ count) {
  const SfInst a = insts[blockIdx.y];
  const int words = a.h * a.strips;                      // (at most 2^27)
  if ((long long)blockIdx.x * kSfThreads >= words) return;             // (the whole workgroup)
  const int idx = (int)blockIdx.x * kSfThreads + (int)threadIdx.x;
  u64 s = 0ull;
  if (idx < words) {
    const int r = idx / a.strips, j = idx - r * a.strips;
    const u64* row = bits + a.src_words + (long long)r * a.strips;
    const u64 v = mask_word(row, j, a.strips, a.w);
    if (v) {
      const u64 up = r > 0 ? mask_word(row - a.strips, j, a.strips, a.w) : 0ull;
      const u64 down = r + 1 < a.h ? mask_word(row + a.strips, j, a.strips, a.w) : 0ull;
      const u64 left = mask_word(row, j - 1, a.strips, a.w), right = mask_word(row, j + 1, a.strips, a.w);
      s = v & ~(up & down & ((v << 1) | (left >> 63)) & ((v >> 1) | (right << 63)));
    }
    surf[a.first + idx] = s;
    if (pc) pc[a.first + idx] = __popcll(s);
  }
  unsigned c = (unsigned)__popcll(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&count[blockIdx.y], (u64)c);
}

// grid (ceil(most destination words / 4), destinations), block 256: a wave per word of the bounds.
__global__ __launch_bounds__(kSfThreads) void sf_gap_kernel(const SfInst* __restrict__ insts, const int* __restrict__ dst,
                                                            const u64* __restrict__ surf, unsigned short* __restrict__ g) {
  const SfInst a = insts[dst[blockIdx.y]];
  const int words = a.h * a.strips;
  const long long word = (long long)blockIdx.x * kSfWaves + (threadIdx.x >> 6);
  if (word >= words) return;                             // (the whole wave)
  const int y = (int)word / a.strips, j = (int)word - y * a.strips, b = threadIdx.x & 63;
  const u64* row = surf + a.first + (long long)y * a.strips;
  int dist = (int)kSfNoGap;
  const u64 z0 = row[j];
  // at or below this bit: the highest one of word j - k stands 64 k + b - hi columns before
  u64 z = z0 & ((2ull << b) - 1ull);
  for (int k = 0;;) {
    if (z) {
      dist = min(dist, 64 * k + b - (63 - __clzll((long long)z)));
      break;
    }
    ++k;
    if (j - k < 0) break;
    z = row[j - k];
  }
  // at or above it: the lowest one of word j + k stands 64 k + lo - b columns after
  z = z0 & (~0ull << b);
  for (int k = 0;;) {
    if (z) {
      dist = min(dist, 64 * k + (__ffsll((long long)z) - 1) - b);
      break;
    }
    ++k;
    if (j + k >= a.strips) break;
    z = row[j + k];
  }
  const int x = j * 64 + b;
  if (x < a.w) g[a.g_off + (long long)y * a.w + x] = (unsigned short)dist;
}

// The squared distance from image pixel (x, y) to the nearest surface pixel of destination d, which has one.  With the hull of
// all bounds below 32768 pixels a side, dx and dy stay below 32768 and every sum below 2^31.
__device__ __forceinline__ unsigned sf_nearest(const SfInst& d, const unsigned short* __restrict__ g, int x, int y) {
  const int cx = min(max(x, d.x1), d.x1 + d.w - 1), cy = min(max(y, d.y1), d.y1 + d.h - 1);
  const unsigned dx0 = (unsigned)abs(x - cx), dy0 = (unsigned)abs(y - cy);
  const unsigned short* col = g + d.g_off + (cx - d.x1);
  const int r0 = cy - d.y1;
  unsigned best = kSfNone;
  for (int k = 0;; ++k) {
    const unsigned dy = dy0 + (unsigned)k, dd = dy * dy;
    const int ru = r0 - k, rd = r0 + k;
    if (dd >= best || (ru < 0 && rd >= d.h)) break;
    if (ru >= 0) {
      const unsigned u = col[(long long)ru * d.w];
      if (u != kSfNoGap) best = min(best, (dx0 + u) * (dx0 + u) + dd);
    }
    if (k > 0 && rd < d.h) {
      const unsigned u = col[(long long)rd * d.w];
      if (u != kSfNoGap) best = min(best, (dx0 + u) * (dx0 + u) + dd);
    }
  }
  return best;
}

// grid min(blocks, kSfMaxGrid), block 256.  slots [n_slots + 1], slots[n_slots].first_block = blocks.  count: the surface pixels
// of every instance.  kRaw: d2 receives every source pixel's distance at slot base + rank (ranks: the scanned popcounts).
// Otherwise out [n_slots][kSfFigures], zero before, receives the sum, the key and the counts within tau.t[0 .. T - 1].
template <int kRaw>
__global__ __launch_bounds__(kSfThreads) void sf_query_kernel(const SfInst* __restrict__ insts, const SfSlot* __restrict__ slots,
                                                              int n_slots, long long blocks, const u64* __restrict__ surf,
                                                              const unsigned short* __restrict__ g, const u64* __restrict__ count,
                                                              Scanned ranks, unsigned* __restrict__ d2, SfTau tau, int T,
                                                              u64* __restrict__ out) {
  __shared__ u64 s_part[kSfWaves][kSfFigures];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    int lo = 0, hi = n_slots - 1;                        // the last slot whose first workgroup is at or before blk: 17 turns
    for (int turn = 0; turn < 18 && lo < hi; ++turn) {
      const int mid = (lo + hi + 1) >> 1;
      if (slots[mid].first_block <= blk) lo = mid; else hi = mid - 1;
    }
    const SfSlot sl = slots[lo];
    const SfInst a = insts[sl.src], d = insts[sl.dst];
    const bool reach = count[sl.dst] != 0ull;            // the destination has a surface
    if (!kRaw && !reach) continue;                       // (the whole workgroup; the host answers such a slot)
    const int words = a.h * a.strips;
    const int w0 = (int)(blk - sl.first_block) * kSfBlockWords + wv * kSfWaveWords;
    const int mine = w0 + lane;
    u64 my_v = 0ull;
    if (lane < kSfWaveWords && mine < words) my_v = surf[a.first + mine];
    u64 live = __ballot(my_v != 0ull);                   // the words of this wave that have a surface pixel
    u64 sum = 0ull, key = 0ull;
    unsigned in[kSfMaxTau];
#pragma unroll
    for (int t = 0; t < kSfMaxTau; ++t) in[t] = 0u;
    while (live) {
      const int t = __ffsll((long long)live) - 1;
      live &= live - 1ull;
      const u64 v = sf_lane_read(my_v, t);
      if ((v >> lane) & 1ull) {                          // (the loop's own condition is the same in every lane)
        const int idx = w0 + t, r = idx / a.strips, xo = (idx - r * a.strips) * 64 + lane;
        const unsigned best = reach ? sf_nearest(d, g, a.x1 + xo, a.y1 + r) : kSfNone;
        if (kRaw) {
          const int rank = ranks.at((int)a.first + idx) - ranks.at((int)a.first) + __popcll(v & ((1ull << lane) - 1ull));
          d2[sl.base + rank] = best;
        } else {
          sum += (u64)best;
          const u64 k = ((u64)best << 32) | (u64)(0xffffffffu - (unsigned)(r * a.w + xo));
          key = k > key ? k : key;
#pragma unroll
          for (int q = 0; q < kSfMaxTau; ++q) in[q] += q < T && best <= (unsigned)tau.t[q] ? 1u : 0u;
        }
      }
    }
    if (kRaw) continue;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o);
      const u64 k = __shfl_xor(key, o);
      key = k > key ? k : key;
#pragma unroll
      for (int q = 0; q < kSfMaxTau; ++q) in[q] += __shfl_xor(in[q], o);
    }
    if (lane == 0) {
      s_part[wv][0] = sum;
      s_part[wv][1] = key;
#pragma unroll
      for (int q = 0; q < kSfMaxTau; ++q) s_part[wv][2 + q] = (u64)in[q];
    }
    __syncthreads();
    const int f = threadIdx.x;
    if (f < kSfFigures) {
      u64 t = s_part[0][f];
#pragma unroll
      for (int w2 = 1; w2 < kSfWaves; ++w2) {
        const u64 o = s_part[w2][f];
        t = f == 1 ? (o > t ? o : t) : t + o;
      }
      u64* at = out + (size_t)lo * kSfFigures + f;
      if (t) {
        if (f == 1) atomicMax(at, t); else atomicAdd(at, t);
      }
    }
    __syncthreads();                                     // s_part is written again
  }
}

namespace {

CallTimer g_sf_timer;
// The raw distances of a call, per device: sized once the counts are read back (the HostScope workspace holds what is known before
// the first launch and cannot grow without losing it).  Guarded by the HostScope's mutex, which the call holds to its end.
DevArena g_sf_raw[16];

// The checked call: both sets, the joint instance table, the slots and what the launches need.
struct SfPlan {
  HostMaskSet A, B;
  std::vector<SfInst> inst;
  std::vector<SfSlot> slot;    // 2 P + 1
  std::vector<int> dst;        // the instances with rows that some pair measures against
  long long words = 0;         // of all rows
  long long g_entries = 0;
  int most_words = 0, most_dst_words = 0;
  long long blocks = 0;        // workgroups of the query
  SfInst* d_inst = nullptr; SfSlot* d_slot = nullptr; int* d_dst = nullptr;
  u64 *d_surf = nullptr, *d_count = nullptr;
  unsigned short* d_g = nullptr;
  void take(WsLayout& l) {
    A.take(l);
    B.take(l);
    d_inst = l.take<SfInst>(inst.size());
    d_slot = l.take<SfSlot>(slot.size());
    d_dst = l.take<int>(dst.size());
    d_surf = l.take<u64>((size_t)words);
    d_g = l.take<unsigned short>((size_t)g_entries);
    d_count = l.take<u64>(inst.size());
  }
  // after take() on the real buffer: B's words are addressed from A's first word
  hipError_t upload(const HostScope& hs) {
    const long long delta = (long long)(B.d_bits - A.d_bits);
    for (size_t c = A.info.size(); c < inst.size(); ++c) inst[c].src_words += delta;
    hipError_t e = A.upload(hs);
    if (e == hipSuccess) e = B.upload(hs);
    if (e == hipSuccess) e = hs.up(d_inst, inst.data(), inst.size() * sizeof(SfInst));
    if (e == hipSuccess) e = hs.up(d_slot, slot.data(), slot.size() * sizeof(SfSlot));
    if (e == hipSuccess) e = hs.up(d_dst, dst.data(), dst.size() * sizeof(int));
    return e;
  }
  void launch_surface(hipStream_t s, int* d_pc) const {
    hipLaunchKernelGGL(sf_surface_kernel, dim3((unsigned)((most_words + kSfThreads - 1) / kSfThreads), (unsigned)inst.size()),
                       dim3(kSfThreads), 0, s, d_inst, A.d_bits, d_surf, d_pc, d_count);
  }
  void launch_gap(hipStream_t s) const {
    if (dst.empty()) return;
    hipLaunchKernelGGL(sf_gap_kernel, dim3((unsigned)((most_dst_words + kSfWaves - 1) / kSfWaves), (unsigned)dst.size()),
                       dim3(kSfThreads), 0, s, d_inst, d_dst, d_surf, d_g);
  }
  template <int kRaw>
  void launch_query(hipStream_t s, Scanned ranks, unsigned* d_d2, const SfTau& tau, int T, u64* d_out) const {
    if (blocks < 1) return;
    hipLaunchKernelGGL(sf_query_kernel<kRaw>, dim3((unsigned)std::min(blocks, kSfMaxGrid)), dim3(kSfThreads), 0, s, d_inst, d_slot,
                       (int)slot.size() - 1, blocks, d_surf, d_g, d_count, ranks, d_d2, tau, T, d_out);
  }
};

// What the entries refuse about their sets and pairs, before anything is launched; the plan of what they accept.  No set B
// (mnc_mask_surface): m = 0 and P = 0.
int sf_check(const char* who, SfPlan* p, const int* a_bounds, const long long* a_offsets, const void* a_bits, size_t a_bytes, int n,
             const int* b_bounds, const long long* b_offsets, const void* b_bits, size_t b_bytes, int m, const int* pairs, int P) {
  MNC_REQUIRE(n >= 0 && n <= kSfMaxN && m >= 0 && m <= kSfMaxN, "%s: n=%d or m=%d not in [0, %d]", who, n, m, kSfMaxN);
  MNC_REQUIRE(P >= 0 && P <= kSfMaxPairs, "%s: P=%d not in [0, %d]", who, P, kSfMaxPairs);
  MNC_REQUIRE(P == 0 || pairs, "%s: null pairs", who);
  int rc = p->A.check(who, "a", a_bounds, a_offsets, a_bits, a_bytes, n, nullptr, nullptr);
  if (rc) return rc;
  rc = p->B.check(who, "b", b_bounds, b_offsets, b_bits, b_bytes, m, nullptr, nullptr);
  if (rc) return rc;
  for (int k = 0; k < P; ++k)
    MNC_REQUIRE(pairs[2 * k] >= 0 && pairs[2 * k] < n && pairs[2 * k + 1] >= 0 && pairs[2 * k + 1] < m,
                "%s: pairs[%d] = (%d, %d) not in [0, %d) x [0, %d)", who, k, pairs[2 * k], pairs[2 * k + 1], n, m);
  int hx1 = INT_MAX, hy1 = INT_MAX, hx2 = INT_MIN, hy2 = INT_MIN;
  long long pixels = 0;
  p->inst.assign((size_t)n + m, SfInst());
  for (int c = 0; c < n + m; ++c) {
    const mnc_mask_info& a = c < n ? p->A.info[c] : p->B.info[c - n];
    SfInst& q = p->inst[c];
    q.first = p->words;
    q.g_off = 0;
    if (!mask_has_rows(a)) continue;
    hx1 = std::min(hx1, a.x1); hy1 = std::min(hy1, a.y1); hx2 = std::max(hx2, a.x2); hy2 = std::max(hy2, a.y2);
    q.src_words = a.offset / 8;
    q.x1 = a.x1; q.y1 = a.y1; q.w = a.x2 - a.x1 + 1; q.h = a.y2 - a.y1 + 1;
    q.strips = mask_strips(q.w);
    pixels += (long long)q.w * q.h;
    p->words += (long long)q.h * q.strips;
  }
  MNC_REQUIRE(hx2 < hx1 || ((long long)hx2 - hx1 < kSfMaxSpan - 1 && (long long)hy2 - hy1 < kSfMaxSpan - 1),
              "%s: the bounds span %lld x %lld pixels (limit %d a side)", who, (long long)hx2 - hx1 + 1, (long long)hy2 - hy1 + 1,
              kSfMaxSpan - 1);
  MNC_REQUIRE(pixels <= kSfMaxPixels, "%s: %lld pixels of rows in the call (limit %lld)", who, pixels, kSfMaxPixels);
  for (const SfInst& q : p->inst) p->most_words = std::max(p->most_words, q.h * q.strips);
  // the slots, their workgroups, and the destinations' place in the g plane
  std::vector<char> is_dst((size_t)n + m, 0);
  p->slot.assign(2 * (size_t)P + 1, SfSlot());
  for (int k = 0; k < P; ++k) {
    const int i = pairs[2 * k], j = n + pairs[2 * k + 1];
    for (int dir = 0; dir < 2; ++dir) {
      SfSlot& s = p->slot[2 * (size_t)k + dir];
      s.src = dir ? j : i;
      s.dst = dir ? i : j;
      s.first_block = p->blocks;
      const SfInst& src = p->inst[s.src];
      p->blocks += (src.h * src.strips + kSfBlockWords - 1) / kSfBlockWords;
      is_dst[s.dst] = 1;
    }
  }
  p->slot[2 * (size_t)P].first_block = p->blocks;
  for (int c = 0; c < n + m; ++c) {
    SfInst& q = p->inst[c];
    if (!is_dst[c] || q.h < 1) continue;
    q.g_off = p->g_entries;
    p->g_entries += (long long)q.w * q.h;
    p->most_dst_words = std::max(p->most_dst_words, q.h * q.strips);
    p->dst.push_back(c);
  }
  return MNC_OK;
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_surface(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int* out_bounds,
                     long long* out_offsets, long long* out_areas, void* out_bits, size_t bits_cap, size_t* bits_bytes,
                     int device_id) {
  const char* who = "mnc_mask_surface";
  MNC_REQUIRE(bits_bytes, "%s: null bits_bytes", who);
  MNC_REQUIRE(n <= 0 || (out_bounds && out_offsets), "%s: null output pointer", who);
  MNC_REQUIRE(n <= 0 || !out_bits || out_areas, "%s: null out_areas", who);
  SfPlan plan;
  int rc = sf_check(who, &plan, bounds, offsets, bits, bytes, n, nullptr, nullptr, nullptr, 0, 0, nullptr, 0);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 4; ++k) out_bounds[4 * (size_t)i + k] = bounds[4 * (size_t)i + k];
    out_offsets[i] = plan.inst[i].first * 8;
  }
  const size_t need = (size_t)plan.words * 8;
  *bits_bytes = need;
  if (!out_bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(bits_cap >= need, "%s: bits_cap %zu is below the %zu bytes of the result", who, bits_cap, need);
  for (int i = 0; i < n; ++i) out_areas[i] = 0;
  if (need == 0) { clear_error(); return MNC_OK; }       // no instance has a row
  auto layout = [&](WsLayout l) {
    plan.take(l);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(plan.upload(hs));
  MNC_HIP_TRY(hipMemsetAsync(plan.d_count, 0, (size_t)n * sizeof(u64), hs.stream));
  TimedSpan span(g_sf_timer);
  span.begin(hs.stream);
  plan.launch_surface(hs.stream, nullptr);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(out_areas, plan.d_count, (size_t)n * sizeof(u64)));
  MNC_HIP_TRY(hs.down(out_bits, plan.d_surf, need));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_surface_stats(const int* a_bounds, const long long* a_offsets, const void* a_bits, size_t a_bytes, int n,
                           const int* b_bounds, const long long* b_offsets, const void* b_bits, size_t b_bytes, int m,
                           const int* pairs, int P, const int* tau2, int T, long long* count, long long* max_d2, int* argmax,
                           long long* sum_d2, long long* within, int device_id) {
  const char* who = "mnc_mask_surface_stats";
  MNC_REQUIRE(T >= 0 && T <= kSfMaxTau, "%s: T=%d not in [0, %d]", who, T, kSfMaxTau);
  MNC_REQUIRE(T == 0 || tau2, "%s: null tau2", who);
  SfTau tau = SfTau();
  for (int t = 0; t < T; ++t) {
    MNC_REQUIRE(tau2[t] >= 0, "%s: tau2[%d]=%d not in [0, 2^31)", who, t, tau2[t]);
    tau.t[t] = tau2[t];
  }
  MNC_REQUIRE(P <= 0 || (count && max_d2 && argmax && sum_d2 && (T == 0 || within)), "%s: null output pointer", who);
  SfPlan plan;
  int rc = sf_check(who, &plan, a_bounds, a_offsets, a_bits, a_bytes, n, b_bounds, b_offsets, b_bits, b_bytes, m, pairs, P);
  if (rc) return rc;
  if (P == 0) { clear_error(); return MNC_OK; }
  const size_t slots = 2 * (size_t)P, insts = plan.inst.size();
  std::vector<u64> h_blk(insts + slots * kSfFigures, 0ull);          // the counts of the instances, then the figures of the slots
  if (plan.words > 0) {
    u64* d_out;
    auto layout = [&](WsLayout l) {
      plan.take(l);
      d_out = l.take<u64>(slots * kSfFigures);
      return l.bytes();
    };
    HostScope hs;
    rc = hs.open(device_id, layout(WsLayout()));
    if (rc) return rc;
    layout(WsLayout(hs.buf));
    MNC_HIP_TRY(plan.upload(hs));
    MNC_HIP_TRY(hipMemsetAsync(plan.d_count, 0, insts * sizeof(u64), hs.stream));
    MNC_HIP_TRY(hipMemsetAsync(d_out, 0, slots * kSfFigures * sizeof(u64), hs.stream));
    TimedSpan span(g_sf_timer);
    span.begin(hs.stream);
    plan.launch_surface(hs.stream, nullptr);
    plan.launch_gap(hs.stream);
    plan.launch_query<0>(hs.stream, Scanned{nullptr, nullptr, 0, 0}, nullptr, tau, T, d_out);
    span.end(hs.stream);
    MNC_HIP_TRY(hipGetLastError());
    MNC_HIP_TRY(hs.down(h_blk.data(), plan.d_count, insts * sizeof(u64)));
    MNC_HIP_TRY(hs.down(h_blk.data() + insts, d_out, slots * kSfFigures * sizeof(u64)));
    MNC_HIP_TRY(hs.sync());
    span.keep();
  }
  for (size_t s = 0; s < slots; ++s) {
    const SfSlot& sl = plan.slot[s];
    const u64* f = h_blk.data() + insts + s * kSfFigures;
    const u64 c_src = h_blk[sl.src], c_dst = h_blk[sl.dst];
    count[s] = (long long)c_src;
    const bool none = c_src == 0ull || c_dst == 0ull;
    sum_d2[s] = none ? 0 : (long long)f[0];
    for (int t = 0; t < T; ++t) within[s * T + t] = none ? 0 : (long long)f[2 + t];
    if (none) {
      max_d2[s] = -1; argmax[2 * s] = -1; argmax[2 * s + 1] = -1;
      continue;
    }
    const SfInst& a = plan.inst[sl.src];
    const unsigned at = 0xffffffffu - (unsigned)(f[1] & 0xffffffffull);
    max_d2[s] = (long long)(f[1] >> 32);
    argmax[2 * s] = a.x1 + (int)(at % (unsigned)a.w);
    argmax[2 * s + 1] = a.y1 + (int)(at / (unsigned)a.w);
  }
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_surface_dist(const int* a_bounds, const long long* a_offsets, const void* a_bits, size_t a_bytes, int n,
                          const int* b_bounds, const long long* b_offsets, const void* b_bits, size_t b_bytes, int m,
                          const int* pairs, int P, long long* ptr, unsigned* d2, size_t cap, size_t* total, int device_id) {
  const char* who = "mnc_mask_surface_dist";
  MNC_REQUIRE(ptr && total, "%s: null ptr or total", who);
  SfPlan plan;
  int rc = sf_check(who, &plan, a_bounds, a_offsets, a_bits, a_bytes, n, b_bounds, b_offsets, b_bits, b_bytes, m, pairs, P);
  if (rc) return rc;
  const size_t slots = 2 * (size_t)P, insts = plan.inst.size();
  if (P == 0 || plan.words == 0) {                       // no pair, or no surface pixel anywhere
    for (size_t s = 0; s <= slots; ++s) ptr[s] = 0;
    *total = 0;
    clear_error();
    return MNC_OK;
  }
  int *d_pc, *d_tile;
  auto layout = [&](WsLayout l) {
    plan.take(l);
    d_pc = l.take<int>((size_t)plan.words);
    d_tile = l.take<int>((size_t)scan_tiles(plan.words) + 1);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  std::vector<u64> h_count(insts, 0ull);
  MNC_HIP_TRY(plan.upload(hs));
  MNC_HIP_TRY(hipMemsetAsync(plan.d_count, 0, insts * sizeof(u64), hs.stream));
  TimedSpan first(g_sf_timer), second(g_sf_timer);
  first.begin(hs.stream);
  plan.launch_surface(hs.stream, d_pc);
  first.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(h_count.data(), plan.d_count, insts * sizeof(u64)));
  MNC_HIP_TRY(hs.sync());                                  // the one read-back: the surface pixels of every instance
  long long entries = 0;
  for (size_t s = 0; s < slots; ++s) {
    plan.slot[s].base = entries;
    entries += (long long)h_count[plan.slot[s].src];
    MNC_REQUIRE(entries <= kSfMaxEntries, "%s: more than %lld distances in the call", who, kSfMaxEntries);
  }
  for (size_t s = 0; s < slots; ++s) ptr[s] = plan.slot[s].base;
  ptr[slots] = entries;
  *total = (size_t)entries;
  if (!d2 || entries == 0) {
    first.keep();
    clear_error();
    return MNC_OK;
  }
  MNC_REQUIRE(cap >= (size_t)entries, "%s: cap %zu is below the %lld distances of the pairs", who, cap, entries);
  rc = arena_ensure(&g_sf_raw[device_id], (size_t)entries * sizeof(unsigned), ((size_t)entries << 1) + 4096, "surface distances",
                    hs.stream);
  if (rc) return rc;
  unsigned* d_d2 = (unsigned*)g_sf_raw[device_id].p;
  MNC_HIP_TRY(hs.up(plan.d_slot, plan.slot.data(), plan.slot.size() * sizeof(SfSlot)));      // (with the bases)
  second.begin(hs.stream);
  const Scanned ranks = scan_launch(hs.stream, d_pc, (int)plan.words, d_tile);
  plan.launch_gap(hs.stream);
  plan.launch_query<1>(hs.stream, ranks, d_d2, SfTau(), 0, nullptr);
  second.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(d2, d_d2, (size_t)entries * sizeof(unsigned)));
  MNC_HIP_TRY(hs.sync());
  second.keep_sum(first);
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_surface_timing(int on, double* last_ms) { return g_sf_timer.set(on, last_ms); }
