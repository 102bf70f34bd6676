// Outlines simplified to a pixel tolerance for gfx950 (include/mnc_hip.h n14): Douglas-Peucker on closed integer loops, in exact
// integer arithmetic, so that this parallel form equals the sequential statement (mnc_amd/contours.py:simplify_numpy) byte for byte.
// There is no floating point in this translation unit.
//
// Every decision of the rule is a pure function of a segment's vertices: the arg-max of the 128-bit numerator N over the vertices
// strictly between its ends, the lowest index on ties, and one comparison 256 N > q^2 D.  So the segments may be visited in any
// order; only the kept flags leave the two simplify kernels, and a scan in index order places the vertices.
//   cs_wave_kernel    one wave per loop of at most 64 vertices (most loops of a mask are pinholes of 4 - 12): lane t holds vertex
//                     t, the kept vertices and the closed segments are two 64-bit masks that every lane holds alike, a segment's
//                     ends come by shuffle.  No LDS, no barrier.  Loops of at most 3 vertices are kept whole here.
//   cs_block_kernel   one workgroup of 8 waves per longer loop (the workgroups stride over the loops and pass the short ones by).
//                     The anchor B and the two chains are reduced by the whole workgroup; then rounds: the open segments lie in
//                     one of two lists (k / 2 entries each: open segments are disjoint and have an inner vertex), every wave
//                     takes segments of the current list, reduces the arg-max and, where the vertex is kept, appends the two
//                     halves that still have an inner vertex to the other list (one LDS atomic hands out the slots: their order
//                     varies from run to run, no flag does).  The rounds end when a list stays empty: as many as the recursion is
//                     deep, k / 2 at the most, all inside the one launch, a barrier each.  Up to kCsLdsVerts vertices a loop's
//                     vertices and lists are staged in LDS; a longer loop is read from global memory and has its lists there.
//   scan_launch       (scan.hip: two launches) the exclusive prefix of the kept flags: in tiles of 1024, then over the tiles.
//   cs_write_kernel   one thread per vertex: a kept vertex and its index into the slot the prefix names; one per loop: the prefix
//                     at its first vertex is its new vert_ptr.
// One memset (the flags) and five launches whatever the data; V' is read back once, to size the copies of the result.
// cs_launch takes device pointers alone: an entry that simplifies the device buffers of mnc_mask_contours is a wrapper of it.
#include <vector>

#include "mnc_internal.h"
#include "scan.h"

namespace mnc {

typedef unsigned __int128 u128;
typedef unsigned long long cs_u64;

constexpr int kCsThreads = 256;
constexpr int kCsWaves = kCsThreads / 64;
constexpr int kCsWaveVerts = 64;                  // loops up to here: one wave
constexpr int kCsBlockThreads = 512;              // cs_block_kernel: 8 waves, a segment each
constexpr int kCsBlockWaves = kCsBlockThreads / 64;
constexpr int kCsLdsVerts = 4096;                 // loops up to here: vertices and segment lists in LDS (32 KiB each)
constexpr int kCsMaxBlocks = 2048;                // workgroups of cs_block_kernel (two of them fit a CU)
constexpr int kCsMaxQ = 1 << 20;
constexpr int kCsMaxCoord = 1 << 24;
constexpr size_t kCsMaxLoops = (size_t)1 << 24;
constexpr size_t kCsMaxVerts = (size_t)1 << 27;

// A candidate of an arg-max: the larger n wins, on equal n the lower m.  m = kCsNone: no candidate (n is 0 then: it loses to every
// vertex).
constexpr int kCsNone = 0x7fffffff;
struct CsBest {
  u128 n;
  int m;
};

__device__ __forceinline__ CsBest cs_better(CsBest a, CsBest b) { return (b.n > a.n || (b.n == a.n && b.m < a.m)) ? b : a; }

// every lane receives the best of the wave
__device__ __forceinline__ CsBest cs_wave_best(CsBest v) {
  if (__any((cs_u64)(v.n >> 64) != 0ull)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const cs_u64 hi = __shfl_xor((cs_u64)(v.n >> 64), o), lo = __shfl_xor((cs_u64)v.n, o);
      const int m = __shfl_xor(v.m, o);
      v = cs_better(v, CsBest{((u128)hi << 64) | lo, m});
    }
  } else {      // no lane's N reaches 2^64 (coordinates of an image): the same comparison with three shuffles a step for five --
                // 134 against 153 us of kernels for the 600x1000 set of tools/contours_simplify_bench.py
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const cs_u64 lo = __shfl_xor((cs_u64)v.n, o);
      const int m = __shfl_xor(v.m, o);
      v = cs_better(v, CsBest{(u128)lo, m});
    }
  }
  return v;
}

__device__ __forceinline__ u128 cs_sq(long long x, long long y) { return (u128)(cs_u64)(x * x + y * y); }   // |x|, |y| <= 2^25

// One segment a -> b: the numerator of the squared distance of p, over the segment's common denominator (the four cases of n14).
struct CsSeg {
  int ax, ay, bx, by;
  long long abx, aby, len;                        // b - a and its square, below 2^52
  __device__ __forceinline__ CsSeg(int2 a, int2 b)
      : ax(a.x), ay(a.y), bx(b.x), by(b.y), abx((long long)b.x - a.x), aby((long long)b.y - a.y) {
    len = abx * abx + aby * aby;
  }
  __device__ __forceinline__ u128 num(int2 p) const {
    const long long apx = (long long)p.x - ax, apy = (long long)p.y - ay;
    if (len == 0) return cs_sq(apx, apy);
    const long long t = apx * abx + apy * aby;
    if (t <= 0) return cs_sq(apx, apy) * (u128)(cs_u64)len;
    if (t >= len) return cs_sq((long long)p.x - bx, (long long)p.y - by) * (u128)(cs_u64)len;
    const long long cr = abx * apy - aby * apx;   // below 2^52 in size
    const cs_u64 c = (cs_u64)(cr < 0 ? -cr : cr);
    return (u128)c * c;
  }
  // 256 N > q^2 D: both sides below 2^110
  __device__ __forceinline__ bool over(u128 n, int q) const {
    return (n << 8) > (u128)((cs_u64)q * (cs_u64)q) * (u128)(cs_u64)(len ? len : 1);
  }
};

// The two chains of a loop once both arg-maxes are known: which of them keep their vertex.  Neither over the tolerance: the third
// anchor, the larger of the two whatever q is (both chains have the denominator |v_B - v_0|^2), the lower index -- chain 0 -- on ties.
__device__ __forceinline__ void cs_chains(const CsSeg& seg, CsBest c0, CsBest c1, int q, bool* keep0, bool* keep1) {
  *keep0 = c0.m != kCsNone && seg.over(c0.n, q);
  *keep1 = c1.m != kCsNone && seg.over(c1.n, q);
  if (!*keep0 && !*keep1) {
    if (cs_better(c0, c1).m == c0.m) *keep0 = true; else *keep1 = true;   // (one of them has a vertex: k >= 4)
  }
}

// grid ceil(n_loops / 4), block 256: one wave per loop.  keep [V] is zero before.
__global__ __launch_bounds__(kCsThreads) void cs_wave_kernel(const long long* __restrict__ vert_ptr, const int2* __restrict__ xy,
                                                             int n_loops, int q, unsigned char* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * kCsWaves + (threadIdx.x >> 6);
  if (l >= n_loops) return;
  const long long base = vert_ptr[l];
  const long long len = vert_ptr[l + 1] - base;
  if (len <= 0 || len > kCsWaveVerts) return;
  const int k = (int)len;
  const int2 p = lane < k ? xy[base + lane] : make_int2(0, 0);
  if (k <= 3) {
    if (lane < k) keep[base + lane] = 1;
    return;
  }
  // the best vertex strictly between i and j of the segment v_i -> v_(j mod k)
  auto best_of = [&](int i, int j, CsSeg* seg) {
    const int jj = j == k ? 0 : j;
    *seg = CsSeg(make_int2(__shfl(p.x, i), __shfl(p.y, i)), make_int2(__shfl(p.x, jj), __shfl(p.y, jj)));
    const bool in = lane > i && lane < j;
    return cs_wave_best(CsBest{in ? seg->num(p) : (u128)0, in ? lane : kCsNone});
  };
  const int2 v0 = make_int2(__shfl(p.x, 0), __shfl(p.y, 0));
  const bool far = lane >= 1 && lane < k;
  const int B = cs_wave_best(CsBest{far ? cs_sq((long long)p.x - v0.x, (long long)p.y - v0.y) : (u128)0, far ? lane : kCsNone}).m;
  cs_u64 kept = 1ull | (1ull << B), closed = 0ull;           // closed: the segment that begins at this kept vertex is finished
  CsSeg seg(v0, v0), seg1(v0, v0);
  const CsBest c0 = best_of(0, B, &seg), c1 = best_of(B, k, &seg1);
  bool keep0, keep1;
  cs_chains(seg, c0, c1, q, &keep0, &keep1);
  if (keep0) kept |= 1ull << c0.m; else closed |= 1ull;
  if (keep1) kept |= 1ull << c1.m; else closed |= 1ull << B;
  for (int turn = 0; turn < 2 * kCsWaveVerts; ++turn) {      // every turn keeps a vertex or closes a segment
    const cs_u64 open = kept & ~closed;
    if (!open) break;
    const int i = __builtin_ctzll(open);
    const cs_u64 rest = i == 63 ? 0ull : kept >> (i + 1);
    const int j = rest ? i + 1 + __builtin_ctzll(rest) : k;
    if (j - i < 2) { closed |= 1ull << i; continue; }
    const CsBest b = best_of(i, j, &seg);
    if (seg.over(b.n, q)) kept |= 1ull << b.m; else closed |= 1ull << i;
  }
  if (lane < k) keep[base + lane] = (unsigned char)((kept >> lane) & 1ull);
}

// The vertices of one loop as cs_block_kernel reads them.
template <bool kLds>
struct CsLoop {
  const int2* g;      // the loop's vertices in global memory
  const int2* s;      // and in LDS, where they are staged
  int k;
  __device__ __forceinline__ int2 at(int m) const { return kLds ? s[m] : g[m]; }
  __device__ __forceinline__ int2 end(int j) const { return at(j == k ? 0 : j); }
};

// The best of the workgroup: every thread brings its own, every thread receives the result.  s_best [kCsBlockWaves]; two barriers.
__device__ __forceinline__ CsBest cs_block_best(CsBest mine, CsBest* s_best) {
  const CsBest w = cs_wave_best(mine);
  __syncthreads();                                           // s_best may still be read from the call before
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = w;
  __syncthreads();
  CsBest all = s_best[0];
#pragma unroll
  for (int k = 1; k < kCsBlockWaves; ++k) all = cs_better(all, s_best[k]);
  return all;
}

// The halves (i, m) and (m, j) of a split segment that have an inner vertex: how many, and into a list
__device__ __forceinline__ int cs_halves(int i, int m, int j) { return (m - i >= 2) + (j - m >= 2); }
__device__ __forceinline__ void cs_put_halves(int i, int m, int j, int2* out) {
  if (m - i >= 2) *out++ = make_int2(i, m);
  if (j - m >= 2) *out = make_int2(m, j);
}

// One loop by the whole workgroup.  keep: the loop's flags; list: its two segment lists of k / 2 entries each (in LDS where the
// vertices are).
template <bool kLds>
__device__ __forceinline__ void cs_block_loop(const CsLoop<kLds> P, int q, unsigned char* __restrict__ keep, int2* __restrict__ list,
                                              CsBest* s_best, int* s_count) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = P.k, cap = k / 2;
  const int2 v0 = P.at(0);
  CsBest mine{0, kCsNone};
  for (int m = 1 + tid; m < k; m += kCsBlockThreads) {
    const int2 p = P.at(m);
    mine = cs_better(mine, CsBest{cs_sq((long long)p.x - v0.x, (long long)p.y - v0.y), m});
  }
  const int B = cs_block_best(mine, s_best).m;
  const int2 vB = P.at(B);
  const CsSeg seg0(v0, vB), seg1(vB, v0);
  mine = CsBest{0, kCsNone};
  for (int m = 1 + tid; m < B; m += kCsBlockThreads) mine = cs_better(mine, CsBest{seg0.num(P.at(m)), m});
  const CsBest c0 = cs_block_best(mine, s_best);
  mine = CsBest{0, kCsNone};
  for (int m = B + 1 + tid; m < k; m += kCsBlockThreads) mine = cs_better(mine, CsBest{seg1.num(P.at(m)), m});
  const CsBest c1 = cs_block_best(mine, s_best);
  bool keep0, keep1;
  cs_chains(seg0, c0, c1, q, &keep0, &keep1);
  // the first list, by one thread; every thread knows its length
  const int n0 = keep0 ? cs_halves(0, c0.m, B) : 0, n1 = keep1 ? cs_halves(B, c1.m, k) : 0;
  int count = n0 + n1;                                       // at most 4, and cap is at least 32
  if (tid == 0) {
    keep[0] = 1;
    keep[B] = 1;
    if (keep0) { keep[c0.m] = 1; cs_put_halves(0, c0.m, B, list); }
    if (keep1) { keep[c1.m] = 1; cs_put_halves(B, c1.m, k, list + n0); }
    s_count[0] = 0;                                          // the counter of round 0's appends
  }
  __syncthreads();
  // Round r reads list r & 1, appends to the other and counts in s_count[r % 3]; it zeroes the counter of round r + 1, which was
  // last read behind the barrier of round r - 2: one barrier a round.
  for (int r = 0; count > 0; ++r) {
    const int2* cur = list + (size_t)(r & 1) * cap;
    int2* next = list + (size_t)(~r & 1) * cap;
    int* counter = s_count + r % 3;
    if (tid == 0) s_count[(r + 1) % 3] = 0;
    for (int s = wave; s < count; s += kCsBlockWaves) {
      const int2 ij = cur[s];
      const CsSeg seg(P.at(ij.x), P.end(ij.y));
      mine = CsBest{0, kCsNone};
      for (int m = ij.x + 1 + lane; m < ij.y; m += 64) mine = cs_better(mine, CsBest{seg.num(P.at(m)), m});
      const CsBest b = cs_wave_best(mine);
      if (lane == 0 && b.m != kCsNone && seg.over(b.n, q)) {
        keep[b.m] = 1;
        const int n = cs_halves(ij.x, b.m, ij.y);
        const int slot = n ? atomicAdd(counter, n) : 0;
        if (slot + n <= cap) cs_put_halves(ij.x, b.m, ij.y, next + slot);   // (always: open segments are disjoint and span 2 or more)
      }
    }
    __syncthreads();
    count = min(*counter, cap);
  }
}

// grid min(n_loops, kCsMaxBlocks), block 512.  keep [V] is zero before; lists [V]: the loops that are not staged in LDS have their
// two lists there, k / 2 entries each from vert_ptr[l] on.
__global__ __launch_bounds__(kCsBlockThreads) void cs_block_kernel(const long long* __restrict__ vert_ptr, const int2* __restrict__ xy,
                                                                   int n_loops, int q, unsigned char* __restrict__ keep,
                                                                   int2* __restrict__ lists) {
  __shared__ int2 s_xy[kCsLdsVerts];
  __shared__ int2 s_list[kCsLdsVerts];
  __shared__ CsBest s_best[kCsBlockWaves];
  __shared__ int s_count[3];
  for (int l = blockIdx.x; l < n_loops; l += gridDim.x) {
    const long long base = vert_ptr[l];
    const long long len = vert_ptr[l + 1] - base;
    if (len <= kCsWaveVerts) continue;                       // (the whole workgroup alike)
    const int k = (int)len;
    if (k <= kCsLdsVerts) {
      for (int m = threadIdx.x; m < k; m += kCsBlockThreads) s_xy[m] = xy[base + m];
      __syncthreads();
      cs_block_loop(CsLoop<true>{xy + base, s_xy, k}, q, keep + base, s_list, s_best, s_count);
    } else {
      cs_block_loop(CsLoop<false>{xy + base, s_xy, k}, q, keep + base, lists + base, s_best, s_count);
    }
    __syncthreads();                                         // s_xy, the lists and the counters are written again
  }
}

// grid ceil(max(V, n_loops + 1) / 256), block 256.
__global__ __launch_bounds__(kCsThreads) void cs_write_kernel(const long long* __restrict__ vert_ptr, const int2* __restrict__ xy,
                                                              int n_loops, const unsigned char* __restrict__ keep, Scanned pre,
                                                              long long* __restrict__ out_vert_ptr, int2* __restrict__ out_xy,
                                                              long long* __restrict__ out_index) {
  const long long g = (long long)blockIdx.x * kCsThreads + threadIdx.x;
  if (g <= n_loops) out_vert_ptr[g] = pre.upto((int)vert_ptr[g]);
  if (g < pre.count && keep[g]) {
    const int slot = pre.at((int)g);
    out_xy[slot] = xy[g];
    out_index[slot] = g;
  }
}

// What a call needs on the device beside its input and its result.
struct CsWork {
  unsigned char* keep;   // [V]
  int* in_tile;          // [V]
  int* tile;             // [tiles + 1]: tile[tiles] = V' after the launches
  int2* lists;           // [V]
};

// The whole rule on device pointers, asynchronous on `s`: vert_ptr [L + 1] and xy [V][2] checked by the caller (1 <= L <= 2^24,
// 1 <= V <= 2^27, the pointers run from 0 to V without decreasing, |coordinate| <= 2^24, 0 <= q <= 2^20) -> out_vert_ptr [L + 1],
// out_xy [V'][2], out_index [V'] and w.tile[scan_tiles(V)] = V'.  The same launches whatever the data.
hipError_t cs_launch(hipStream_t s, const long long* vert_ptr, const int* xy, int n_loops, int n_verts, int q, const CsWork& w,
                     long long* out_vert_ptr, int* out_xy, long long* out_index) {
  const int2* p = (const int2*)xy;
  const dim3 block(kCsThreads);
  const hipError_t e = hipMemsetAsync(w.keep, 0, (size_t)n_verts, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cs_wave_kernel, dim3((n_loops + kCsWaves - 1) / kCsWaves), block, 0, s, vert_ptr, p, n_loops, q, w.keep);
  hipLaunchKernelGGL(cs_block_kernel, dim3(n_loops < kCsMaxBlocks ? n_loops : kCsMaxBlocks), dim3(kCsBlockThreads), 0, s, vert_ptr, p, n_loops, q,
                     w.keep, w.lists);
  const Scanned pre = scan_launch(s, w.keep, n_verts, w.in_tile, w.tile);
  const long long items = n_verts > n_loops + 1 ? n_verts : n_loops + 1;
  hipLaunchKernelGGL(cs_write_kernel, dim3((unsigned)((items + kCsThreads - 1) / kCsThreads)), block, 0, s, vert_ptr, p, n_loops,
                     w.keep, pre, out_vert_ptr, (int2*)out_xy, out_index);
  return hipGetLastError();
}

namespace {

// mnc_contours_simplify_timing: a HIP event pair around the launches of the next calls, the last call's time kept
CallTimer g_cs_timer;

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_contours_simplify(const long long* vert_ptr, const int* xy, size_t n_loops, size_t n_verts, int q, long long* out_vert_ptr,
                          int* out_xy, long long* out_index, size_t* out_verts, int device_id) {
  const char* who = "mnc_contours_simplify";
  MNC_REQUIRE(q >= 0 && q <= kCsMaxQ, "%s: q=%d not in [0, %d]", who, q, kCsMaxQ);
  MNC_REQUIRE(n_loops <= kCsMaxLoops, "%s: n_loops=%zu above %zu", who, n_loops, kCsMaxLoops);
  MNC_REQUIRE(n_verts <= kCsMaxVerts, "%s: n_verts=%zu above %zu", who, n_verts, kCsMaxVerts);
  MNC_REQUIRE(vert_ptr && out_vert_ptr && out_verts, "%s: null vert_ptr, out_vert_ptr or out_verts", who);
  MNC_REQUIRE(n_verts == 0 || (xy && out_xy && out_index), "%s: null xy, out_xy or out_index", who);
  MNC_REQUIRE(vert_ptr[0] == 0, "%s: vert_ptr[0]=%lld is not 0", who, vert_ptr[0]);
  for (size_t l = 0; l < n_loops; ++l)
    MNC_REQUIRE(vert_ptr[l + 1] >= vert_ptr[l], "%s: vert_ptr decreases at loop %zu (%lld after %lld)", who, l, vert_ptr[l + 1],
                vert_ptr[l]);
  MNC_REQUIRE(vert_ptr[n_loops] == (long long)n_verts, "%s: vert_ptr ends at %lld, not at the %zu vertices given", who,
              vert_ptr[n_loops], n_verts);
  for (size_t v = 0; v < 2 * n_verts; ++v)
    MNC_REQUIRE(xy[v] >= -kCsMaxCoord && xy[v] <= kCsMaxCoord, "%s: coordinate %d of vertex %zu outside [-%d, %d]", who, xy[v], v / 2,
                kCsMaxCoord, kCsMaxCoord);
  if (n_loops == 0 || n_verts == 0) {
    for (size_t l = 0; l <= n_loops; ++l) out_vert_ptr[l] = 0;
    *out_verts = 0;
    clear_error();
    return MNC_OK;
  }

  const int L = (int)n_loops, V = (int)n_verts, tiles = scan_tiles(V);
  long long *d_vert_ptr, *d_out_vert_ptr, *d_out_index; int *d_xy, *d_out_xy; CsWork w;
  auto layout = [&](WsLayout l) {
    d_vert_ptr = l.take<long long>(n_loops + 1);
    d_xy = l.take<int>(2 * n_verts);
    w.keep = l.take<unsigned char>(n_verts);
    w.in_tile = l.take<int>(n_verts);
    w.tile = l.take<int>((size_t)tiles + 1);
    w.lists = l.take<int2>(n_verts);
    d_out_vert_ptr = l.take<long long>(n_loops + 1);
    d_out_xy = l.take<int>(2 * n_verts);
    d_out_index = l.take<long long>(n_verts);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  hipStream_t s = hs.stream;
  MNC_HIP_TRY(hs.up(d_vert_ptr, vert_ptr, (n_loops + 1) * 8));
  MNC_HIP_TRY(hs.up(d_xy, xy, 2 * n_verts * sizeof(int)));
  TimedSpan span(g_cs_timer);
  span.begin(s);
  MNC_HIP_TRY(cs_launch(s, d_vert_ptr, d_xy, L, V, q, w, d_out_vert_ptr, d_out_xy, d_out_index));
  span.end(s);
  int kept = 0;
  MNC_HIP_TRY(hs.down(&kept, w.tile + tiles, sizeof(int)));
  MNC_HIP_TRY(hs.sync());
  MNC_HIP_TRY(hs.down(out_vert_ptr, d_out_vert_ptr, (n_loops + 1) * 8));
  MNC_HIP_TRY(hs.down(out_xy, d_out_xy, 2 * (size_t)kept * sizeof(int)));
  MNC_HIP_TRY(hs.down(out_index, d_out_index, (size_t)kept * 8));
  MNC_HIP_TRY(hs.sync());
  *out_verts = (size_t)kept;
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_contours_simplify_timing(int on, double* last_ms) { return g_cs_timer.set(on, last_ms); }
