// Outlines of packed instance masks as polygons for gfx950 (include/mnc_hip.h n13), on the PackedMasks layout of inst_masks.hip
// (n5), without unpacking a mask.  The helpers that work on values are mask_contour.h (host and device).
//
// A w x h instance has (w + 1) x (h + 1) lattice points, cut into words of 64 like its pixels; a boundary edge belongs to its tail
// point.  The point words of a set are numbered in raster order, instance after instance (at most 2^25 of them).
//   ct_count_kernel   one thread per point word: the edges that leave its points (ct_edges: four bit expressions of the pixel words
//                     above and below and their carries), counted; the total of the set as a 64-bit sum.
//   scan_launch       (scan.hip) the exclusive prefix of the counts: in tiles of 1024, then over the tiles.  An edge's id is the prefix at
//                     its word + the edges below it in the word (ct_edge_id): ids are in the order instance, tail y, tail x, direction.
//                     The total E is read back: it sizes the edge buffers and the number of rounds, ceil(log2(E)).
//   ct_succ_kernel    one thread per point word: succ[e] of its edges (ct_successor), their tail and direction, and at the
//                     successor whether it turns (= its tail is a vertex).  succ is a permutation: every slot is written once.
//   ct_min_kernel     one round of pointer jumping with a running minimum, from one pair of buffers into the other: after round k
//                     lead[e] is the smallest id among the 2^k edges from e on.  After the last round it is the smallest of the
//                     cycle: the edge that leaves the loop's smallest (y, x) point, the loop's first vertex.
//   ct_cut_kernel     every cycle cut in front of its leader: the list successor of an edge whose successor is a leader is none.
//   ct_rank_kernel    one round of Wyllie's list ranking with weight 1 on the vertices, buffers swapped as above: after the last
//                     round rank[e] is the number of vertices from e to the end of its list, so rank[leader] is the loop's vertex
//                     count and rank[leader] - rank[e] the slot of vertex e.
//   ct_heads_kernel   flag[e] = e is a leader, vcnt[e] = its loop's vertex count (0 for the others).  The scan of the flags numbers
//                     the loops, the scan of the counts gives vert_ptr: both in leader order, which is the order the rule demands.
//   ct_loop_ptr_kernel  the first loop of every instance: the prefix at its first edge.  L and V are read back: they size the result.
//   ct_write_kernel   one thread per edge: its vertex into its slot, vert_ptr by the leader, and for a vertical edge +x resp. -x
//                     added to area[loop] (the sum of x dy round the loop: the shoelace area without the halving).
// Every round is its own launch; no workgroup waits for another; every loop in a kernel is bounded by what the launch knows (the
// 64 points of a word, log2 of the instance count, the tiles of a scan).  Integer atomics only (64-bit adds), every other output slot
// is written once with an ordinary store: the same input gives the same bytes on every run.
// Bound: 12 + 2 ceil(log2(E)) small dependent kernel launches, two memsets and three read-backs; latency, not bandwidth
// (tools/mask_contours_bench.py, profiles/mask_contours_bench.txt).
#include <vector>

#include "mask_contour.h"
#include "mask_set.h"
#include "scan.h"

namespace mnc {

constexpr int kCtThreads = 256;
constexpr int kCtMaxN = 2048;                   // instances of one call
constexpr long long kCtMaxWords = 1ll << 25;    // point words of one call
constexpr long long kCtMaxEdges = 1ll << 30;    // edges of one call: ids, ranks and vertex slots are ints

// The point rows of one instance: what the host adds to the set's own table (MaskSet::info).
struct CtInst {
  int vh, vs;          // point rows (h + 1) and point words per row (0 without rows)
  int word0;           // its first word among the point words of the set
};

// One instance as a thread sees it; the G of mask_contour.h:ct_successor.
struct CtGrid {
  int w, h, rs, vs, word0;
  const u64* rows;
  Scanned ids;
  // pixel word j of pixel row y and the pixel before it; 0 outside
  __device__ __forceinline__ void row(int y, int j, u64* v, u64* carry) const {
    *v = 0ull; *carry = 0ull;
    if (y < 0 || y >= h) return;
    const u64* r = rows + (long long)y * rs;
    *v = mask_word(r, j, rs, w);
    *carry = mask_word(r, j - 1, rs, w) >> 63;
  }
  __device__ __forceinline__ CtEdges edges(int y, int j) const {
    u64 up, upc, dn, dnc;
    row(y - 1, j, &up, &upc);
    row(y, j, &dn, &dnc);
    return ct_edges(up, upc, dn, dnc);
  }
  __device__ __forceinline__ int base(int y, int j) const { return ids.at(word0 + y * vs + j); }
};

struct CtAt {
  int i, y, j;
};

// The instance, point row and word of point word g: the last instance that begins at or before g (one without words begins where
// the next does).
__device__ __forceinline__ CtAt ct_decode(const CtInst* __restrict__ insts, int n, int g) {
  const int lo = mask_owner<&CtInst::word0>(insts, n, g);
  const int local = g - insts[lo].word0;
  return {lo, local / insts[lo].vs, local % insts[lo].vs};
}

__device__ __forceinline__ CtGrid ct_grid(const MaskSet& A, const CtInst* __restrict__ insts, int i, Scanned ids) {
  const mnc_mask_info s = A.info[i];
  const int w = s.x2 - s.x1 + 1;
  return {w, s.y2 - s.y1 + 1, mask_strips(w), insts[i].vs, insts[i].word0, A.bits + s.offset / 8, ids};
}

// grid ceil(words / 256), block 256.  cnt [words]; *total += the edges of the set, one atomic per wave.
__global__ __launch_bounds__(kCtThreads) void ct_count_kernel(MaskSet A, const CtInst* __restrict__ insts, int n, int words,
                                                              int* __restrict__ cnt, unsigned long long* __restrict__ total) {
  const int g = blockIdx.x * kCtThreads + threadIdx.x;
  int c = 0;
  if (g < words) {
    const CtAt at = ct_decode(insts, n, g);
    c = ct_count(ct_grid(A, insts, at.i, Scanned{}).edges(at.y, at.j));
    cnt[g] = c;
  }
  int sum = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, (unsigned long long)sum);
}

// What is known of every edge once its word has been visited.
struct CtEdgeInfo {
  int* succ;               // [E]
  int* x;                  // [E] the tail, image coordinates
  int* y;                  // [E]
  unsigned char* dir;      // [E]
  unsigned char* vertex;   // [E] 1: the edge before has another direction
};

// grid ceil(words / 256), block 256.  lead0[e] = e and next0[e] = succ[e]: the state before the first round of ct_min_kernel.
__global__ __launch_bounds__(kCtThreads) void ct_succ_kernel(MaskSet A, const CtInst* __restrict__ insts, int n, int words, Scanned ids,
                                                             int eight, int edges, CtEdgeInfo info, int* __restrict__ lead0,
                                                             int* __restrict__ next0) {
  const int g = blockIdx.x * kCtThreads + threadIdx.x;
  if (g >= words) return;
  const CtAt at = ct_decode(insts, n, g);
  const CtGrid m = ct_grid(A, insts, at.i, ids);
  const CtEdges own = m.edges(at.y, at.j);
  u64 points = ct_any(own);
  if (!points) return;
  const mnc_mask_info s = A.info[at.i];
  const int base = ids.at(g), X = s.x1 + at.j * 64, Y = s.y1 + at.y;
  int e = base;
  for (int turn = 0; turn < 64 && points; ++turn) {      // the points of the word that an edge leaves, lowest first
    const int b = __builtin_ctzll(points);
    points &= points - 1ull;
    for (int d = 0; d < 4; ++d) {
      if (!((own.d[d] >> b) & 1ull)) continue;
      int sd;
      int to = ct_successor(m, at.y, at.j, own, base, b, d, eight, &sd);
      // (cannot be: the ids of the heads come from the same words and the same scan)
      if (to < 0 || to >= edges) { to = e; sd = d; }
      info.succ[e] = to;
      info.x[e] = X + b;
      info.y[e] = Y;
      info.dir[e] = (unsigned char)d;
      info.vertex[to] = (unsigned char)(sd != d);
      lead0[e] = e;
      next0[e] = to;
      ++e;
    }
  }
}

// grid ceil(E / 256), block 256.
__global__ __launch_bounds__(kCtThreads) void ct_min_kernel(const int* __restrict__ lead_in, const int* __restrict__ next_in, int edges,
                                                            int* __restrict__ lead_out, int* __restrict__ next_out) {
  const int e = blockIdx.x * kCtThreads + threadIdx.x;
  if (e >= edges) return;
  const int t = next_in[e];
  lead_out[e] = min(lead_in[e], lead_in[t]);
  next_out[e] = next_in[t];
}

// grid ceil(E / 256), block 256.  The lists: next0[e] = -1 where the successor leads its loop; rank0[e] = the edge's own weight.
__global__ __launch_bounds__(kCtThreads) void ct_cut_kernel(CtEdgeInfo info, const int* __restrict__ lead, int edges,
                                                            int* __restrict__ rank0, int* __restrict__ next0) {
  const int e = blockIdx.x * kCtThreads + threadIdx.x;
  if (e >= edges) return;
  const int s = info.succ[e];
  next0[e] = lead[s] == s ? -1 : s;
  rank0[e] = info.vertex[e];
}

// grid ceil(E / 256), block 256.
__global__ __launch_bounds__(kCtThreads) void ct_rank_kernel(const int* __restrict__ rank_in, const int* __restrict__ next_in, int edges,
                                                             int* __restrict__ rank_out, int* __restrict__ next_out) {
  const int e = blockIdx.x * kCtThreads + threadIdx.x;
  if (e >= edges) return;
  const int t = next_in[e];
  rank_out[e] = rank_in[e] + (t >= 0 ? rank_in[t] : 0);
  next_out[e] = t >= 0 ? next_in[t] : -1;
}

// grid ceil(E / 256), block 256.
__global__ __launch_bounds__(kCtThreads) void ct_heads_kernel(const int* __restrict__ lead, const int* __restrict__ rank, int edges,
                                                              int* __restrict__ flag, int* __restrict__ vcnt) {
  const int e = blockIdx.x * kCtThreads + threadIdx.x;
  if (e >= edges) return;
  const bool head = lead[e] == e;
  flag[e] = head;
  vcnt[e] = head ? rank[e] : 0;
}

// grid ceil((n + 1) / 256), block 256.  loop_ptr [n + 1]: the loops before the first edge of instance i.
__global__ __launch_bounds__(kCtThreads) void ct_loop_ptr_kernel(const CtInst* __restrict__ insts, int n, int words, Scanned ids,
                                                                 Scanned number, long long* __restrict__ loop_ptr) {
  const int i = blockIdx.x * kCtThreads + threadIdx.x;
  if (i > n) return;
  const int w0 = i < n ? insts[i].word0 : words;
  loop_ptr[i] = number.upto(ids.upto(w0));
}

// grid ceil(E / 256), block 256.  area [L] is zero before.
__global__ __launch_bounds__(kCtThreads) void ct_write_kernel(CtEdgeInfo info, const int* __restrict__ lead, const int* __restrict__ rank,
                                                              int edges, Scanned number, Scanned vbase, int verts,
                                                              long long* __restrict__ vert_ptr, unsigned long long* __restrict__ area,
                                                              int* __restrict__ xy) {
  const int e = blockIdx.x * kCtThreads + threadIdx.x;
  if (e >= edges) return;
  const int head = lead[e], loop = number.at(head), first = vbase.at(head);
  if (e == head) vert_ptr[loop] = first;
  const int x = info.x[e], d = info.dir[e];
  if (info.vertex[e]) {
    const long long slot = (long long)first + (rank[head] - rank[e]);
    if (slot >= 0 && slot < verts) {                     // (always: e is a vertex of its leader's list)
      xy[2 * slot] = x;
      xy[2 * slot + 1] = info.y[e];
    }
  }
  if (d == kCtSouth) atomicAdd(area + loop, (unsigned long long)(long long)x);
  if (d == kCtNorth) atomicAdd(area + loop, (unsigned long long)(long long)-x);
}

namespace {

// The second and third workspace of a call, per device: sized once the edge total resp. the loop and vertex totals are read back
// (the HostScope workspace holds what is known before the first launch and cannot grow without losing it).  Guarded by the
// HostScope's mutex, which the call holds to its end.
DevArena g_ct_edges[16], g_ct_out[16];

// mnc_mask_contours_timing: a HIP event pair around the launches of the next calls, the last call's time kept
CallTimer g_ct_timer;

inline int ct_blocks(long long items) { return (int)((items + kCtThreads - 1) / kCtThreads); }

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_contours(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
                      long long* loop_ptr, long long* vert_ptr, long long* area, int* xy, size_t loop_cap, size_t vert_cap,
                      size_t* n_loops, size_t* n_verts, int device_id) {
  const char* who = "mnc_mask_contours";
  MNC_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity=%d is not 4 or 8", who, connectivity);
  MNC_REQUIRE(n >= 0 && n <= kCtMaxN, "%s: n=%d not in [0, %d]", who, n, kCtMaxN);
  HostMaskSet set;
  int rc = set.check(who, "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
  if (rc) return rc;
  std::vector<CtInst> insts((size_t)n + 1);
  long long at = 0;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& s = set.info[i];
    const int w = s.x2 - s.x1 + 1, h = s.y2 - s.y1 + 1;
    const bool rows = w >= 1 && h >= 1;
    insts[i] = {rows ? h + 1 : 0, rows ? mask_strips(w + 1) : 0, (int)at};
    at += (long long)insts[i].vh * insts[i].vs;
    MNC_REQUIRE(at <= kCtMaxWords, "%s: more than %lld words of rows in the set (at masks[%d])", who, kCtMaxWords, i);
  }
  insts[n] = {0, 0, (int)at};
  const int words = (int)at;
  MNC_REQUIRE(loop_ptr && n_loops && n_verts, "%s: null output pointer", who);
  MNC_REQUIRE(!xy || (vert_ptr && area), "%s: null vert_ptr or area", who);
  for (int i = 0; i <= n; ++i) loop_ptr[i] = 0;
  *n_loops = 0;
  *n_verts = 0;
  if (words == 0) { clear_error(); return MNC_OK; }

  const int eight = connectivity == 8;
  CtInst* d_insts; int *d_cnt, *d_tile; unsigned long long* d_total; long long* d_loop_ptr;
  auto layout = [&](WsLayout l) {
    set.take(l);
    d_insts = l.take<CtInst>((size_t)n + 1);
    d_cnt = l.take<int>(words);
    d_tile = l.take<int>((size_t)scan_tiles(words) + 1);
    d_total = l.take<unsigned long long>(1);
    d_loop_ptr = l.take<long long>((size_t)n + 1);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  hipStream_t s = hs.stream;
  TimedSpan span(g_ct_timer);
  span.begin(s);
  MNC_HIP_TRY(set.upload(hs));
  MNC_HIP_TRY(hs.up(d_insts, insts.data(), insts.size() * sizeof(CtInst)));
  MNC_HIP_TRY(hipMemsetAsync(d_total, 0, 8, s));
  const MaskSet A = set.view();
  hipLaunchKernelGGL(ct_count_kernel, dim3(ct_blocks(words)), dim3(kCtThreads), 0, s, A, d_insts, n, words, d_cnt, d_total);
  const Scanned ids = scan_launch(s, d_cnt, words, d_tile);
  MNC_HIP_TRY(hipGetLastError());
  unsigned long long total = 0;
  MNC_HIP_TRY(hs.down(&total, d_total, 8));
  MNC_HIP_TRY(hs.sync());
  MNC_REQUIRE(total <= (unsigned long long)kCtMaxEdges, "%s: %llu boundary edges in the set (limit 2^30)", who, total);
  if (total == 0) {                                      // every mask is empty: loop_ptr stays 0
    span.end(s);
    MNC_HIP_TRY(hs.sync());
    span.keep();
    clear_error();
    return MNC_OK;
  }
  const int E = (int)total;
  int rounds = 0;
  while ((1ll << rounds) < E) ++rounds;                  // ceil(log2(E)): 2^rounds edges from any edge on go round its cycle

  CtEdgeInfo info;
  int *d_lead[2], *d_next[2], *d_rank[2], *d_flag, *d_vcnt, *d_tile2, *d_tile3;
  auto edge_layout = [&](WsLayout l) {
    info.succ = l.take<int>(E);
    info.x = l.take<int>(E);
    info.y = l.take<int>(E);
    info.dir = l.take<unsigned char>(E);
    info.vertex = l.take<unsigned char>(E);
    for (int k = 0; k < 2; ++k) {
      d_lead[k] = l.take<int>(E);
      d_next[k] = l.take<int>(E);
      d_rank[k] = l.take<int>(E);
    }
    d_flag = l.take<int>(E);
    d_vcnt = l.take<int>(E);
    d_tile2 = l.take<int>((size_t)scan_tiles(E) + 1);
    d_tile3 = l.take<int>((size_t)scan_tiles(E) + 1);
    return l.bytes();
  };
  size_t need = edge_layout(WsLayout());
  rc = arena_ensure(&g_ct_edges[device_id], need, (need >> 1) + 4096, "contour edge buffers", s);
  if (rc) return rc;
  edge_layout(WsLayout(g_ct_edges[device_id].p));
  const dim3 per_edge(ct_blocks(E)), block(kCtThreads);
  hipLaunchKernelGGL(ct_succ_kernel, dim3(ct_blocks(words)), block, 0, s, A, d_insts, n, words, ids, eight, E, info, d_lead[0], d_next[0]);
  for (int k = 0; k < rounds; ++k)
    hipLaunchKernelGGL(ct_min_kernel, per_edge, block, 0, s, d_lead[k & 1], d_next[k & 1], E, d_lead[~k & 1], d_next[~k & 1]);
  const int* lead = d_lead[rounds & 1];
  hipLaunchKernelGGL(ct_cut_kernel, per_edge, block, 0, s, info, lead, E, d_rank[0], d_next[0]);
  for (int k = 0; k < rounds; ++k)
    hipLaunchKernelGGL(ct_rank_kernel, per_edge, block, 0, s, d_rank[k & 1], d_next[k & 1], E, d_rank[~k & 1], d_next[~k & 1]);
  const int* rank = d_rank[rounds & 1];
  hipLaunchKernelGGL(ct_heads_kernel, per_edge, block, 0, s, lead, rank, E, d_flag, d_vcnt);
  const Scanned number = scan_launch(s, d_flag, E, d_tile2), vbase = scan_launch(s, d_vcnt, E, d_tile3);
  hipLaunchKernelGGL(ct_loop_ptr_kernel, dim3(ct_blocks(n + 1)), block, 0, s, d_insts, n, words, ids, number, d_loop_ptr);
  MNC_HIP_TRY(hipGetLastError());
  int V = 0;
  MNC_HIP_TRY(hs.down(loop_ptr, d_loop_ptr, ((size_t)n + 1) * 8));
  MNC_HIP_TRY(hs.down(&V, d_tile3 + vbase.tiles, sizeof(int)));
  MNC_HIP_TRY(hs.sync());
  const size_t L = (size_t)loop_ptr[n];
  *n_loops = L;
  *n_verts = (size_t)V;
  if (!xy) {
    span.end(s);
    MNC_HIP_TRY(hs.sync());
    span.keep();
    clear_error();
    return MNC_OK;
  }
  MNC_REQUIRE(loop_cap >= L && vert_cap >= (size_t)V, "%s: loop_cap %zu or vert_cap %zu is below the %zu loops and %zu vertices of the masks",
              who, loop_cap, vert_cap, L, (size_t)V);

  long long* d_vert_ptr; unsigned long long* d_area; int* d_xy;
  auto out_layout = [&](WsLayout l) {
    d_vert_ptr = l.take<long long>(L);
    d_area = l.take<unsigned long long>(L);
    d_xy = l.take<int>(2 * (size_t)V);
    return l.bytes();
  };
  need = out_layout(WsLayout());
  rc = arena_ensure(&g_ct_out[device_id], need, (need >> 1) + 4096, "contour result buffers", s);
  if (rc) return rc;
  out_layout(WsLayout(g_ct_out[device_id].p));
  MNC_HIP_TRY(hipMemsetAsync(d_area, 0, L * 8, s));
  hipLaunchKernelGGL(ct_write_kernel, per_edge, block, 0, s, info, lead, rank, E, number, vbase, V, d_vert_ptr, d_area, d_xy);
  span.end(s);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(vert_ptr, d_vert_ptr, L * 8));
  MNC_HIP_TRY(hs.down(area, d_area, L * 8));
  MNC_HIP_TRY(hs.down(xy, d_xy, 2 * (size_t)V * sizeof(int)));
  MNC_HIP_TRY(hs.sync());
  vert_ptr[L] = V;
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_contours_timing(int on, double* last_ms) { return g_ct_timer.set(on, last_ms); }
