// The set algebra of packed instance masks (include/mnc_hip.h n17), for gfx950, on the PackedMasks layout of inst_masks.hip (n5),
// without unpacking a mask: and, or, xor, minus, copy and complement of two sets instance by instance (mnc_mask_combine), the union
// or intersection of groups of instances (mnc_mask_merge), and the layering of a set into disjoint instances (mnc_mask_layer).  The
// statements of the rules are mnc_amd/algebra.py:combine_numpy, merge_numpy and layer_numpy; this file computes the same tables
// and words bit for bit.  All arithmetic is integer.
//
// The three entries are one expression.  Output instance o has a LOOSE FRAME -- a box that follows from the operands' bounds and
// the window alone, outside of which its result cannot have a pixel -- one optional operand `a` of set A, and a list of operands
// of set B (idx[lo .. hi - 1]):
//     q = the OR of the list's instances (the AND with `all`),   v = a op q,   cut to the frame.
//   combine   a = instance i of A, the list is instance i (or the only one) of B, op as given; copy and not have no list
//   merge     no a, the list is the group's members, op = or, `all` for the intersecting kind (A is B)
//   layer     a = instance i, the list is the instances before i in the order whose bounds meet i's, op = minus (A is B)
// al_word forms the 64 result bits of a frame row from any column on: every operand row is read at its own signed bit position
// through mask_word_at (funnel shift of two neighbouring words, padding bits masked, 0 outside the row), a row outside an
// operand's bounds reads 0, and the frame -- which already is intersected with the window -- is applied as a word mask.
//
//   al_extent_kernel   one lane per word of the loose frame: al_word, then the word's row and its lowest and highest set column
//                      (ctz / clz), reduced over the wave by shuffles and joined by integer atomicMin / atomicMax into four
//                      extents per instance, relative to the frame.
//   al_size_kernel     one lane per instance: the tight bounds from the extents ((0, 0, -1, -1) when no word was non-zero) and
//                      the words of its rows; scan_launch (scan.h) turns the counts into the offsets.
//   al_fill_kernel     one lane per word of the TIGHT frame (the grid is sized for the loose one; lanes past the tight words
//                      leave): al_word again at the tight position, stored once; the popcounts are summed over the wave and
//                      added to the instance's area by one integer atomic.
// Five launches whatever the data, nothing read back in between; the tight bounds and the areas come back first, the host derives
// the offsets from the bounds exactly as the scan did, and copies exactly the bytes of the result.  The only atomics are integer
// min, max and add: the same input gives the same bytes on every run.
//
// Bound: latency.  100 instances of an image are a few hundred KB of words that sit in L2; a lane reads at most two words per
// operand and row.  A merge reads every member per output word, a layer every listed neighbour.  Measured at 100 instances of a
// 600 x 1000 image, call with its copies / kernels alone: a | b 0.24 ms / 27 us, merge(by="class") 0.24 ms / 71 us (a class's frame
// is nearly the image and every word reads 25 members), layered() 0.16 ms / 26 us (profiles/mask_algebra_bench.txt).  20 VGPRs, no
// LDS and no scratch in any kernel.
#include <algorithm>
#include <climits>
#include <vector>

#include "mask_set.h"
#include "scan.h"

namespace mnc {

constexpr int kAlThreads = 256;
constexpr int kAlMaxN = 2048;                  // instances of a set and of a result (mnc_mask_boundary's limit)
constexpr int kAlMaxCoord = 1 << 24;
constexpr long long kAlMaxPixels = 1ll << 27;  // pixels of the loose frames of one call
constexpr long long kAlMaxMembers = 1ll << 20;

enum AlOp { kAlAnd = 0, kAlOr = 1, kAlXor = 2, kAlMinus = 3, kAlCopy = 4, kAlNot = 5 };

// One output instance: the loose frame (fw or fh 0: no pixel, skipped by every kernel), the operand of A (-1: none) and the list.
struct AlJob {
  int fx, fy, fw, fh;
  int a, lo, hi, pad_;
};

// Extents relative to the frame (al_extent_kernel; maxx < 0: no pixel), then the tight bounds in image coordinates (al_size_kernel).
struct AlBox {
  int x1, y1, x2, y2;
};

// The 64 bits of instance i from image column x on, in image row y: 0 outside its bounds.
__device__ __forceinline__ u64 al_read(const mnc_mask_info* __restrict__ info, const u64* __restrict__ bits, int i, int x, int y) {
  const mnc_mask_info& m = info[i];
  const int x1 = m.x1, y1 = m.y1, w = m.x2 - x1 + 1;
  if (w < 1 || y < y1 || y > m.y2) return 0ull;
  const int strips = mask_strips(w);
  return mask_word_at(bits + m.offset / 8 + (long long)(y - y1) * strips, x - x1, strips, w);
}

// The 64 result bits of job j from image column x >= j.fx on, in image row y of the frame.  Both passes call it.
__device__ __forceinline__ u64 al_word(const AlJob& j, const MaskSet& A, const MaskSet& B, const int* __restrict__ idx, int op, int all,
                                       int x, int y) {
  const u64 p = j.a >= 0 ? al_read(A.info, A.bits, j.a, x, y) : 0ull;
  u64 q = all ? ~0ull : 0ull;
  for (int k = j.lo; k < j.hi; ++k) {
    const u64 r = al_read(B.info, B.bits, idx[k], x, y);
    q = all ? q & r : q | r;
  }
  u64 v = op == kAlAnd ? p & q : op == kAlOr ? p | q : op == kAlXor ? p ^ q : op == kAlMinus ? p & ~q : op == kAlCopy ? p : ~p;
  const int valid = j.fx + j.fw - x;                       // columns of the frame from x on
  if (valid < 64) v &= valid > 0 ? (1ull << valid) - 1ull : 0ull;
  return v;
}

// grid (ceil(most loose-frame words / 256), jobs), block 256: a lane per word of the loose frame.
__global__ __launch_bounds__(kAlThreads) void al_extent_kernel(const AlJob* __restrict__ jobs, MaskSet A, MaskSet B,
                                                               const int* __restrict__ idx, int op, int all, AlBox* __restrict__ ext) {
  const int o = blockIdx.y;
  const AlJob j = jobs[o];
  if (j.fw < 1 || j.fh < 1) return;
  const int strips = mask_strips(j.fw);
  const long long t = (long long)blockIdx.x * kAlThreads + threadIdx.x;
  int minx = INT_MAX, miny = INT_MAX, maxx = -1, maxy = -1;
  if (t < (long long)j.fh * strips) {
    const int y = (int)(t / strips), c = (int)(t - (long long)y * strips);
    const u64 v = al_word(j, A, B, idx, op, all, j.fx + c * 64, j.fy + y);
    if (v) {
      minx = c * 64 + (__ffsll((long long)v) - 1);
      maxx = c * 64 + 63 - __clzll((long long)v);
      miny = maxy = y;
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    minx = min(minx, __shfl_xor(minx, s));
    miny = min(miny, __shfl_xor(miny, s));
    maxx = max(maxx, __shfl_xor(maxx, s));
    maxy = max(maxy, __shfl_xor(maxy, s));
  }
  if ((threadIdx.x & 63) == 0 && maxx >= 0) {
    atomicMin(&ext[o].x1, minx);
    atomicMin(&ext[o].y1, miny);
    atomicMax(&ext[o].x2, maxx);
    atomicMax(&ext[o].y2, maxy);
  }
}

// grid ceil(jobs / 256), block 256: the extents in place into the tight bounds, and the words of their rows.
__global__ __launch_bounds__(kAlThreads) void al_size_kernel(const AlJob* __restrict__ jobs, int n, AlBox* __restrict__ box,
                                                             int* __restrict__ words) {
  const int o = blockIdx.x * kAlThreads + threadIdx.x;
  if (o >= n) return;
  const AlJob j = jobs[o];
  const AlBox e = box[o];
  AlBox b = {0, 0, -1, -1};
  int count = 0;
  if (j.fw >= 1 && j.fh >= 1 && e.x2 >= 0) {
    b.x1 = j.fx + e.x1; b.y1 = j.fy + e.y1; b.x2 = j.fx + e.x2; b.y2 = j.fy + e.y2;
    count = (e.y2 - e.y1 + 1) * mask_strips(e.x2 - e.x1 + 1);      // (at most the 2^27 words of the call's loose frames)
  }
  box[o] = b;
  words[o] = count;
}

// grid (ceil(most loose-frame words / 256), jobs), block 256: a lane per word of the tight frame.
__global__ __launch_bounds__(kAlThreads) void al_fill_kernel(const AlJob* __restrict__ jobs, MaskSet A, MaskSet B,
                                                             const int* __restrict__ idx, int op, int all, const AlBox* __restrict__ box,
                                                             Scanned first, u64* __restrict__ out, u64* __restrict__ area) {
  const int o = blockIdx.y;
  const AlBox b = box[o];
  if (b.x2 < b.x1) return;
  const AlJob j = jobs[o];
  const int strips = mask_strips(b.x2 - b.x1 + 1);
  const long long t = (long long)blockIdx.x * kAlThreads + threadIdx.x;
  const bool live = t < (long long)(b.y2 - b.y1 + 1) * strips;
  if (__ballot(live) == 0ull) return;                      // (the whole wave)
  int set = 0;
  if (live) {
    const int y = (int)(t / strips), c = (int)(t - (long long)y * strips);
    const u64 v = al_word(j, A, B, idx, op, all, b.x1 + c * 64, b.y1 + y);
    out[(long long)first.at(o) + t] = v;
    set = __popcll(v);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) set += __shfl_xor(set, s);
  if ((threadIdx.x & 63) == 0 && set) atomicAdd(&area[o], (u64)set);
}

namespace {

inline bool al_rows(const mnc_mask_info& a) { return a.x2 >= a.x1 && a.y2 >= a.y1; }

// The jobs of one call and what its launches need.
struct AlCall {
  std::vector<AlJob> jobs;
  std::vector<int> idx;
  int op = kAlOr, all = 0;
  const int* window = nullptr;
  long long most_words = 0, bound_words = 0, pixels = 0;
  // The job of the next output instance: the frame (x1, y1, x2, y2) intersected with the window.
  void add(int x1, int y1, int x2, int y2, int a, long long lo, long long hi) {
    if (window) {
      x1 = std::max(x1, window[0]); y1 = std::max(y1, window[1]);
      x2 = std::min(x2, window[2]); y2 = std::min(y2, window[3]);
    }
    AlJob j = {0, 0, 0, 0, a, (int)lo, (int)hi, 0};
    if (x2 >= x1 && y2 >= y1) {
      j.fx = x1; j.fy = y1; j.fw = x2 - x1 + 1; j.fh = y2 - y1 + 1;
      const long long w = (long long)j.fh * mask_strips(j.fw);
      pixels += (long long)j.fw * j.fh;
      bound_words += w;
      most_words = std::max(most_words, w);
    }
    jobs.push_back(j);
  }
  void add_empty() { add(0, 0, -1, -1, -1, 0, 0); }
};

// What every entry refuses about a set, as mnc_mask_boundary does.
int al_check_set(const char* who, const char* name, HostMaskSet* set, const int* bounds, const long long* offsets, const void* bits,
                 size_t bytes, int n, const float* scores) {
  MNC_REQUIRE(n >= 0 && n <= kAlMaxN, "%s: %s has n=%d not in [0, %d]", who, name, n, kAlMaxN);
  std::vector<long long> areas((size_t)n, 0);
  return set->check(who, name, bounds, offsets, areas.data(), bits, bytes, n, nullptr, scores);
}

CallTimer g_al_timer;

// The rest of every entry once its jobs are made: the protocol of the sizes, the answers of the host, the launches, the copies.
int al_run(const char* who, const AlCall& c, HostMaskSet& a, HostMaskSet* B, int* out_bounds, long long* out_offsets,
           long long* out_areas, void* out_bits, size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id) {
  const int n = (int)c.jobs.size();
  MNC_REQUIRE(c.pixels <= kAlMaxPixels, "%s: %lld pixels of loose-frame rows in the call (limit %lld)", who, c.pixels, kAlMaxPixels);
  MNC_REQUIRE(!out_bits || bits_bytes, "%s: null bits_bytes", who);
  MNC_REQUIRE(!out_bits || n == 0 || (out_bounds && out_offsets && out_areas), "%s: null output pointer", who);
  const size_t bound = (size_t)c.bound_words * 8;
  *bits_bound = bound;
  if (!out_bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(bits_cap >= bound, "%s: bits_cap %zu is below the %zu bytes of the loose frames", who, bits_cap, bound);
  for (int o = 0; o < n; ++o) {
    int* q = out_bounds + 4 * (size_t)o;
    q[0] = 0; q[1] = 0; q[2] = -1; q[3] = -1;
    out_offsets[o] = 0;
    out_areas[o] = 0;
  }
  *bits_bytes = 0;
  if (bound == 0) { clear_error(); return MNC_OK; }        // no frame has a row
  const bool two = B != nullptr;
  AlJob* d_jobs; int *d_idx, *d_words, *d_tile; AlBox* d_box; u64 *d_out, *d_area;
  auto layout = [&](WsLayout l) {
    a.take(l);
    if (two) B->take(l);
    d_jobs = l.take<AlJob>(n);
    d_idx = l.take<int>(c.idx.size());
    d_box = l.take<AlBox>(n);
    d_words = l.take<int>(n);
    d_tile = l.take<int>((size_t)scan_tiles(n) + 1);
    d_out = l.take<u64>((size_t)c.bound_words);
    d_area = l.take<u64>(n);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  std::vector<AlBox> box((size_t)n, AlBox{INT_MAX, INT_MAX, -1, -1});
  std::vector<u64> area((size_t)n, 0ull);
  MNC_HIP_TRY(a.upload(hs));
  if (two) MNC_HIP_TRY(B->upload(hs));
  MNC_HIP_TRY(hs.up(d_jobs, c.jobs.data(), (size_t)n * sizeof(AlJob)));
  MNC_HIP_TRY(hs.up(d_idx, c.idx.data(), c.idx.size() * sizeof(int)));
  MNC_HIP_TRY(hs.up(d_box, box.data(), (size_t)n * sizeof(AlBox)));
  MNC_HIP_TRY(hs.up(d_area, area.data(), (size_t)n * sizeof(u64)));
  const MaskSet va = a.view(), vb = two ? B->view() : va;
  const dim3 grid((unsigned)((c.most_words + kAlThreads - 1) / kAlThreads), (unsigned)n);
  TimedSpan span(g_al_timer);
  span.begin(hs.stream);
  hipLaunchKernelGGL(al_extent_kernel, grid, dim3(kAlThreads), 0, hs.stream, d_jobs, va, vb, d_idx, c.op, c.all, d_box);
  hipLaunchKernelGGL(al_size_kernel, dim3((unsigned)((n + kAlThreads - 1) / kAlThreads)), dim3(kAlThreads), 0, hs.stream, d_jobs, n,
                     d_box, d_words);
  const Scanned first = scan_launch(hs.stream, d_words, n, d_tile);
  hipLaunchKernelGGL(al_fill_kernel, grid, dim3(kAlThreads), 0, hs.stream, d_jobs, va, vb, d_idx, c.op, c.all, d_box, first, d_out,
                     d_area);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(box.data(), d_box, (size_t)n * sizeof(AlBox)));
  MNC_HIP_TRY(hs.down(area.data(), d_area, (size_t)n * sizeof(u64)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  long long at = 0;                                        // the offsets as the scan placed them: the bytes of the tight rows
  for (int o = 0; o < n; ++o) at += mask_bytes(box[o].x2 - box[o].x1 + 1, box[o].y2 - box[o].y1 + 1);
  if (at < 0 || (size_t)at > bound) {                      // (cannot be: a tight frame lies inside its loose one)
    set_error("%s: the result's %lld bytes exceed the bound %zu", who, at, bound);
    return MNC_ERR_HIP;
  }
  MNC_HIP_TRY(hs.down(out_bits, d_out, (size_t)at));
  MNC_HIP_TRY(hs.sync());
  at = 0;
  for (int o = 0; o < n; ++o) {
    int* q = out_bounds + 4 * (size_t)o;
    q[0] = box[o].x1; q[1] = box[o].y1; q[2] = box[o].x2; q[3] = box[o].y2;
    out_offsets[o] = at;
    out_areas[o] = (long long)area[o];
    at += mask_bytes(box[o].x2 - box[o].x1 + 1, box[o].y2 - box[o].y1 + 1);
  }
  *bits_bytes = (size_t)at;
  clear_error();
  return MNC_OK;
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_combine(const int* a_bounds, const long long* a_offsets, const void* a_bits, size_t a_bytes, int n_a, const int* b_bounds,
                     const long long* b_offsets, const void* b_bits, size_t b_bytes, int n_b, int op, const int* window, int* out_bounds,
                     long long* out_offsets, long long* out_areas, void* out_bits, size_t bits_cap, size_t* bits_bound,
                     size_t* bits_bytes, int device_id) {
  const char* who = "mnc_mask_combine";
  MNC_REQUIRE(bits_bound, "%s: null bits_bound", who);
  MNC_REQUIRE(op >= 0 && op <= 5, "%s: op=%d is not 0 (and), 1 (or), 2 (xor), 3 (minus), 4 (copy) or 5 (not)", who, op);
  MNC_REQUIRE(n_b == 0 || n_b == 1 || n_b == n_a, "%s: n_b=%d is not 0, 1 or n_a=%d", who, n_b, n_a);
  MNC_REQUIRE(op >= kAlCopy || n_b > 0 || n_a <= 0, "%s: op=%d needs a set b", who, op);
  MNC_REQUIRE(op != kAlNot || window, "%s: op 5 (not) needs a window", who);
  if (window) {
    for (int k = 0; k < 4; ++k)
      MNC_REQUIRE(window[k] > -kAlMaxCoord && window[k] < kAlMaxCoord, "%s: window coordinate %d out of range", who, window[k]);
    MNC_REQUIRE(window[2] >= window[0] && window[3] >= window[1], "%s: the window (%d, %d, %d, %d) is empty", who, window[0],
                window[1], window[2], window[3]);
  }
  HostMaskSet A, B;
  int rc = al_check_set(who, "a", &A, a_bounds, a_offsets, a_bits, a_bytes, n_a, nullptr);
  if (rc) return rc;
  const bool two = op < kAlCopy && n_b > 0;
  if (two) {
    rc = al_check_set(who, "b", &B, b_bounds, b_offsets, b_bits, b_bytes, n_b, nullptr);
    if (rc) return rc;
  }
  AlCall c;
  c.op = op;
  c.window = window;
  for (int i = 0; i < n_a; ++i) {
    const mnc_mask_info& a = A.info[i];
    if (!two) {
      if (op == kAlNot) c.add(window[0], window[1], window[2], window[3], i, 0, 0);
      else if (al_rows(a)) c.add(a.x1, a.y1, a.x2, a.y2, i, 0, 0);
      else c.add_empty();
      continue;
    }
    const int k = n_b == 1 ? 0 : i;
    const mnc_mask_info& b = B.info[k];
    c.idx.push_back(k);
    const bool ra = al_rows(a), rb = al_rows(b);
    if (op == kAlAnd) {
      if (ra && rb) c.add(std::max(a.x1, b.x1), std::max(a.y1, b.y1), std::min(a.x2, b.x2), std::min(a.y2, b.y2), i, i, i + 1);
      else c.add_empty();
    } else if (op == kAlMinus) {
      if (ra) c.add(a.x1, a.y1, a.x2, a.y2, i, i, i + 1);
      else c.add_empty();
    } else if (ra && rb) {
      c.add(std::min(a.x1, b.x1), std::min(a.y1, b.y1), std::max(a.x2, b.x2), std::max(a.y2, b.y2), i, i, i + 1);
    } else if (ra || rb) {
      const mnc_mask_info& m = ra ? a : b;
      c.add(m.x1, m.y1, m.x2, m.y2, i, i, i + 1);
    } else {
      c.add_empty();
    }
  }
  return al_run(who, c, A, two ? &B : nullptr, out_bounds, out_offsets, out_areas, out_bits, bits_cap, bits_bound, bits_bytes,
                device_id);
}

// see include/mnc_hip.h
int mnc_mask_merge(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const long long* group_ptr,
                   const int* members, int G, int intersect, int* out_bounds, long long* out_offsets, long long* out_areas,
                   void* out_bits, size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id) {
  const char* who = "mnc_mask_merge";
  MNC_REQUIRE(bits_bound, "%s: null bits_bound", who);
  MNC_REQUIRE(G >= 0 && G <= kAlMaxN, "%s: G=%d not in [0, %d]", who, G, kAlMaxN);
  MNC_REQUIRE(G == 0 || group_ptr, "%s: null group_ptr", who);
  HostMaskSet A;
  int rc = al_check_set(who, "masks", &A, bounds, offsets, bits, bytes, n, nullptr);
  if (rc) return rc;
  if (G > 0) {
    MNC_REQUIRE(group_ptr[0] == 0, "%s: group_ptr[0]=%lld is not 0", who, group_ptr[0]);
    for (int g = 0; g < G; ++g) {
      MNC_REQUIRE(group_ptr[g + 1] >= group_ptr[g], "%s: group_ptr is not monotone at %d", who, g);
      MNC_REQUIRE(group_ptr[g + 1] <= kAlMaxMembers, "%s: more than %lld members", who, kAlMaxMembers);
    }
    MNC_REQUIRE(group_ptr[G] == 0 || members, "%s: null members", who);
    for (long long k = 0; k < group_ptr[G]; ++k)
      MNC_REQUIRE(members[k] >= 0 && members[k] < n, "%s: members[%lld]=%d not in [0, %d)", who, k, members[k], n);
  }
  AlCall c;
  c.op = kAlOr;
  c.all = intersect ? 1 : 0;
  if (G > 0) c.idx.assign(members, members + group_ptr[G]);
  for (int g = 0; g < G; ++g) {
    int x1 = INT_MAX, y1 = INT_MAX, x2 = INT_MIN, y2 = INT_MIN;
    bool any = false, every = true;
    for (long long k = group_ptr[g]; k < group_ptr[g + 1]; ++k) {
      const mnc_mask_info& m = A.info[members[k]];
      if (!al_rows(m)) { every = false; continue; }
      if (!any || !intersect) {
        x1 = any ? std::min(x1, m.x1) : m.x1; y1 = any ? std::min(y1, m.y1) : m.y1;
        x2 = any ? std::max(x2, m.x2) : m.x2; y2 = any ? std::max(y2, m.y2) : m.y2;
      } else {
        x1 = std::max(x1, m.x1); y1 = std::max(y1, m.y1); x2 = std::min(x2, m.x2); y2 = std::min(y2, m.y2);
      }
      any = true;
    }
    if (any && (every || !intersect)) c.add(x1, y1, x2, y2, -1, group_ptr[g], group_ptr[g + 1]);
    else c.add_empty();
  }
  return al_run(who, c, A, nullptr, out_bounds, out_offsets, out_areas, out_bits, bits_cap, bits_bound, bits_bytes, device_id);
}

// see include/mnc_hip.h
int mnc_mask_layer(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const float* scores,
                   const int* order, int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits, size_t bits_cap,
                   size_t* bits_bound, size_t* bits_bytes, int device_id) {
  const char* who = "mnc_mask_layer";
  MNC_REQUIRE(bits_bound, "%s: null bits_bound", who);
  MNC_REQUIRE(n <= 0 || order || scores, "%s: neither order nor scores", who);
  HostMaskSet A;
  int rc = al_check_set(who, "masks", &A, bounds, offsets, bits, bytes, n, nullptr);
  if (rc) return rc;
  std::vector<int> rank((size_t)n, -1), seq((size_t)n);
  if (order) {
    for (int k = 0; k < n; ++k) {
      MNC_REQUIRE(order[k] >= 0 && order[k] < n && rank[order[k]] < 0, "%s: order is not a permutation at %d", who, k);
      rank[order[k]] = k;
      seq[k] = order[k];
    }
  } else {
    for (int i = 0; i < n; ++i) {
      MNC_REQUIRE(scores[i] == scores[i], "%s: scores[%d] is NaN", who, i);
      seq[i] = i;
    }
    std::stable_sort(seq.begin(), seq.end(), [&](int p, int q) { return scores[p] > scores[q]; });
    for (int k = 0; k < n; ++k) rank[seq[k]] = k;
  }
  AlCall c;
  c.op = kAlMinus;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = A.info[i];
    if (!al_rows(a)) { c.add_empty(); continue; }
    const long long lo = (long long)c.idx.size();
    for (int k = 0; k < rank[i]; ++k) {                    // the instances before i whose bounds meet i's
      const mnc_mask_info& m = A.info[seq[k]];
      if (al_rows(m) && m.x1 <= a.x2 && m.x2 >= a.x1 && m.y1 <= a.y2 && m.y2 >= a.y1) c.idx.push_back(seq[k]);
    }
    c.add(a.x1, a.y1, a.x2, a.y2, i, lo, (long long)c.idx.size());
  }
  return al_run(who, c, A, nullptr, out_bounds, out_offsets, out_areas, out_bits, bits_cap, bits_bound, bits_bytes, device_id);
}

// see include/mnc_hip.h
int mnc_mask_algebra_timing(int on, double* last_ms) { return g_al_timer.set(on, last_ms); }
