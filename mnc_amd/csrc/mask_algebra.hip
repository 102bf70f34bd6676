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
// The result is tight and its size depends on the data: the protocol, its five launches and its driver are mask_tight.h's.  Here
// the unit of work is a lane per word:
//   al_extent_kernel   one lane per word of the loose frame: al_word, then tight_join.
//   al_fill_kernel     one lane per word of the TIGHT frame: al_word again at the tight position, stored once, then tight_count.
//
// Bound: latency.  100 instances of an image are a few hundred KB of words that sit in L2; a lane reads at most two words per
// operand and row.  A merge reads every member per output word, a layer every listed neighbour.  Measured at 100 instances of a
// 600 x 1000 image, call with its copies / kernels alone: a | b 0.24 ms / 27 us, merge(by="class") 0.21 ms / 69 us (a class's frame
// is nearly the image and every word reads 25 members), layered() 0.15 ms / 26 us (profiles/mask_algebra_bench.txt).  20 VGPRs, no
// LDS and no scratch in any kernel.
#include <algorithm>
#include <climits>
#include <vector>

#include "mask_tight.h"

namespace mnc {

constexpr int kAlThreads = 256;
constexpr long long kAlMaxMembers = 1ll << 20;

enum AlOp { kAlAnd = 0, kAlOr = 1, kAlXor = 2, kAlMinus = 3, kAlCopy = 4, kAlNot = 5 };

// One output instance: its loose frame, the operand of A (-1: none) and the list.  The frame stays the head of the job -- one
// table, one copy and one 32-byte read per lane -- and tight_size_kernel steps over the rest.
struct AlJob : TightFrame {
  int a = -1, lo = 0, hi = 0, pad_ = 0;
};

// The 64 result bits of job j from image column x >= j.fx on, in image row y of the frame.  Both passes call it.
__device__ __forceinline__ u64 al_word(const AlJob& j, const MaskSet& A, const MaskSet& B, const int* __restrict__ idx, int op, int all,
                                       int x, int y) {
  const u64 p = j.a >= 0 ? mask_read(A.info[j.a], A.bits, x, y) : 0ull;
  u64 q = all ? ~0ull : 0ull;
  for (int k = j.lo; k < j.hi; ++k) {
    const u64 r = mask_read(B.info[idx[k]], B.bits, x, y);
    q = all ? q & r : q | r;
  }
  u64 v = op == kAlAnd ? p & q : op == kAlOr ? p | q : op == kAlXor ? p ^ q : op == kAlMinus ? p & ~q : op == kAlCopy ? p : ~p;
  const int valid = j.fx + j.fw - x;                       // columns of the frame from x on
  if (valid < 64) v &= valid > 0 ? (1ull << valid) - 1ull : 0ull;
  return v;
}

// grid (ceil(most loose-frame words / 256), jobs), block 256: a lane per word of the loose frame.
__global__ __launch_bounds__(kAlThreads) void al_extent_kernel(const AlJob* __restrict__ jobs, MaskSet A, MaskSet B,
                                                               const int* __restrict__ idx, int op, int all, TightBox* __restrict__ ext) {
  const int o = blockIdx.y;
  const AlJob j = jobs[o];
  if (j.fw < 1 || j.fh < 1) return;
  const int strips = mask_strips(j.fw);
  const long long t = (long long)blockIdx.x * kAlThreads + threadIdx.x;
  int y = 0, c = 0;
  u64 v = 0ull;
  if (t < (long long)j.fh * strips) {
    y = (int)(t / strips);
    c = (int)(t - (long long)y * strips);
    v = al_word(j, A, B, idx, op, all, j.fx + c * 64, j.fy + y);
  }
  tight_join(ext + o, v, c * 64, y);
}

// grid (ceil(most loose-frame words / 256), jobs), block 256: a lane per word of the tight frame.
__global__ __launch_bounds__(kAlThreads) void al_fill_kernel(const AlJob* __restrict__ jobs, MaskSet A, MaskSet B,
                                                             const int* __restrict__ idx, int op, int all,
                                                             const TightBox* __restrict__ box, Scanned first, u64* __restrict__ out,
                                                             u64* __restrict__ area) {
  const int o = blockIdx.y;
  const TightBox b = box[o];
  if (b.x2 < b.x1) return;
  const AlJob j = jobs[o];
  const int strips = mask_strips(b.x2 - b.x1 + 1);
  const long long t = (long long)blockIdx.x * kAlThreads + threadIdx.x;
  const bool live = t < (long long)(b.y2 - b.y1 + 1) * strips;
  if (__ballot(live) == 0ull) return;                      // (the whole wave)
  u64 v = 0ull;
  if (live) {
    const int y = (int)(t / strips), c = (int)(t - (long long)y * strips);
    v = al_word(j, A, B, idx, op, all, b.x1 + c * 64, b.y1 + y);
    out[(long long)first.at(o) + t] = v;
  }
  tight_count(area + o, v);
}

namespace {

// One call (mask_tight.h): the jobs, and beside them the sets (B null: A is B), the lists of the jobs and the expression.
struct AlCall : TightCall<AlJob> {
  HostMaskSet& A;
  HostMaskSet* B;
  std::vector<int> idx;
  int* d_idx = nullptr;
  int op = kAlOr, all = 0;
  AlCall(HostMaskSet& a, HostMaskSet* b) : A(a), B(b) {}
  // The job of the next output instance: the frame (x1, y1, x2, y2) intersected with the window.
  void add(int x1, int y1, int x2, int y2, int a, long long lo, long long hi) {
    AlJob j;
    j.a = a; j.lo = (int)lo; j.hi = (int)hi;
    TightCall::add(x1, y1, x2, y2, j);
  }
  void take(WsLayout& l) {
    A.take(l);
    if (B) B->take(l);
    d_idx = l.take<int>(idx.size());
  }
  hipError_t upload(const HostScope& hs) const {
    hipError_t e = A.upload(hs);
    if (e == hipSuccess && B) e = B->upload(hs);
    return e != hipSuccess ? e : hs.up(d_idx, idx.data(), idx.size() * sizeof(int));
  }
  dim3 grid() const { return dim3((unsigned)((most_words + kAlThreads - 1) / kAlThreads), (unsigned)jobs.size()); }
  void extent(hipStream_t s, const AlJob* d_jobs, TightBox* d_ext) const {
    hipLaunchKernelGGL(al_extent_kernel, grid(), dim3(kAlThreads), 0, s, d_jobs, A.view(), (B ? B : &A)->view(), d_idx, op, all,
                       d_ext);
  }
  void fill(hipStream_t s, const AlJob* d_jobs, const TightBox* d_box, Scanned first, u64* d_out, u64* d_area) const {
    hipLaunchKernelGGL(al_fill_kernel, grid(), dim3(kAlThreads), 0, s, d_jobs, A.view(), (B ? B : &A)->view(), d_idx, op, all,
                       d_box, first, d_out, d_area);
  }
};

// What every entry refuses about a set, as mnc_mask_boundary does.
int al_check_set(const char* who, const char* name, HostMaskSet* set, const int* bounds, const long long* offsets, const void* bits,
                 size_t bytes, int n, const float* scores) {
  MNC_REQUIRE(n >= 0 && n <= kTightMaxN, "%s: %s has n=%d not in [0, %d]", who, name, n, kTightMaxN);
  return set->check(who, name, bounds, offsets, bits, bytes, n, nullptr, scores);
}

CallTimer g_al_timer;

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
    const int rc = tight_check_window(who, window);
    if (rc) return rc;
  }
  HostMaskSet A, B;
  int rc = al_check_set(who, "a", &A, a_bounds, a_offsets, a_bits, a_bytes, n_a, nullptr);
  if (rc) return rc;
  const bool two = op < kAlCopy && n_b > 0;
  if (two) {
    rc = al_check_set(who, "b", &B, b_bounds, b_offsets, b_bits, b_bytes, n_b, nullptr);
    if (rc) return rc;
  }
  AlCall c(A, two ? &B : nullptr);
  c.op = op;
  c.window = window;
  for (int i = 0; i < n_a; ++i) {
    const mnc_mask_info& a = A.info[i];
    if (!two) {
      if (op == kAlNot) c.add(window[0], window[1], window[2], window[3], i, 0, 0);
      else if (mask_has_rows(a)) c.add(a.x1, a.y1, a.x2, a.y2, i, 0, 0);
      else c.add_empty();
      continue;
    }
    const int k = n_b == 1 ? 0 : i;
    const mnc_mask_info& b = B.info[k];
    c.idx.push_back(k);
    const bool ra = mask_has_rows(a), rb = mask_has_rows(b);
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
  return tight_run(who, c, g_al_timer, out_bounds, out_offsets, out_areas, out_bits, bits_cap, bits_bound, bits_bytes, device_id);
}

// see include/mnc_hip.h
int mnc_mask_merge(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const long long* group_ptr,
                   const int* members, int G, int intersect, int* out_bounds, long long* out_offsets, long long* out_areas,
                   void* out_bits, size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id) {
  const char* who = "mnc_mask_merge";
  MNC_REQUIRE(bits_bound, "%s: null bits_bound", who);
  MNC_REQUIRE(G >= 0 && G <= kTightMaxN, "%s: G=%d not in [0, %d]", who, G, kTightMaxN);
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
  AlCall c(A, nullptr);
  c.op = kAlOr;
  c.all = intersect ? 1 : 0;
  if (G > 0) c.idx.assign(members, members + group_ptr[G]);
  for (int g = 0; g < G; ++g) {
    int x1 = INT_MAX, y1 = INT_MAX, x2 = INT_MIN, y2 = INT_MIN;
    bool any = false, every = true;
    for (long long k = group_ptr[g]; k < group_ptr[g + 1]; ++k) {
      const mnc_mask_info& m = A.info[members[k]];
      if (!mask_has_rows(m)) { every = false; continue; }
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
  return tight_run(who, c, g_al_timer, out_bounds, out_offsets, out_areas, out_bits, bits_cap, bits_bound, bits_bytes, device_id);
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
  AlCall c(A, nullptr);
  c.op = kAlMinus;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = A.info[i];
    if (!mask_has_rows(a)) { c.add_empty(); continue; }
    const long long lo = (long long)c.idx.size();
    for (int k = 0; k < rank[i]; ++k) {                    // the instances before i whose bounds meet i's
      const mnc_mask_info& m = A.info[seq[k]];
      if (mask_has_rows(m) && m.x1 <= a.x2 && m.x2 >= a.x1 && m.y1 <= a.y2 && m.y2 >= a.y1) c.idx.push_back(seq[k]);
    }
    c.add(a.x1, a.y1, a.x2, a.y2, i, lo, (long long)c.idx.size());
  }
  return tight_run(who, c, g_al_timer, out_bounds, out_offsets, out_areas, out_bits, bits_cap, bits_bound, bits_bytes, device_id);
}

// see include/mnc_hip.h
int mnc_mask_algebra_timing(int on, double* last_ms) { return g_al_timer.set(on, last_ms); }
