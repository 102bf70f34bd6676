// Connected components of packed instance masks for gfx950 (include/mnc_hip.h n12), on the PackedMasks layout of inst_masks.hip (n5),
// without unpacking a mask: the component table, the selection by area, the filling of holes, one instance per component.  Runs are
// labelled, not pixels; the helpers that work on values and on the parent array are mask_cc.h (host and device).
//
// Every instance is seen through a VIEW: the mask itself (frame = 0), or, for the holes, the complement of its box grown by a frame
// of one pixel (frame = 1: (w + 2) x (h + 2), the frame set).  The words of all views of a set are numbered in raster order, instance
// after instance (at most 2^25 of them); one thread works on one word.
//   cc_count_kernel     the run starts of a word, v & ~((v << 1) | carry), counted.
//   scan_launch         (scan.hip) the exclusive prefix of the counts: in tiles of 1024, then over the tiles; a run's id is the prefix
//                       at its word + the starts below it in the word (cc_run_at).  The total is read back: it sizes parent[].
//   cc_union_kernel     the runs of a word united with the runs of the row above that they touch (cc_link_word): lock-free, the
//                       smaller id always becomes the parent.
//   cc_flatten_kernel   parent[r] = the root of r; flag[r] = r is a root.  The scan of the flags numbers the components: roots are
//                       the first runs of their components, run ids are in raster order, so the numbers are in first-pixel order.
//   cc_comp_ptr_kernel  the first component of every instance: the prefix at its first run.  Read back: it sizes the table.
//   cc_table_kernel     area (atomic add), box (atomic min / max) per component, four atomics per run by the thread that holds the
//                       run's start; anchor, y1 and the root run are stored by the one thread that holds the root's start.
//   cc_rank_kernel      one workgroup per instance: the `keep`-th largest key (area, then the lower number) by a bitwise search.
//   cc_select_kernel / cc_fill_kernel / cc_split_kernel   the writers: one thread per word of the result takes the runs of the
//                       source words under it, asks their roots, and stores the word once, padding cleared.
// Nothing depends on the order in which an atomic arrives: sums, minima and maxima of integers, and the final parent[] is the root
// of every run whatever the order of the links was.
// Bound: every pass reads the words of the set a small constant number of times from L2 and 4 to 12 bytes per word of prefix;
// the union and the writers add one dependent load per run.  tools/mask_components_bench.py, profiles/mask_components_bench.txt.
#include <atomic>
#include <vector>

#include "mask_cc.h"
#include "mask_set.h"
#include "scan.h"

namespace mnc {

constexpr int kCcThreads = 256;
constexpr int kCcMaxN = 2048;                   // instances of one call
constexpr long long kCcMaxWords = 1ll << 25;    // words of all views of one call: 32 runs a word, run ids < 2^30

// The view of one instance: what the host adds to the set's own table (MaskSet::info).
struct CcInst {
  int vw, vh, vs;      // the view's width, height and words per row (0 without rows)
  int rs;              // the words per row of the mask itself
  int word0;           // its first word among the words of all views
  int real0;           // its first word among the words of all masks (the writers of select and fill_holes)
};

// One instance as a thread sees it: the set's entry and the view together.
struct CcGeom {
  int w, x1, y1;       // the bounds' width and corner
  int vw, vh, vs, rs, word0;
  const u64* rows;     // the first row's words
};

__device__ __forceinline__ CcGeom cc_geom(const MaskSet& A, const CcInst* __restrict__ insts, int i) {
  const mnc_mask_info s = A.info[i];
  const CcInst v = insts[i];
  return {s.x2 - s.x1 + 1, s.x1, s.y1, v.vw, v.vh, v.vs, v.rs, v.word0, A.bits + s.offset / 8};
}

// Word j of row y of the view; 0 outside the row.
__device__ __forceinline__ u64 cc_view_word(const CcGeom& m, int y, int j, int frame) {
  if (j < 0 || j >= m.vs) return 0ull;
  if (!frame) return mask_word(m.rows + (long long)y * m.rs, j, m.rs, m.w);
  // view pixel (X, Y) is the complement of mask pixel (X - 1, Y - 1); mask_word_at reads 0 before and past the row
  u64 v = y == 0 || y == m.vh - 1 ? ~0ull : ~mask_word_at(m.rows + (long long)(y - 1) * m.rs, j * 64 - 1, m.rs, m.w);
  const int valid = m.vw - (j << 6);
  if (valid < 64) v &= (1ull << valid) - 1ull;
  return v;
}

__device__ __forceinline__ u64 cc_view_starts(const CcGeom& m, int y, int j, int frame, u64 v) {
  return cc_starts(v, cc_view_word(m, y, j - 1, frame) >> 63);
}

struct CcAt {
  int i, y, j;
};

// The instance, row and word of word g: the last instance that begins at or before g (one without words begins where the next does).
template <bool kReal>
__device__ __forceinline__ CcAt cc_decode(const CcInst* __restrict__ insts, int n, int g) {
  const int lo = kReal ? mask_owner<&CcInst::real0>(insts, n, g) : mask_owner<&CcInst::word0>(insts, n, g);
  const int local = g - (kReal ? insts[lo].real0 : insts[lo].word0);
  const int per = kReal ? insts[lo].rs : insts[lo].vs;
  return {lo, local / per, local % per};
}

// dst[key] += v for the live lanes of a wave, every lane of which comes here: one atomic per wave where its live lanes share the
// key (neighbouring words of one instance, the usual case), one per lane otherwise.  Integer sums: the same total either way.
__device__ __forceinline__ void cc_wave_add(unsigned long long* __restrict__ dst, int key, int v, bool live) {
  const bool has = live && v != 0;
  const u64 any = __ballot(has);
  if (!any) return;                                      // (uniform)
  const int first = __builtin_ctzll(any), lane = threadIdx.x & 63;
  const int key0 = __shfl(key, first);
  int sum = has ? v : 0;
  if (__ballot(has && key != key0)) {                    // (uniform)
    if (has) atomicAdd(dst + key, (unsigned long long)sum);
    return;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == first) atomicAdd(dst + key0, (unsigned long long)sum);
}

// grid ceil(words / 256), block 256.
__global__ __launch_bounds__(kCcThreads) void cc_count_kernel(MaskSet A, const CcInst* __restrict__ insts, int n, int frame, int words,
                                                              int* __restrict__ cnt) {
  const int g = blockIdx.x * kCcThreads + threadIdx.x;
  if (g >= words) return;
  const CcAt at = cc_decode<false>(insts, n, g);
  const CcGeom m = cc_geom(A, insts, at.i);
  const u64 v = cc_view_word(m, at.y, at.j, frame);
  cnt[g] = v ? __popcll(cc_view_starts(m, at.y, at.j, frame, v)) : 0;
}

// grid ceil(runs / 256), block 256.
__global__ __launch_bounds__(kCcThreads) void cc_init_kernel(int* __restrict__ parent, int runs) {
  const int r = blockIdx.x * kCcThreads + threadIdx.x;
  if (r < runs) parent[r] = r;
}

// grid ceil(words / 256), block 256.  e = 1: 8-connectivity.
__global__ __launch_bounds__(kCcThreads) void cc_union_kernel(MaskSet A, const CcInst* __restrict__ insts, int n, int frame, int words,
                                                              Scanned base, int* parent, int e) {
  const int g = blockIdx.x * kCcThreads + threadIdx.x;
  if (g >= words) return;
  const CcAt at = cc_decode<false>(insts, n, g);
  if (at.y == 0) return;
  const CcGeom m = cc_geom(A, insts, at.i);
  const u64 v = cc_view_word(m, at.y, at.j, frame);
  if (!v) return;
  const int ga = g - m.vs, ya = at.y - 1;                // the word above
  const u64 a = cc_view_word(m, ya, at.j, frame);
  const u64 a_prev = cc_view_word(m, ya, at.j - 1, frame);
  int left_run = -1, right_run = -1;
  if (e && (v & 1ull) && (a_prev >> 63))
    left_run = cc_run_at(base.at(ga - 1), cc_view_starts(m, ya, at.j - 1, frame, a_prev), 63);
  if (e && (v >> 63)) {
    const u64 a_next = cc_view_word(m, ya, at.j + 1, frame);
    if (a_next & 1ull) right_run = cc_run_at(base.at(ga + 1), cc_starts(a_next, a >> 63), 0);
  }
  if (!a && left_run < 0 && right_run < 0) return;
  // (every find inside ends: parents only decrease, mask_cc.h:cc_find)
  cc_link_word(parent, v, cc_view_starts(m, at.y, at.j, frame, v), base.at(g), a, cc_starts(a, a_prev >> 63), a ? base.at(ga) : 0,
               left_run, right_run, e);
}

// grid ceil(runs / 256), block 256.  After the unions: parent[r] = the root of r (a lowering like any other: threads that still
// walk through r find the same root), flag[r] = r is one.
__global__ __launch_bounds__(kCcThreads) void cc_flatten_kernel(int* parent, int runs, int* __restrict__ flag) {
  const int r = blockIdx.x * kCcThreads + threadIdx.x;
  if (r >= runs) return;
  const int root = cc_root(parent, r);
  if (root != r) cc_lower(parent + r, root);
  flag[r] = root == r;
}

// grid ceil((n + 1) / 256), block 256.  comp_ptr [n + 1]: the components before the first run of instance i.
__global__ __launch_bounds__(kCcThreads) void cc_comp_ptr_kernel(const CcInst* __restrict__ insts, int n, int words, Scanned base, Scanned number,
                                                                 long long* __restrict__ comp_ptr) {
  const int i = blockIdx.x * kCcThreads + threadIdx.x;
  if (i > n) return;
  const int w0 = i < n ? insts[i].word0 : words;
  comp_ptr[i] = number.upto(base.upto(w0));
}

// The table of the components on the device.
struct CcTable {
  unsigned long long* area;   // [C]
  int* box;                   // [C][4]
  int* anchor;                // [C][2]
  int* root;                  // [C] the root run
};

// grid ceil(C / 256), block 256.
__global__ __launch_bounds__(kCcThreads) void cc_table_init_kernel(CcTable t, long long comps) {
  const long long c = (long long)blockIdx.x * kCcThreads + threadIdx.x;
  if (c >= comps) return;
  t.area[c] = 0ull;
  t.box[4 * c] = 0x7fffffff; t.box[4 * c + 1] = 0x7fffffff;
  t.box[4 * c + 2] = -0x7fffffff; t.box[4 * c + 3] = -0x7fffffff;
}

// grid ceil(words / 256), block 256 (frame = 0 views: the masks themselves).  One thread per word takes the runs that START in it
// and walks each to its end through the words that follow: four atomics per run, not per word of it.
__global__ __launch_bounds__(kCcThreads) void cc_table_kernel(MaskSet A, const CcInst* __restrict__ insts, int n, int words,
                                                              Scanned base, const int* __restrict__ parent, Scanned number, CcTable t) {
  const int g = blockIdx.x * kCcThreads + threadIdx.x;
  if (g >= words) return;
  const CcAt at = cc_decode<false>(insts, n, g);
  const CcGeom m = cc_geom(A, insts, at.i);
  u64 v = cc_view_word(m, at.y, at.j, 0);
  if (!v) return;
  const u64 starts = cc_view_starts(m, at.y, at.j, 0, v);
  const int b = base.at(g), X = m.x1 + at.j * 64, y = m.y1 + at.y;
  while (v) {
    const u64 seg = cc_take_seg(v);
    if (!(starts & seg)) continue;                       // goes on from the word before: counted where it starts
    const int lo = cc_low_bit(seg);
    int len = __popcll(seg);
    if (seg >> 63)
      for (int j = at.j + 1; j < m.vs; ++j) {            // the run's pieces in the following words
        const u64 next = cc_view_word(m, at.y, j, 0);
        const int more = ~next ? cc_low_bit(~next) : 64;
        len += more;
        if (more < 64) break;
      }
    const int r = cc_run_at(b, starts, lo), root = parent[r];
    const int c = number.at(root);
    atomicAdd(&t.area[c], (unsigned long long)len);
    atomicMin(&t.box[4 * c], X + lo);
    atomicMax(&t.box[4 * c + 2], X + lo + len - 1);
    atomicMax(&t.box[4 * c + 3], y);
    if (r == root) {                                     // the first run of the component: one thread per component
      t.box[4 * c + 1] = y;
      t.anchor[2 * c] = X + lo; t.anchor[2 * c + 1] = y;
      t.root[c] = r;
    }
  }
}

// The order of the selection: larger area first, equal areas to the lower number (k = the number inside the instance).
__device__ __forceinline__ u64 cc_key(unsigned long long area, long long k) { return (area << 32) | (u64)(0xffffffffu - (unsigned)k); }

// grid n, block 256.  thr[i] = the keep-th largest key of instance i's components; 0 when all of them are among the keep largest.
__global__ __launch_bounds__(kCcThreads) void cc_rank_kernel(const long long* __restrict__ comp_ptr, const unsigned long long* __restrict__ area,
                                                             int keep, u64* __restrict__ thr) {
  __shared__ int s_wave[kCcThreads / 64];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long lo = comp_ptr[i], count = comp_ptr[i + 1] - lo;
  if (keep == 0 || count <= keep) {                      // (uniform over the workgroup)
    if (threadIdx.x == 0) thr[i] = 0ull;
    return;
  }
  // The largest T that at least `keep` keys reach, bit by bit from the top.  The keys differ, so exactly `keep` reach it.  A count
  // is capped at 2^30 per thread sum -- more than `keep` (an int) either way.
  u64 T = 0ull;
  for (int bit = 63; bit >= 0; --bit) {
    const u64 cand = T | (1ull << bit);
    int mine = 0;
    for (long long k = threadIdx.x; k < count; k += kCcThreads) mine += cc_key(area[lo + k], k) >= cand;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    long long reach = 0;
    for (int k = 0; k < kCcThreads / 64; ++k) reach += s_wave[k];
    if (reach >= keep) T = cand;
    __syncthreads();                                     // s_wave is written again
  }
  if (threadIdx.x == 0) thr[i] = T;
}

// grid ceil(words / 256), block 256.  out: the words at the input's places; areas [n] are added to.
__global__ __launch_bounds__(kCcThreads) void cc_select_kernel(MaskSet A, const CcInst* __restrict__ insts, int n, int words,
                                                               Scanned base, const int* __restrict__ parent, Scanned number,
                                                               const long long* __restrict__ comp_ptr,
                                                               const unsigned long long* __restrict__ area, const u64* __restrict__ thr,
                                                               long long min_area, u64* __restrict__ out,
                                                               unsigned long long* __restrict__ out_area) {
  const int g = blockIdx.x * kCcThreads + threadIdx.x;
  const bool live = g < words;
  int inst = 0, count = 0;
  if (live) {
    const CcAt at = cc_decode<false>(insts, n, g);
    const CcGeom m = cc_geom(A, insts, at.i);
    u64 v = cc_view_word(m, at.y, at.j, 0), kept = 0ull;
    if (v) {
      const u64 starts = cc_view_starts(m, at.y, at.j, 0, v);
      const int b = base.at(g);
      const long long c0 = comp_ptr[at.i];
      const u64 T = thr[at.i];
      while (v) {
        const u64 seg = cc_take_seg(v);
        const long long c = number.at(parent[cc_run_at(b, starts, cc_low_bit(seg))]);
        const unsigned long long ar = area[c];
        if ((long long)ar >= min_area && cc_key(ar, c - c0) >= T) kept |= seg;
      }
    }
    out[(m.rows - A.bits) + (long long)at.y * m.rs + at.j] = kept;
    inst = at.i;
    count = __popcll(kept);
  }
  cc_wave_add(out_area, inst, count, live);
}

// grid ceil(real words / 256), block 256.  The labelling ran on the frame = 1 views; the frame's component is the one of the
// instance's first run.  out as cc_select_kernel's.
__global__ __launch_bounds__(kCcThreads) void cc_fill_kernel(MaskSet A, const CcInst* __restrict__ insts, int n, int real_words,
                                                             Scanned base, const int* __restrict__ parent, u64* __restrict__ out,
                                                             unsigned long long* __restrict__ out_area) {
  const int g = blockIdx.x * kCcThreads + threadIdx.x;
  const bool live = g < real_words;
  int inst = 0, count = 0;
  if (live) {
    const CcAt at = cc_decode<true>(insts, n, g);
    const CcGeom m = cc_geom(A, insts, at.i);
    u64 word = mask_word(m.rows + (long long)at.y * m.rs, at.j, m.rs, m.w);
    const int outside = base.at(m.word0);                // view pixel (0, 0) is set and begins the first run, a root
    // mask pixel x of row y is view pixel (x + 1, y + 1): bits 1 .. 63 of view word j and bit 0 of view word j + 1
    for (int k = 0; k < 2; ++k) {
      const int J = at.j + k;
      const u64 whole = cc_view_word(m, at.y + 1, J, 1);
      u64 v = k ? whole & 1ull : whole;
      if (!v) continue;
      const u64 starts = cc_view_starts(m, at.y + 1, J, 1, whole);
      const int b = base.at(m.word0 + (at.y + 1) * m.vs + J);
      while (v) {
        const u64 seg = cc_take_seg(v);
        if (parent[cc_run_at(b, starts, cc_low_bit(seg))] != outside) word |= k ? seg << 63 : seg >> 1;
      }
    }
    out[(m.rows - A.bits) + (long long)at.y * m.rs + at.j] = word;
    inst = at.i;
    count = __popcll(word);
  }
  cc_wave_add(out_area, inst, count, live);
}

// grid ceil(out words / 256), block 256.  One instance per component: oword [C + 1] the first word of each in `out`, source [C]
// its instance; box and root from the table.
__global__ __launch_bounds__(kCcThreads) void cc_split_kernel(MaskSet A, const CcInst* __restrict__ insts, Scanned base,
                                                              const int* __restrict__ parent, CcTable t, long long comps,
                                                              const long long* __restrict__ oword, const int* __restrict__ source,
                                                              long long out_words, u64* __restrict__ out) {
  const long long g = (long long)blockIdx.x * kCcThreads + threadIdx.x;
  if (g >= out_words) return;
  long long lo = 0, hi = comps - 1;                      // the component that holds word g (every component has words)
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (oword[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const long long c = lo;
  const CcGeom m = cc_geom(A, insts, source[c]);
  const int ow = t.box[4 * c + 2] - t.box[4 * c] + 1, os = mask_strips(ow);
  const int row = (int)((g - oword[c]) / os), j = (int)((g - oword[c]) % os);
  const int y = t.box[4 * c + 1] - m.y1 + row, X0 = t.box[4 * c] - m.x1 + j * 64;   // in the instance
  const int q = X0 >> 6, s = X0 & 63, root = t.root[c];
  u64 word = 0ull;
  for (int k = 0; k < 2; ++k) {
    if (k && !s) break;
    u64 v = cc_view_word(m, y, q + k, 0);
    if (!v) continue;
    const u64 starts = cc_view_starts(m, y, q + k, 0, v);
    const int b = base.at(m.word0 + y * m.vs + q + k);
    while (v) {
      const u64 seg = cc_take_seg(v);
      if (parent[cc_run_at(b, starts, cc_low_bit(seg))] == root) word |= k ? seg << (64 - s) : seg >> s;
    }
  }
  const int valid = ow - (j << 6);
  if (valid < 64) word &= (1ull << valid) - 1ull;
  out[g] = word;
}

namespace {

// The second and third workspace of a call, per device: sized once the run total resp. the component total is read back (the
// HostScope workspace holds what is known before the first launch and cannot grow without losing it).  Guarded by the HostScope's
// mutex, which the call holds to its end.
DevArena g_cc_runs[16], g_cc_comps[16];

// mnc_mask_components_timing: a HIP event pair around the launches of the next calls, the last call's time kept
CallTimer g_cc_timer;

inline int cc_blocks(long long items) { return (int)((items + kCcThreads - 1) / kCcThreads); }

// The labelling of one set: what the host knows before the first launch, the buffers, the launch sequence.
struct CcJob {
  const char* who;
  HostMaskSet set;
  std::vector<CcInst> insts;          // [n + 1]
  int n = 0, frame = 0, e = 0, device = 0;
  int words = 0, real_words = 0;      // of the views, of the masks
  // HostScope workspace
  CcInst* d_insts = nullptr;
  int *d_cnt = nullptr, *d_tile = nullptr;
  long long* d_comp_ptr = nullptr;
  // g_cc_runs
  int *d_parent = nullptr, *d_flag = nullptr, *d_tile2 = nullptr;
  int runs = 0;
  std::vector<long long> comp_ptr;    // [n + 1], read back
  long long comps = 0;
  // g_cc_comps
  CcTable table = {};
  u64* d_thr = nullptr;
  long long* d_oword = nullptr;
  int* d_source = nullptr;

  Scanned base = {}, number = {};     // the scans of d_cnt over the words and of d_flag over the runs, once launched

  // The checks of every entry, before anything is launched.  ordered: the rows must stand in order without overlap.
  int prepare(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n_in, int connectivity, int frame_in,
              bool ordered, int device_id) {
    MNC_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity=%d is not 4 or 8", who, connectivity);
    MNC_REQUIRE(n_in >= 0 && n_in <= kCcMaxN, "%s: n=%d not in [0, %d]", who, n_in, kCcMaxN);
    n = n_in; frame = frame_in; e = connectivity == 8; device = device_id;
    const int rc = set.check(who, "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
    if (rc) return rc;
    insts.assign((size_t)n + 1, CcInst());
    long long at = 0, real = 0, end = 0;
    for (int i = 0; i < n; ++i) {
      const mnc_mask_info& s = set.info[i];
      CcInst& m = insts[i];
      const int w = s.x2 - s.x1 + 1, h = s.y2 - s.y1 + 1;
      const bool rows = w >= 1 && h >= 1;
      m.vw = rows ? w + 2 * frame : 0; m.vh = rows ? h + 2 * frame : 0; m.vs = mask_strips(m.vw);
      m.rs = rows ? mask_strips(w) : 0;
      m.word0 = (int)at; m.real0 = (int)real;
      at += (long long)m.vh * m.vs;
      real += rows ? (long long)h * m.rs : 0;
      MNC_REQUIRE(at <= kCcMaxWords, "%s: more than %lld words of rows in the set (at masks[%d])", who, kCcMaxWords, i);
      if (rows && ordered) {
        MNC_REQUIRE(s.offset >= end, "%s: the rows of masks[%d] (offset %lld) begin before the end of the rows before (%lld)", who, i,
                    s.offset, end);
        end = s.offset + mask_bytes(w, h);
      }
    }
    insts[n].word0 = (int)at; insts[n].real0 = (int)real;
    words = (int)at; real_words = (int)real;
    comp_ptr.assign((size_t)n + 1, 0);
    return MNC_OK;
  }

  void take(WsLayout& l) {
    set.take(l);
    d_insts = l.take<CcInst>((size_t)n + 1);
    d_cnt = l.take<int>(words);
    d_tile = l.take<int>((size_t)scan_tiles(words) + 1);
    d_comp_ptr = l.take<long long>((size_t)n + 1);
  }

  // Upload, count, unite, number: runs, comp_ptr and comps are known on the host afterwards (two read-backs).  want_comps = false
  // (fill_holes) stops after the flattening.
  int label(const HostScope& hs, bool want_comps) {
    hipStream_t s = hs.stream;
    MNC_HIP_TRY(set.upload(hs));
    MNC_HIP_TRY(hs.up(d_insts, insts.data(), insts.size() * sizeof(CcInst)));
    hipLaunchKernelGGL(cc_count_kernel, dim3(cc_blocks(words)), dim3(kCcThreads), 0, s, set.view(), d_insts, n, frame, words, d_cnt);
    base = scan_launch(s, d_cnt, words, d_tile);
    MNC_HIP_TRY(hipGetLastError());
    MNC_HIP_TRY(hs.down(&runs, d_tile + base.tiles, sizeof(int)));
    MNC_HIP_TRY(hs.sync());
    comps = 0;
    if (runs <= 0) return MNC_OK;                        // every mask is empty: comp_ptr stays 0
    auto layout = [&](WsLayout l) {
      d_parent = l.take<int>(runs);
      d_flag = l.take<int>(runs);
      d_tile2 = l.take<int>((size_t)scan_tiles(runs) + 1);
      return l.bytes();
    };
    const size_t need = layout(WsLayout());
    const int rc = arena_ensure(&g_cc_runs[device], need, (need >> 1) + 4096, "connected-component run buffers", s);
    if (rc) return rc;
    layout(WsLayout(g_cc_runs[device].p));
    hipLaunchKernelGGL(cc_init_kernel, dim3(cc_blocks(runs)), dim3(kCcThreads), 0, s, d_parent, runs);
    hipLaunchKernelGGL(cc_union_kernel, dim3(cc_blocks(words)), dim3(kCcThreads), 0, s, set.view(), d_insts, n, frame, words, base, d_parent, e);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_blocks(runs)), dim3(kCcThreads), 0, s, d_parent, runs, d_flag);
    if (want_comps) {
      number = scan_launch(s, d_flag, runs, d_tile2);
      hipLaunchKernelGGL(cc_comp_ptr_kernel, dim3(cc_blocks(n + 1)), dim3(kCcThreads), 0, s, d_insts, n, words, base, number, d_comp_ptr);
    }
    MNC_HIP_TRY(hipGetLastError());
    if (want_comps) {
      MNC_HIP_TRY(hs.down(comp_ptr.data(), d_comp_ptr, comp_ptr.size() * 8));
      MNC_HIP_TRY(hs.sync());
      comps = comp_ptr[n];
    }
    return MNC_OK;
  }

  // The table of the components (comps > 0), with room for the selection's thresholds and the split's lists behind it.
  int make_table(const HostScope& hs, bool split) {
    auto layout = [&](WsLayout l) {
      table.area = l.take<unsigned long long>((size_t)comps);
      table.box = l.take<int>(4 * (size_t)comps);
      table.anchor = l.take<int>(2 * (size_t)comps);
      table.root = l.take<int>((size_t)comps);
      d_thr = l.take<u64>(n);
      d_oword = l.take<long long>(split ? (size_t)comps + 1 : 0);
      d_source = l.take<int>(split ? (size_t)comps : 0);
      return l.bytes();
    };
    const size_t need = layout(WsLayout());
    const int rc = arena_ensure(&g_cc_comps[device], need, (need >> 1) + 4096, "connected-component tables", hs.stream);
    if (rc) return rc;
    layout(WsLayout(g_cc_comps[device].p));
    hipLaunchKernelGGL(cc_table_init_kernel, dim3(cc_blocks(comps)), dim3(kCcThreads), 0, hs.stream, table, comps);
    hipLaunchKernelGGL(cc_table_kernel, dim3(cc_blocks(words)), dim3(kCcThreads), 0, hs.stream, set.view(), d_insts, n, words, base,
                       d_parent, number, table);
    MNC_HIP_TRY(hipGetLastError());
    return MNC_OK;
  }

  // The rows of the result of select / fill_holes, which stand where the input's do: the pieces of [0, used) that hold rows.
  int download_rows(const HostScope& hs, void* out_bits, const u64* d_out) const {
    long long lo = -1, hi = -1;
    for (int i = 0; i <= n; ++i) {
      const long long a = i < n ? set.info[i].offset : -1;
      const long long b = i < n ? a + mask_bytes(set.info[i].x2 - set.info[i].x1 + 1, set.info[i].y2 - set.info[i].y1 + 1) : -1;
      if (i < n && a == b) continue;
      if (i < n && a == hi) { hi = b; continue; }
      if (hi > lo) MNC_HIP_TRY(hs.down((char*)out_bits + lo, (const char*)d_out + lo, (size_t)(hi - lo)));
      lo = a; hi = b;
    }
    return MNC_OK;
  }
};

// select and fill_holes: the same outputs, the same frame around the writer.
int cc_rewrite(CcJob& job, const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
               bool fill, int min_area, int keep, long long* out_areas, void* out_bits, size_t bits_cap, int device_id) {
  const char* who = job.who;
  MNC_REQUIRE(min_area >= 0 && keep >= 0, "%s: min_area=%d or keep=%d is negative", who, min_area, keep);
  int rc = job.prepare(bounds, offsets, bits, bytes, n, connectivity, fill ? 1 : 0, true, device_id);
  if (rc) return rc;
  MNC_REQUIRE(n == 0 || out_areas, "%s: null out_areas", who);
  MNC_REQUIRE(job.set.used == 0 || out_bits, "%s: null out_bits", who);
  MNC_REQUIRE(bits_cap >= job.set.used, "%s: bits_cap %zu is below the %zu bytes the rows reach", who, bits_cap, job.set.used);
  for (int i = 0; i < n; ++i) out_areas[i] = 0;
  if (job.words == 0) { clear_error(); return MNC_OK; }
  u64* d_out; unsigned long long* d_area;
  auto layout = [&](WsLayout l) {
    job.take(l);
    d_out = l.take<u64>(job.set.used / 8);
    d_area = l.take<unsigned long long>(n);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  TimedSpan span(g_cc_timer);
  span.begin(hs.stream);
  rc = job.label(hs, !fill);
  if (rc) return rc;
  hipStream_t s = hs.stream;
  MNC_HIP_TRY(hipMemsetAsync(d_area, 0, (size_t)n * 8, s));
  if (job.runs <= 0) {
    // nothing is set (select), resp. nothing can be: a view with a frame always has runs
    MNC_HIP_TRY(hipMemsetAsync(d_out, 0, job.set.used, s));
  } else if (fill) {
    hipLaunchKernelGGL(cc_fill_kernel, dim3(cc_blocks(job.real_words)), dim3(kCcThreads), 0, s, job.set.view(), job.d_insts, n,
                       job.real_words, job.base, job.d_parent, d_out, d_area);
  } else {
    rc = job.make_table(hs, false);
    if (rc) return rc;
    hipLaunchKernelGGL(cc_rank_kernel, dim3(n), dim3(kCcThreads), 0, s, job.d_comp_ptr, job.table.area, keep, job.d_thr);
    hipLaunchKernelGGL(cc_select_kernel, dim3(cc_blocks(job.words)), dim3(kCcThreads), 0, s, job.set.view(), job.d_insts, n, job.words,
                       job.base, job.d_parent, job.number, job.d_comp_ptr, job.table.area, job.d_thr, (long long)min_area, d_out,
                       d_area);
  }
  span.end(s);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(out_areas, d_area, (size_t)n * 8));
  rc = job.download_rows(hs, out_bits, d_out);
  if (rc) return rc;
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_components(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
                        long long* comp_ptr, long long* area, int* bbox, int* anchor, size_t comp_cap, size_t* n_comp, int device_id) {
  CcJob job;
  const char* who = job.who = "mnc_mask_components";
  int rc = job.prepare(bounds, offsets, bits, bytes, n, connectivity, 0, false, device_id);
  if (rc) return rc;
  MNC_REQUIRE(comp_ptr && n_comp, "%s: null output pointer", who);
  MNC_REQUIRE(!area || (bbox && anchor), "%s: null bbox or anchor", who);
  for (int i = 0; i <= n; ++i) comp_ptr[i] = 0;
  *n_comp = 0;
  if (job.words == 0) { clear_error(); return MNC_OK; }
  auto layout = [&](WsLayout l) {
    job.take(l);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  TimedSpan span(g_cc_timer);
  span.begin(hs.stream);
  rc = job.label(hs, true);
  if (rc) return rc;
  const size_t C = (size_t)job.comps;
  for (int i = 0; i <= n; ++i) comp_ptr[i] = job.comp_ptr[i];
  *n_comp = C;
  if (!area || C == 0) {
    span.end(hs.stream);
    MNC_HIP_TRY(hs.sync());
    span.keep();
    clear_error();
    return MNC_OK;
  }
  MNC_REQUIRE(comp_cap >= C, "%s: comp_cap %zu is below the %zu components of the masks", who, comp_cap, C);
  rc = job.make_table(hs, false);
  if (rc) return rc;
  span.end(hs.stream);
  MNC_HIP_TRY(hs.down(area, job.table.area, C * 8));
  MNC_HIP_TRY(hs.down(bbox, job.table.box, C * 16));
  MNC_HIP_TRY(hs.down(anchor, job.table.anchor, C * 8));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_select(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity, int min_area,
                    int keep, long long* out_areas, void* out_bits, size_t bits_cap, int device_id) {
  CcJob job;
  job.who = "mnc_mask_select";
  return cc_rewrite(job, bounds, offsets, bits, bytes, n, connectivity, false, min_area, keep, out_areas, out_bits, bits_cap, device_id);
}

// see include/mnc_hip.h
int mnc_mask_fill_holes(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity,
                        long long* out_areas, void* out_bits, size_t bits_cap, int device_id) {
  CcJob job;
  job.who = "mnc_mask_fill_holes";
  return cc_rewrite(job, bounds, offsets, bits, bytes, n, connectivity, true, 0, 0, out_areas, out_bits, bits_cap, device_id);
}

// see include/mnc_hip.h
int mnc_mask_split(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int connectivity, int* out_bounds,
                   long long* out_offsets, long long* out_areas, int* out_source, size_t comp_cap, size_t* n_comp, void* out_bits,
                   size_t bits_cap, size_t* bits_bytes, int device_id) {
  CcJob job;
  const char* who = job.who = "mnc_mask_split";
  int rc = job.prepare(bounds, offsets, bits, bytes, n, connectivity, 0, false, device_id);
  if (rc) return rc;
  MNC_REQUIRE(n_comp && bits_bytes, "%s: null size pointer", who);
  MNC_REQUIRE(!out_bits || (out_bounds && out_offsets && out_areas && out_source), "%s: null output pointer", who);
  *n_comp = 0;
  *bits_bytes = 0;
  if (job.words == 0) { clear_error(); return MNC_OK; }
  auto layout = [&](WsLayout l) {
    job.take(l);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  TimedSpan span(g_cc_timer);
  span.begin(hs.stream);
  rc = job.label(hs, true);
  if (rc) return rc;
  const size_t C = (size_t)job.comps;
  *n_comp = C;
  if (C == 0) { clear_error(); return MNC_OK; }
  rc = job.make_table(hs, true);
  if (rc) return rc;
  std::vector<long long> area(C), oword(C + 1);
  std::vector<int> box(4 * C), source(C);
  MNC_HIP_TRY(hs.down(area.data(), job.table.area, C * 8));
  MNC_HIP_TRY(hs.down(box.data(), job.table.box, C * 16));
  MNC_HIP_TRY(hs.sync());
  long long at = 0;
  for (int i = 0; i < n; ++i)
    for (long long c = job.comp_ptr[i]; c < job.comp_ptr[i + 1]; ++c) {
      source[(size_t)c] = i;
      oword[(size_t)c] = at;
      at += mask_bytes(box[4 * c + 2] - box[4 * c] + 1, box[4 * c + 3] - box[4 * c + 1] + 1) / 8;
    }
  oword[C] = at;
  *bits_bytes = (size_t)at * 8;
  if (!out_bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(at <= (1ll << 31), "%s: the result holds %lld words of rows (limit 2^31)", who, at);
  MNC_REQUIRE(comp_cap >= C && bits_cap >= (size_t)at * 8,
              "%s: comp_cap %zu or bits_cap %zu is below the %zu components and %zu bytes of the result", who, comp_cap, bits_cap, C,
              (size_t)at * 8);
  CallBuf d_out;                                         // the result's rows: known only now
  rc = d_out.alloc(who, (size_t)at * 8);
  if (rc) return rc;
  MNC_HIP_TRY(hs.up(job.d_oword, oword.data(), (C + 1) * 8));
  MNC_HIP_TRY(hs.up(job.d_source, source.data(), C * 4));
  hipLaunchKernelGGL(cc_split_kernel, dim3(cc_blocks(at)), dim3(kCcThreads), 0, hs.stream, job.set.view(), job.d_insts, job.base,
                     job.d_parent, job.table, (long long)C, job.d_oword, job.d_source, at, (u64*)d_out.p);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(out_bits, d_out.p, (size_t)at * 8));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  for (size_t c = 0; c < C; ++c) {
    for (int k = 0; k < 4; ++k) out_bounds[4 * c + k] = box[4 * c + k];
    out_offsets[c] = oword[c] * 8;
    out_areas[c] = area[c];
    out_source[c] = source[c];
  }
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_components_timing(int on, double* last_ms) { return g_cc_timer.set(on, last_ms); }
