// The contingency table of two integer label maps (include/mnc_hip.h n20), for gfx950: for every pair of values (a, b) that occurs
// at the same pixel, the number of such pixels -- what panopticapi forms with np.unique(gt * 256^3 + pred, return_counts=True) and a
// semantic evaluator with np.bincount(C * gt + pred).  The statement of the rule is mnc_amd/pairs.py:label_pairs_numpy; this file
// computes the same ids, ranks and counts exactly.  All arithmetic is integer; the only atomics are integer or (presence bits, the
// range flag) and integer add (the counts), which commute; the order of the output comes from prefix sums over the bitmap words and
// over the table's cells, never from the arrival order of an atomic: the same input gives the same bytes on every run.
//
// mnc_label_pairs, two groups of launches with one read-back of a few words between them (the host sizes the table from na and nb):
//   lb_presence_kernel   (label_bits.h, once per map) the presence bits of the values into one bitmap of 2 x 2^19 words, b's half
//                        after a's; a value outside [0, 2^24) sets no bit and joins 1 into the range flag by an integer atomicOr.
//   lb_count_kernel      (label_bits.h) the popcounts of the 2^20 words.
//   scan_launch          (scan.h, two launches) their exclusive prefix: the rank of a value of a is the prefix of its word plus the
//                        set bits below it; of b the same less na, the prefix at b's first word (tile 512 of the scan: 2^19 words are
//                        512 tiles exactly, so b's half is addressed by a Scanned whose two pointers are moved).
//   -- read back: na, na + nb, the range flag --
//   lp_count_global_kernel / lp_count_lds_kernel
//                        the two maps again, flat: a lane owns kLbRun consecutive pixels (one 16-byte load per map), joins
//                        consecutive equal pairs into runs; the lanes of a wave whose pixels continue one run join it by shuffles
//                        first, so a run costs one rank lookup and one integer atomicAdd of its length per wave it crosses.  The
//                        global plan adds into the zeroed int32 table [na][nb] in device memory (a count is at most 2^26).  The LDS
//                        plan, for tables of at most kLpLdsCells cells: a workgroup adds into a zeroed table in LDS while it
//                        grid-strides over chunks of 1024 pixels, and adds its non-zero cells to the global table once at the end.
//                        The plans give identical integers.
//   lp_nonzero_kernel    a wave per 64 cells ballots the non-zero ones and stores their number.
//   scan_launch          (two launches) the exclusive prefix of those numbers; its total is the number of pairs.
//   lp_write_kernel      the ballot again: cell c is written as (c / nb, c % nb, count) at prefix + rank among the wave's bits, into
//                        one result block packed for the m pairs there are: m, the ids, ia, ib, count.
//   lb_ids_kernel        (label_bits.h) the ids of both maps at their ranks into that block, b's after a's.
// The block comes back in one copy where the table cannot have more than kLpAtOnce pairs, else m first and then its bytes.
//
// Bound: latency -- a dozen short launches of about 5 us each and the read-back in their middle.  On the class maps of a 600 x 1000
// image (5 x 5 cells, nearly every pixel in a few of them) the counting launch takes 11 us under the LDS plan and 253 us under the
// global one, whose same-address atomics serialise; on its instance map against a shifted copy (99 x 99 cells) 14 us against 101 us;
// at 375 x 500, 9 against 71 us and 11 against 22 us: the LDS plan is kept, up to the 64 KB of one workgroup per CU.  All launches of
// a call take 126 and 154 us at 600 x 1000, 74 to 130 us at 375 x 500; the calls with their copies 0.30 and 0.34 ms, 0.19 to 0.25 ms
// (profiles/label_pairs_bench.txt).  Registers, LDS and scratch, from the code objects: lp_count_global_kernel 18 VGPRs, no LDS;
// lp_count_lds_kernel 35 VGPRs, 64 KB LDS (its grid is at most one workgroup per CU); lp_nonzero_kernel 6 VGPRs; lp_write_kernel 12
// VGPRs; the kernels of label_bits.h 6 to 12 VGPRs; no scratch in any of them.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "label_bits.h"

namespace mnc {

constexpr int kLpMaxIds = 65536;                   // distinct values of one map
constexpr long long kLpMaxCells = 1ll << 22;       // na * nb
constexpr int kLpLdsCells = 16384;                 // the LDS plan's largest table: 64 KB (mnc_amd/pairs.py LDS_CELLS)
constexpr int kLpLdsBlocks = 256;                  // its grid: at most one workgroup per CU, whatever its LDS
constexpr int kLpHead = 64;                        // ints before the ids in the result block: [0] = the number of pairs
constexpr long long kLpAtOnce = 16384;             // tables of at most this many possible pairs come back in one copy
constexpr int kLpChunk = kLbThreads * kLbRun;      // pixels of one workgroup pass
static_assert(kLbMaxWords % kScanTile == 0, "b's half of the bitmap starts on a scan tile");

// Both maps' ranks: a's bitmap and prefix, b's the same moved by 2^19 words, whose prefix counts a's na values too.
struct LpRanks {
  const unsigned *pa, *pb;
  Scanned sa, sb;
  int na, nb;
  // the cell of the pair of values (va, vb), -1 where one of them has no rank inside the table (never, after the host's checks)
  __device__ __forceinline__ int cell(int va, int vb) const {
    const int ra = lb_rank(pa, kLbMaxWords, sa, va);
    const int rb = lb_rank(pb, kLbMaxWords, sb, vb) - na;
    return ra >= 0 && ra < na && rb >= 0 && rb < nb ? ra * nb + rb : -1;
  }
};

// One pass of a workgroup over the kLpChunk pixels from its thread's p on: `table` (global or LDS) receives one atomicAdd per run
// and wave.  Every lane of the workgroup comes here.
__device__ __forceinline__ void lp_chunk(const int* __restrict__ a, const int* __restrict__ b, long long p, long long total,
                                         const LpRanks& rk, int* table) {
  const bool live = p < total;
  int va[kLbRun] = {0, 0, 0, 0}, vb[kLbRun] = {0, 0, 0, 0};
  int count = 0;
  if (live) {
    count = lb_load(a, p, total, va[0], va[1], va[2], va[3]);
    lb_load(b, p, total, vb[0], vb[1], vb[2], vb[3]);
  }
  const int lane = threadIdx.x & 63;
  // Positions are counted inside the wave's 256 pixels.  The last run of a lane is held back: a lane that is one run joins the last
  // run of the lane before it when the pair is the same, and the first lane of such a segment -- its head -- adds for all of it.
  int ra = va[0], rb = vb[0], rstart = lane * kLbRun, runs = 0;
#pragma unroll
  for (int e = 1; e < kLbRun; ++e) {
    if (e < count && (va[e] != ra || vb[e] != rb)) {
      const int c = rk.cell(ra, rb);
      if (c >= 0) atomicAdd(table + c, lane * kLbRun + e - rstart);
      ra = va[e]; rb = vb[e]; rstart = lane * kLbRun + e;
      ++runs;
    }
  }
  const int qa = __shfl_up(ra, 1), qb = __shfl_up(rb, 1), qlive = __shfl_up((int)live, 1);
  const bool joins = live && runs == 0 && lane > 0 && qlive && qa == ra && qb == rb;
  const u64 alive = __ballot(live), heads = __ballot(live && !joins);
  if (alive == 0ull) return;                               // (the whole wave)
  // the last lane of this lane's segment: the one before the next head, or the last live lane
  const u64 after = heads & ~((2ull << lane) - 1ull);
  const int last = after ? __ffsll((long long)after) - 2 : 63 - __clzll((long long)alive);
  const int rend = __shfl(lane * kLbRun + count, min(max(last, 0), 63));
  if (live && !joins) {
    const int c = rk.cell(ra, rb);
    if (c >= 0) atomicAdd(table + c, rend - rstart);
  }
}

// grid ceil(total / 1024), block 256.  table [na * nb] is zero before.
__global__ __launch_bounds__(kLbThreads) void lp_count_global_kernel(const int* __restrict__ a, const int* __restrict__ b,
                                                                     long long total, LpRanks rk, int* table) {
  lp_chunk(a, b, ((long long)blockIdx.x * kLbThreads + threadIdx.x) * kLbRun, total, rk, table);
}

// grid min(chunks, kLpLdsBlocks), block 256; cells = na * nb <= kLpLdsCells.  table [cells] is zero before.
__global__ __launch_bounds__(kLbThreads) void lp_count_lds_kernel(const int* __restrict__ a, const int* __restrict__ b, long long total,
                                                                  long long chunks, LpRanks rk, int cells, int* table) {
  __shared__ int s_table[kLpLdsCells];
  for (int c = threadIdx.x; c < cells; c += kLbThreads) s_table[c] = 0;
  __syncthreads();
  for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x)
    lp_chunk(a, b, (ch * kLbThreads + threadIdx.x) * kLbRun, total, rk, s_table);
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += kLbThreads) {
    const int v = s_table[c];
    if (v) atomicAdd(table + c, v);
  }
}

// grid ceil(cells / 256), block 256: a wave per 64 cells.  cnt [ceil(cells / 64)].
__global__ __launch_bounds__(kLbThreads) void lp_nonzero_kernel(const int* __restrict__ table, int cells, int* __restrict__ cnt) {
  const int c = blockIdx.x * kLbThreads + threadIdx.x;
  const u64 m = __ballot(c < cells && table[c] != 0);
  if ((threadIdx.x & 63) == 0 && c < cells) cnt[c >> 6] = __popcll(m);
}

// Where the pairs lie in the result block, in ints from its start, for m pairs: ia [m] at `at`, ib [m] after it, count [m] as
// 64-bit words from the next even int on.  Host and device compute it alike.
__host__ __device__ __forceinline__ long long lp_count_at(long long at, long long m) { return (at + 2 * m + 1) & ~1ll; }

// The same grid.  The non-zero cell c becomes pair pre.at(c / 64) + its rank among the wave's non-zero cells, written into the block
// packed for the m pairs there are (m is the scan's total); with more than cap pairs nothing is written: the host refuses such a
// table from m alone.  blk[0] = m.
__global__ __launch_bounds__(kLbThreads) void lp_write_kernel(const int* __restrict__ table, int cells, int nb, Scanned pre,
                                                              long long cap, long long at, int* __restrict__ blk) {
  const int c = blockIdx.x * kLbThreads + threadIdx.x, lane = threadIdx.x & 63;
  const int v = c < cells ? table[c] : 0;
  const u64 bits = __ballot(v != 0);
  const long long m = pre.tile[pre.tiles];
  if (c == 0) blk[0] = (int)m;
  if (v == 0 || m > cap) return;
  const long long k = pre.at(c >> 6) + __popcll(bits & ((1ull << lane) - 1ull));
  blk[at + k] = c / nb;
  blk[at + m + k] = c - (c / nb) * nb;
  reinterpret_cast<long long*>(blk + lp_count_at(at, m))[k] = v;
}

namespace {

CallTimer g_lp_timer;
std::atomic<int> g_lp_count_only{0};               // mnc_label_pairs_timing(2): the span is the counting launch alone
std::atomic<int> g_lp_global_only{0};              // mnc_label_pairs_plan(1): the global plan whatever the size

unsigned lp_blocks(long long units) { return (unsigned)((units + kLbThreads - 1) / kLbThreads); }

// The first value of m outside the range, for the message: the host looks only after the kernels have flagged one.
bool lp_find_bad(const int* m, int W, long long total, const char* who, const char* name) {
  for (long long p = 0; p < total; ++p)
    if (m[p] < 0 || m[p] >= kLbMaxId) {
      set_error("%s: %s[%lld][%lld]=%d not in [0, %d)", who, name, p / W, p % W, m[p], kLbMaxId);
      return true;
    }
  return false;
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_label_pairs(const int* a, const int* b, int H, int W, int cap_ids, long long cap_pairs, int* na, int* a_ids, int* nb,
                    int* b_ids, long long* n_pairs, int* ia, int* ib, long long* count, int device_id) {
  const char* who = "mnc_label_pairs";
  MNC_REQUIRE(a && b && na && nb && n_pairs, "%s: null pointer", who);
  MNC_REQUIRE(cap_ids >= 0 && cap_pairs >= 0, "%s: cap_ids=%d or cap_pairs=%lld is negative", who, cap_ids, cap_pairs);
  MNC_REQUIRE((cap_ids == 0 || (a_ids && b_ids)) && (cap_pairs == 0 || (ia && ib && count)), "%s: a null output", who);
  MNC_REQUIRE(H >= 1 && H <= kLbMaxSide && W >= 1 && W <= kLbMaxSide, "%s: H=%d or W=%d not in [1, %d]", who, H, W, kLbMaxSide);
  MNC_REQUIRE((long long)H * W <= kLbMaxPixels, "%s: %lld pixels (limit %lld)", who, (long long)H * W, kLbMaxPixels);
  const long long total = (long long)H * W;
  const int words = 2 * kLbMaxWords;
  const long long max_cells = std::min(kLpMaxCells, total * total), max_pairs = std::min(std::min(max_cells, total), cap_pairs);
  const long long max_waves = (max_cells + 63) / 64;
  int *d_a, *d_b, *d_cnt, *d_tile, *d_table, *d_pcnt, *d_ptile, *d_blk;
  unsigned *d_present, *d_bad;
  auto layout = [&](WsLayout l) {
    d_a = l.take<int>((size_t)total);
    d_b = l.take<int>((size_t)total);
    d_present = l.take<unsigned>((size_t)words);
    d_cnt = l.take<int>((size_t)words);
    d_tile = l.take<int>((size_t)scan_tiles(words) + 1);
    d_bad = l.take<unsigned>(1);                           // (after d_tile: one copy reads both back)
    d_table = l.take<int>((size_t)max_cells);
    d_pcnt = l.take<int>((size_t)max_waves);
    d_ptile = l.take<int>((size_t)scan_tiles(max_waves) + 1);
    d_blk = l.take<int>((size_t)(kLpHead + 2 * kLpMaxIds + 4 * max_pairs + 2));
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  const bool count_only = g_lp_count_only.load(std::memory_order_relaxed) != 0;
  MNC_HIP_TRY(hs.up(d_a, a, (size_t)total * sizeof(int)));
  MNC_HIP_TRY(hs.up(d_b, b, (size_t)total * sizeof(int)));
  MNC_HIP_TRY(hipMemsetAsync(d_present, 0, (size_t)words * sizeof(unsigned), hs.stream));
  MNC_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(unsigned), hs.stream));
  TimedSpan ranks(g_lp_timer), rest(g_lp_timer);
  if (!count_only) ranks.begin(hs.stream);
  const long long chunks = (total + kLpChunk - 1) / kLpChunk;
  LbSkip none;
  none.n = 0;
  for (int k = 0; k < kLbMaxSkip; ++k) none.v[k] = -1;
  hipLaunchKernelGGL(lb_presence_kernel, dim3((unsigned)chunks), dim3(kLbThreads), 0, hs.stream, d_a, total, kLbMaxWords, d_present, d_bad);
  hipLaunchKernelGGL(lb_presence_kernel, dim3((unsigned)chunks), dim3(kLbThreads), 0, hs.stream, d_b, total, kLbMaxWords,
                     d_present + kLbMaxWords, d_bad);
  hipLaunchKernelGGL(lb_count_kernel, dim3(lp_blocks(words)), dim3(kLbThreads), 0, hs.stream, d_present, words, none, d_cnt);
  const Scanned pre = scan_launch(hs.stream, d_cnt, words, d_tile);
  if (!count_only) ranks.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  // one copy from the prefix at b's first tile (na) over the total (na + nb) to the flag
  const int* d_first = d_tile + kLbMaxWords / kScanTile;
  std::vector<int> back((size_t)((const int*)d_bad - d_first) + 1);
  MNC_HIP_TRY(hs.down(back.data(), d_first, back.size() * sizeof(int)));
  MNC_HIP_TRY(hs.sync());
  const int found_a = back[0], found_ab = back[pre.tiles - kLbMaxWords / kScanTile];
  const unsigned bad = (unsigned)back.back();
  if (bad) {
    if (lp_find_bad(a, W, total, who, "a") || lp_find_bad(b, W, total, who, "b")) return MNC_ERR_INVALID;
    MNC_REQUIRE(false, "%s: a value not in [0, %d)", who, kLbMaxId);
  }
  const int found_b = found_ab - found_a;
  const long long cells = (long long)found_a * found_b;
  const int limit = std::min(cap_ids, kLpMaxIds);
  if (found_a > limit || found_b > limit || cells > kLpMaxCells) {
    *na = found_a;
    *nb = found_b;
    MNC_REQUIRE(found_a <= limit && found_b <= limit, "%s: the maps have %d and %d values (cap %d, limit %d)", who, found_a, found_b,
                cap_ids, kLpMaxIds);
    MNC_REQUIRE(false, "%s: %d x %d values are %lld cells (limit %lld)", who, found_a, found_b, cells, kLpMaxCells);
  }
  LpRanks rk;
  rk.pa = d_present;
  rk.pb = d_present + kLbMaxWords;
  rk.sa = Scanned{pre.in_tile, pre.tile, kLbMaxWords, kLbMaxWords / kScanTile};
  rk.sb = Scanned{pre.in_tile + kLbMaxWords, pre.tile + kLbMaxWords / kScanTile, kLbMaxWords, kLbMaxWords / kScanTile};
  rk.na = found_a;
  rk.nb = found_b;
  const int waves = (int)((cells + 63) / 64);
  const long long at = kLpHead + found_a + found_b;          // ints of the result block before ia
  const bool lds = cells <= kLpLdsCells && !g_lp_global_only.load(std::memory_order_relaxed);
  if (!count_only) rest.begin(hs.stream);
  MNC_HIP_TRY(hipMemsetAsync(d_table, 0, (size_t)cells * sizeof(int), hs.stream));
  if (count_only) rest.begin(hs.stream);
  if (lds)
    hipLaunchKernelGGL(lp_count_lds_kernel, dim3((unsigned)std::min<long long>(chunks, kLpLdsBlocks)), dim3(kLbThreads), 0, hs.stream,
                       d_a, d_b, total, chunks, rk, (int)cells, d_table);
  else
    hipLaunchKernelGGL(lp_count_global_kernel, dim3((unsigned)chunks), dim3(kLbThreads), 0, hs.stream, d_a, d_b, total, rk, d_table);
  if (count_only) rest.end(hs.stream);
  hipLaunchKernelGGL(lp_nonzero_kernel, dim3(lp_blocks(cells)), dim3(kLbThreads), 0, hs.stream, d_table, (int)cells, d_pcnt);
  const Scanned ppre = scan_launch(hs.stream, d_pcnt, waves, d_ptile);
  hipLaunchKernelGGL(lp_write_kernel, dim3(lp_blocks(cells)), dim3(kLbThreads), 0, hs.stream, d_table, (int)cells, found_b, ppre,
                     max_pairs, at, d_blk);
  hipLaunchKernelGGL(lb_ids_kernel, dim3(lp_blocks(words)), dim3(kLbThreads), 0, hs.stream, d_present, words, pre, 2 * kLpMaxIds,
                     d_blk + kLpHead);
  if (!count_only) rest.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  // The block: kLpHead ints of which the first is m, the ids of a and of b, then ia, ib and count packed for m pairs.  A table that
  // cannot have many pairs comes back whole in one copy; of any other m comes first, then exactly the block's bytes.
  const long long most = std::min(cells, max_pairs);
  auto block_ints = [&](long long pairs) { return (size_t)(lp_count_at(at, pairs) + 2 * pairs); };
  std::vector<int> blk(most <= kLpAtOnce ? block_ints(most) : (size_t)1);
  MNC_HIP_TRY(hs.down(blk.data(), d_blk, blk.size() * sizeof(int)));
  MNC_HIP_TRY(hs.sync());
  const int m = blk[0];
  if (m > cap_pairs) {
    *na = found_a;
    *nb = found_b;
    *n_pairs = m;
    MNC_REQUIRE(false, "%s: the maps have %d pairs (cap %lld)", who, m, cap_pairs);
  }
  if (most > kLpAtOnce) {
    blk.resize(block_ints(m));
    MNC_HIP_TRY(hs.down(blk.data(), d_blk, blk.size() * sizeof(int)));
    MNC_HIP_TRY(hs.sync());
  }
  std::copy(blk.begin() + kLpHead, blk.begin() + kLpHead + found_a, a_ids);
  for (int k = 0; k < found_b; ++k) b_ids[k] = blk[(size_t)kLpHead + found_a + k] - kLbMaxId;    // (b's bits lie 2^24 values after a's)
  std::copy(blk.begin() + at, blk.begin() + at + m, ia);
  std::copy(blk.begin() + at + m, blk.begin() + at + 2 * (long long)m, ib);
  if (m) memcpy(count, blk.data() + lp_count_at(at, m), (size_t)m * sizeof(long long));
  if (count_only) rest.keep(); else rest.keep_sum(ranks);
  *na = found_a;
  *nb = found_b;
  *n_pairs = m;
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_label_pairs_plan(int plan) {
  MNC_REQUIRE(plan == 0 || plan == 1, "mnc_label_pairs_plan: plan=%d is not 0 or 1", plan);
  g_lp_global_only.store(plan);
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_label_pairs_timing(int on, double* last_ms) {
  g_lp_count_only.store(on == 2 ? 1 : 0);
  return g_lp_timer.set(on, last_ms);
}
