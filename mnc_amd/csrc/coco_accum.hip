// COCO's accumulate -- the per-image match tables of a whole set turned into precision [T][R][K][A][M] and recall [T][K][A][M]
// (the published cocoeval.py:accumulate) -- in one call, for gfx950 (include/mnc_hip.h n10).  The statement of the rule is
// mnc_amd/coco_eval.py:accumulate; this file computes the same tables bit for bit: every quantity is an integer count or one IEEE
// double division.
//
//   accum_keys_kernel       one thread per detection: key = (class index, -1 as K) << 32 | the order-preserving transform of
//                           -score that mv.hip makes (-0.0 as +0.0), value = the detection's index.
//   accum_hist_kernel       one workgroup per sort tile of kAccumSortTile keys: the tile's histogram of one 8-bit digit (integer
//   accum_hist_scan_kernel  LDS atomics: a sum), stored digit-major; one workgroup per digit scans its row of tile counts;
//   accum_scatter_kernel    one workgroup per tile scans the 256 digit totals again (cheaper than a launch), ranks its keys
//                           and scatters them.  A key's rank within its tile is stable by construction: every wave owns a
//                           contiguous quarter of the tile and takes it in rounds of 64 keys -- wave ballots give the lanes that
//                           hold the same digit, the popcount of the lower ones is the rank within the round, a per-wave LDS
//                           counter carries the rounds, and the waves' counters are summed in wave order.  No atomic's arrival
//                           order is ever a rank.
//                           ceil((32 + bits of K) / 8) passes, least significant digit first: equal (class, score) keep the
//                           input order, which is (image, index) -- the tie rule of np.argsort(kind="mergesort").
//   accum_segments_kernel   the class segment starts from the sorted keys: thread i stores i for every class between its left
//                           neighbour's and its own.  No atomics.
//   accum_npig_kernel       npig[k][a] by integer atomic adds (a sum).
//   accum_gather_kernel     the flag planes into sorted order, once; and per detection one byte whose bit m is rank < max_dets[m]
//                           (M <= 8), so that a cell reads two contiguous bytes an element.
//   accum_cells_kernel      one workgroup per (k, a, m, t).  tp is non-decreasing and x -> (double)x / (double)npig is monotone,
//                           so "the first i with rc_i >= rec_thrs[r]" is "the first i with tp_i >= need_r", need_r the least
//                           count c with (double)c / (double)npig >= rec_thrs[r] -- found per threshold by bisection on exactly
//                           that comparison, each threshold by itself (no sorted thresholds assumed).  The forward pass over the
//                           class segment then only has to count (tp and fp totals -> recall); the backward pass walks the
//                           chunks of kAccumScanChunk elements from the right with the carried suffix counts and the carried
//                           maximum of pr, rebuilds tp_j / fp_j = totals - suffix counts, forms pr_j = tp_j / ((fp_j + tp_j) +
//                           2^-52), scans the maximum from the right within the chunk, and every threshold whose need_r falls
//                           into the chunk's range of tp bisects the chunk's tp_j in LDS and takes the maximum there.  A
//                           detection at or above max_dets[m] counts as neither tp nor fp: it repeats its left neighbour's pr
//                           (or 0 in front), which changes no maximum, so the list of a smaller max_det needs no compaction.
//                           No per-element intermediate leaves the workgroup.
// No floating-point atomics; integer atomics only where the result is a sum.  The same input gives the same bits from run to run.
//
// Bound: the sort is HBM-bound in principle (12 bytes a key read twice and written once a pass) and launch-bound at the sizes of
// a dataset (5 10^5 keys: 3 launches a pass).  The cells are latency-bound: A * M * T walks of every class segment, two bytes an
// element from L2, one double division an element.
//
// Compiled with -ffp-contract=off as mask_match.hip is.
#include <cmath>
#include <vector>

#include "mnc_internal.h"
#include "scan.h"

namespace mnc {

typedef unsigned long long u64;

constexpr int kAccumThreads = 256;
constexpr int kAccumWaves = kAccumThreads / 64;
constexpr int kAccumSortItems = 8;                                 // keys of one thread, one of each round of its wave
constexpr int kAccumSortTile = 2048;                               // = kAccumThreads * kAccumSortItems keys of one workgroup
constexpr int kAccumScanItems = 4;
constexpr int kAccumScanChunk = 1024;                              // = kAccumThreads * kAccumScanItems elements of one step of a cell
constexpr int kAccumMaxN = 1 << 24;
constexpr int kAccumMaxK = 4096;
constexpr int kAccumMaxT = 16;
constexpr int kAccumMaxA = 8;
constexpr int kAccumMaxM = 8;
constexpr int kAccumMaxR = 1024;
constexpr int kAccumMaxDet = 2048;
static_assert(kAccumSortTile == kAccumThreads * kAccumSortItems && kAccumScanChunk == kAccumThreads * kAccumScanItems, "tile sizes");

// grid ceil(N / 256), block 256.
__global__ __launch_bounds__(kAccumThreads) void accum_keys_kernel(const int* __restrict__ cls, const float* __restrict__ score, int N,
                                                                   int K, u64* __restrict__ keys, unsigned* __restrict__ vals) {
  const int i = blockIdx.x * kAccumThreads + threadIdx.x;
  if (i >= N) return;
  const int c = cls[i];
  const float v = -score[i] + 0.0f;                                // -0.0 -> +0.0; a NaN was refused by the host
  const unsigned u = __float_as_uint(v);
  const unsigned o = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);  // ascending in -score
  keys[i] = ((u64)(unsigned)(c < 0 ? K : c) << 32) | o;
  vals[i] = (unsigned)i;
}

__device__ __forceinline__ int accum_digit(u64 key, int shift) { return (int)((key >> shift) & 255u); }

// grid tiles, block 256.  hist [256][tiles].
__global__ __launch_bounds__(kAccumThreads) void accum_hist_kernel(const u64* __restrict__ keys, int N, int shift, int tiles,
                                                                   unsigned* __restrict__ hist) {
  __shared__ unsigned s_hist[256];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * kAccumSortTile;
#pragma unroll
  for (int it = 0; it < kAccumSortItems; ++it) {
    const int i = base + it * kAccumThreads + threadIdx.x;
    if (i < N) atomicAdd(&s_hist[accum_digit(keys[i], shift)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * tiles + blockIdx.x] = s_hist[threadIdx.x];
}

// The exclusive scan of one value a thread over the workgroup's 256 threads; *total = the sum.  s_w: kAccumWaves words of LDS.
__device__ __forceinline__ unsigned accum_block_excl_scan(unsigned v, unsigned* s_w, unsigned* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned incl = wave_incl_scan(v, lane);
  __syncthreads();                                                 // s_w may still be read from the call before
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  unsigned before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kAccumWaves; ++w) {
    const unsigned c = s_w[w];
    before += w < wave ? c : 0u;
    sum += c;
  }
  *total = sum;
  return before + incl - v;
}

// grid 256 (one digit each), block 256.  hist [256][tiles] -> its rows' exclusive scans in place; totals [256].
__global__ __launch_bounds__(kAccumThreads) void accum_hist_scan_kernel(unsigned* __restrict__ hist, int tiles,
                                                                        unsigned* __restrict__ totals) {
  __shared__ unsigned s_w[kAccumWaves];
  unsigned* row = hist + (size_t)blockIdx.x * tiles;
  unsigned carry = 0;
  for (int t0 = 0; t0 < tiles; t0 += kAccumThreads) {
    const int t = t0 + threadIdx.x;
    const unsigned v = t < tiles ? row[t] : 0u;
    unsigned sum;
    const unsigned ex = accum_block_excl_scan(v, s_w, &sum);
    if (t < tiles) row[t] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// grid tiles, block 256.  Wave w owns keys [512 w, 512 w + 512) of the tile, round `it` of it the 64 keys from 64 it on: tile
// order is (wave, round, lane).  hist holds the exclusive scans of accum_hist_scan_kernel, totals the digits' counts.
__global__ __launch_bounds__(kAccumThreads) void accum_scatter_kernel(const u64* __restrict__ keys, const unsigned* __restrict__ vals,
                                                                      int N, int shift, int tiles, const unsigned* __restrict__ hist,
                                                                      const unsigned* __restrict__ totals, u64* __restrict__ keys_out,
                                                                      unsigned* __restrict__ vals_out) {
  __shared__ unsigned s_w[kAccumWaves];
  __shared__ unsigned s_base[256];                                 // where the tile's keys of a digit begin in the output
  __shared__ unsigned s_cnt[kAccumWaves][256];                     // per wave and digit: the keys seen so far; then the waves before
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    unsigned sum;
    const unsigned below = accum_block_excl_scan(totals[threadIdx.x], s_w, &sum);      // keys of a smaller digit, all tiles
    s_base[threadIdx.x] = below + hist[(size_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kAccumWaves; ++w) s_cnt[w][threadIdx.x] = 0;
  }
  __syncthreads();
  volatile unsigned* cnt = s_cnt[wave];
  const int base = blockIdx.x * kAccumSortTile + wave * (64 * kAccumSortItems);
  u64 key[kAccumSortItems];
  unsigned val[kAccumSortItems], rank[kAccumSortItems];
#pragma unroll
  for (int it = 0; it < kAccumSortItems; ++it) {
    const int i = base + it * 64 + lane;
    const bool valid = i < N;
    key[it] = valid ? keys[i] : 0ull;
    val[it] = valid ? vals[i] : 0u;
    const int d = accum_digit(key[it], shift);
    u64 same = __ballot(valid);                                    // -> the valid lanes of this round with the digit d
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const u64 m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    const unsigned seen = valid ? cnt[d] : 0u;
    rank[it] = seen + (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    __builtin_amdgcn_wave_barrier();
    if (valid && (same >> lane) == 1ull) cnt[d] = seen + (unsigned)__popcll(same);    // the highest lane of the group, alone
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    unsigned run = 0;                                              // thread d: the waves' counts of digit d, summed in wave order
#pragma unroll
    for (int w = 0; w < kAccumWaves; ++w) {
      const unsigned c = s_cnt[w][threadIdx.x];
      s_cnt[w][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kAccumSortItems; ++it) {
    const int i = base + it * 64 + lane;
    if (i < N) {
      const int d = accum_digit(key[it], shift);
      const unsigned pos = s_base[d] + s_cnt[wave][d] + rank[it];
      if (pos < (unsigned)N) {                                     // (always: the histogram counted these keys)
        keys_out[pos] = key[it];
        vals_out[pos] = val[it];
      }
    }
  }
}

// grid ceil((N + 1) / 256), block 256.  seg [K + 1]: where class k begins in the sorted order; seg[K] = the end of the evaluated.
__global__ __launch_bounds__(kAccumThreads) void accum_segments_kernel(const u64* __restrict__ keys, int N, int K, int* __restrict__ seg) {
  const int i = blockIdx.x * kAccumThreads + threadIdx.x;
  if (i > N) return;
  const int lo = i == 0 ? 0 : (int)(keys[i - 1] >> 32) + 1;
  const int hi = i == N ? K : min((int)(keys[i] >> 32), K);
  for (int c = lo; c <= hi; ++c) seg[c] = i;
}

// grid ceil(A * Gn / 256), block 256.  npig [K][A], zero before the launch.
__global__ __launch_bounds__(kAccumThreads) void accum_npig_kernel(const int* __restrict__ gcls, const unsigned char* __restrict__ gig,
                                                                   int Gn, int A, u64* __restrict__ npig) {
  const long long p = (long long)blockIdx.x * kAccumThreads + threadIdx.x;
  if (p >= (long long)A * Gn) return;
  const int a = (int)(p / Gn), g = (int)(p % Gn);
  const int c = gcls[g];
  if (c >= 0 && gig[p] == 0) atomicAdd(&npig[(size_t)c * A + a], 1ull);
}

struct AccumMaxDets { int v[kAccumMaxM]; };

// grid (ceil(N / 256), A * T + 1), block 256.  Row y < A * T: flag plane y into sorted order; the last row: the max_det bits.
__global__ __launch_bounds__(kAccumThreads) void accum_gather_kernel(const unsigned* __restrict__ perm, const unsigned char* __restrict__ flags,
                                                                     const int* __restrict__ rank, int N, int planes, int M,
                                                                     AccumMaxDets md, unsigned char* __restrict__ sflags,
                                                                     unsigned char* __restrict__ sbits) {
  const int p = blockIdx.x * kAccumThreads + threadIdx.x;
  if (p >= N) return;
  const unsigned src = perm[p];
  if (src >= (unsigned)N) return;                                  // (never: perm is a permutation)
  const int y = blockIdx.y;
  if (y < planes) {
    sflags[(size_t)y * N + p] = flags[(size_t)y * N + src];
  } else {
    const int r = rank[src];
    unsigned bits = 0;
#pragma unroll
    for (int m = 0; m < kAccumMaxM; ++m) bits |= (m < M && r < md.v[m]) ? 1u << m : 0u;
    sbits[p] = (unsigned char)bits;
  }
}

__device__ __forceinline__ double accum_wave_suffix_max(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double down = __shfl_down(v, o);
    if (lane + o < 64) v = fmax(v, down);
  }
  return v;
}

// grid K * A * M * T (t fastest, then m, a, k), block 256.
__global__ __launch_bounds__(kAccumThreads) void accum_cells_kernel(const unsigned char* __restrict__ sflags, const unsigned char* __restrict__ sbits,
                                                                    const int* __restrict__ seg, const u64* __restrict__ npig,
                                                                    const double* __restrict__ rec_thrs, int N, int K, int T, int A, int M,
                                                                    int R, double* __restrict__ precision, double* __restrict__ recall) {
  __shared__ unsigned s_w[kAccumWaves];
  __shared__ double s_wmax[kAccumWaves];
  __shared__ int s_need[kAccumMaxR];
  __shared__ double s_q[kAccumMaxR];
  __shared__ int s_tp[kAccumScanChunk];
  __shared__ double s_max[kAccumScanChunk];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int cell = blockIdx.x;
  const int t = cell % T; cell /= T;
  const int m = cell % M; cell /= M;
  const int a = cell % A;
  const int k = cell / A;
  double* prec = precision + (((size_t)t * R * K + k) * A + a) * M + m;        // + r * K * A * M
  const size_t pstride = (size_t)K * A * M;
  double* rec = recall + (((size_t)t * K + k) * A + a) * M + m;
  const u64 np = npig[(size_t)k * A + a];
  if (np == 0) {
    for (int r = tid; r < R; r += kAccumThreads) prec[r * pstride] = -1.0;
    if (tid == 0) *rec = -1.0;
    return;
  }
  const double dnp = (double)np;
  const int s0 = seg[k], len = seg[k + 1] - s0;
  const unsigned char* fl = sflags + (size_t)(a * T + t) * N + s0;
  const unsigned char* mb = sbits + s0;
  // forward: the totals
  unsigned mine = 0, mine_fp = 0;
  for (int j = tid; j < len; j += kAccumThreads) {
    const bool in = (mb[j] >> m) & 1;
    const unsigned f = fl[j];
    mine += (in && f == 1u) ? 1u : 0u;
    mine_fp += (in && f == 0u) ? 1u : 0u;
  }
  unsigned tp_total, fp_total;
  (void)accum_block_excl_scan(mine, s_w, &tp_total);
  (void)accum_block_excl_scan(mine_fp, s_w, &fp_total);
  if (tid == 0) *rec = (double)tp_total / dnp;                     // 0 tp (no detection among them) gives 0.0
  // the least count that reaches each threshold; tp_total + 1: none does
  for (int r = tid; r < R; r += kAccumThreads) {
    const double thr = rec_thrs[r];
    unsigned lo = 0, hi = tp_total + 1u;
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      if ((double)mid / dnp >= thr) hi = mid; else lo = mid + 1u;
    }
    s_need[r] = (int)lo;
    s_q[r] = 0.0;
  }
  // backward
  unsigned tp_after = tp_total, fp_after = fp_total;               // the counts up to and including the chunk's last element
  double carry = 0.0;                                              // the maximum of pr to the right of the chunk (pr >= 0)
  const int chunks = (len + kAccumScanChunk - 1) / kAccumScanChunk;
  for (int c = chunks - 1; c >= 0; --c) {
    const int c0 = c * kAccumScanChunk, cn = min(len - c0, kAccumScanChunk);
    unsigned tpb[kAccumScanItems], fpb[kAccumScanItems];
    unsigned packed = 0;                                           // tp | fp << 16 of the thread's elements (<= 4 each)
#pragma unroll
    for (int i = 0; i < kAccumScanItems; ++i) {
      const int j = tid * kAccumScanItems + i;
      const bool valid = j < cn;
      const bool in = valid && ((mb[c0 + (valid ? j : 0)] >> m) & 1);
      const unsigned f = valid ? fl[c0 + j] : 2u;
      tpb[i] = (in && f == 1u) ? 1u : 0u;
      fpb[i] = (in && f == 0u) ? 1u : 0u;
      packed += tpb[i] + (fpb[i] << 16);
    }
    unsigned sum;
    const unsigned ex = accum_block_excl_scan(packed, s_w, &sum);  // <= 1024 in either half
    const unsigned tp_before = tp_after - (sum & 0xFFFFu), fp_before = fp_after - (sum >> 16);
    unsigned tp = tp_before + (ex & 0xFFFFu), fp = fp_before + (ex >> 16);
    double pr[kAccumScanItems];
#pragma unroll
    for (int i = 0; i < kAccumScanItems; ++i) {
      tp += tpb[i];
      fp += fpb[i];
      const int j = tid * kAccumScanItems + i;
      s_tp[j] = (int)tp;                                           // past cn: tp_after, the row stays non-decreasing
      pr[i] = j < cn ? (double)tp / ((double)(fp + tp) + 2.220446049250313e-16) : 0.0;
    }
#pragma unroll
    for (int i = kAccumScanItems - 2; i >= 0; --i) pr[i] = fmax(pr[i], pr[i + 1]);
    const double incl = accum_wave_suffix_max(pr[0], lane);        // this thread's elements and those of the higher lanes
    const double next = __shfl_down(incl, 1);
    if (lane == 0) s_wmax[wave] = incl;
    __syncthreads();
    double right = carry, all = carry;                             // right: everything after this thread's elements
#pragma unroll
    for (int w = 0; w < kAccumWaves; ++w) {
      const double v = s_wmax[w];
      right = w > wave ? fmax(right, v) : right;
      all = fmax(all, v);
    }
    if (lane < 63) right = fmax(right, next);
#pragma unroll
    for (int i = 0; i < kAccumScanItems; ++i) s_max[tid * kAccumScanItems + i] = fmax(pr[i], right);
    __syncthreads();
    for (int r = tid; r < R; r += kAccumThreads) {
      const unsigned need = (unsigned)s_need[r];
      int at = -1;
      if (need == 0u) {
        at = c == 0 ? 0 : -1;                                      // rc_0 >= the threshold already
      } else if (need > tp_before && need <= tp_after) {
        int lo = 0, hi = cn - 1;                                   // s_tp[cn - 1] = tp_after >= need
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if ((unsigned)s_tp[mid] >= need) hi = mid; else lo = mid + 1;
        }
        at = lo;
      }
      if (at >= 0) s_q[r] = s_max[at];
    }
    carry = all;
    tp_after = tp_before;
    fp_after = fp_before;
    __syncthreads();                                               // s_tp, s_max and s_wmax are written again
  }
  __syncthreads();
  for (int r = tid; r < R; r += kAccumThreads) prec[r * pstride] = s_q[r];
}

namespace {

// mnc_coco_accum_timing: a HIP event pair around the launches of the next calls (tools/coco_accum_bench.py)
CallTimer g_accum_timer;

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_coco_accumulate(const int* dt_class_idx, const float* dt_score, const int* dt_rank, const unsigned char* dt_flags, int N,
                        const int* gt_class_idx, const unsigned char* gt_ignore, int Gn, int K, int T, int A, const int* max_dets, int M,
                        const double* rec_thrs, int R, double* precision, double* recall, long long* npig, int device_id) {
  const char* who = "mnc_coco_accumulate";
  MNC_REQUIRE(N >= 0 && N <= kAccumMaxN, "%s: N=%d not in [0, 2^24]", who, N);
  MNC_REQUIRE(Gn >= 0 && Gn <= kAccumMaxN, "%s: Gn=%d not in [0, 2^24]", who, Gn);
  MNC_REQUIRE(K >= 1 && K <= kAccumMaxK, "%s: K=%d not in [1, %d]", who, K, kAccumMaxK);
  MNC_REQUIRE(T >= 1 && T <= kAccumMaxT, "%s: T=%d not in [1, %d]", who, T, kAccumMaxT);
  MNC_REQUIRE(A >= 1 && A <= kAccumMaxA, "%s: A=%d not in [1, %d]", who, A, kAccumMaxA);
  MNC_REQUIRE(M >= 1 && M <= kAccumMaxM, "%s: M=%d not in [1, %d]", who, M, kAccumMaxM);
  MNC_REQUIRE(R >= 1 && R <= kAccumMaxR, "%s: R=%d not in [1, %d]", who, R, kAccumMaxR);
  MNC_REQUIRE(precision && recall, "%s: null precision or recall", who);
  MNC_REQUIRE(max_dets && rec_thrs, "%s: null max_dets or rec_thrs", who);
  MNC_REQUIRE(N == 0 || (dt_class_idx && dt_score && dt_rank && dt_flags), "%s: null table of the detections", who);
  MNC_REQUIRE(Gn == 0 || (gt_class_idx && gt_ignore), "%s: null table of the ground truths", who);
  AccumMaxDets md = {};
  for (int m = 0; m < M; ++m) {
    MNC_REQUIRE(max_dets[m] >= 1 && max_dets[m] <= kAccumMaxDet, "%s: max_dets[%d]=%d not in [1, %d]", who, m, max_dets[m], kAccumMaxDet);
    md.v[m] = max_dets[m];
  }
  for (int r = 0; r < R; ++r) MNC_REQUIRE(!std::isnan(rec_thrs[r]), "%s: recall threshold %d is NaN", who, r);
  for (int i = 0; i < N; ++i) {
    MNC_REQUIRE(dt_class_idx[i] >= -1 && dt_class_idx[i] < K, "%s: class index %d of detection %d not in [-1, %d)", who, dt_class_idx[i], i, K);
    MNC_REQUIRE(dt_rank[i] >= 0, "%s: rank %d of detection %d is negative", who, dt_rank[i], i);
    MNC_REQUIRE(!std::isnan(dt_score[i]), "%s: score %d is NaN", who, i);
  }
  const size_t planes = (size_t)A * T, nflags = planes * (size_t)N, ngig = (size_t)A * Gn;
  {
    unsigned char top = 0;
    for (size_t i = 0; i < nflags; ++i) top = dt_flags[i] > top ? dt_flags[i] : top;
    MNC_REQUIRE(top <= 3, "%s: a flag byte of %d (bit 0 matched, bit 1 ignored; nothing above 3)", who, (int)top);
    top = 0;
    for (size_t i = 0; i < ngig; ++i) top = gt_ignore[i] > top ? gt_ignore[i] : top;
    MNC_REQUIRE(top <= 1, "%s: an ignore byte of %d is not 0 / 1", who, (int)top);
  }
  for (int g = 0; g < Gn; ++g)
    MNC_REQUIRE(gt_class_idx[g] >= -1 && gt_class_idx[g] < K, "%s: class index %d of ground truth %d not in [-1, %d)", who, gt_class_idx[g], g, K);
  const size_t cells = (size_t)K * A * M, nrec = cells * T, nprec = nrec * R;
  if (N == 0 || Gn == 0) {
    // nothing to sort: a cell without a not-ignored ground truth stays -1, every other one has an empty list
    std::vector<long long> count((size_t)K * A, 0);
    for (int a = 0; a < A; ++a)
      for (int g = 0; g < Gn; ++g)
        if (gt_class_idx[g] >= 0 && !gt_ignore[(size_t)a * Gn + g]) ++count[(size_t)gt_class_idx[g] * A + a];
    for (size_t i = 0; i < nrec; ++i) recall[i] = count[(i / M) % ((size_t)K * A)] ? 0.0 : -1.0;
    for (size_t i = 0; i < nprec; ++i) precision[i] = count[(i / M) % ((size_t)K * A)] ? 0.0 : -1.0;
    if (npig) for (size_t i = 0; i < (size_t)K * A; ++i) npig[i] = count[i];
    clear_error();
    return MNC_OK;
  }
  const int tiles = cdiv(N, kAccumSortTile);
  int class_bits = 0;
  while ((K >> class_bits) != 0) ++class_bits;                     // the class field holds 0 .. K
  const int passes = (32 + class_bits + 7) / 8;
  int *d_cls, *d_rank, *d_gcls, *d_seg;
  float* d_score;
  unsigned char *d_flags, *d_gig, *d_sflags, *d_sbits;
  double *d_thrs, *d_prec, *d_rec;
  u64 *d_keys[2], *d_npig;
  unsigned *d_vals[2], *d_hist, *d_totals;
  auto layout = [&](WsLayout l) {
    d_cls = l.take<int>(N);
    d_score = l.take<float>(N);
    d_rank = l.take<int>(N);
    d_flags = l.take<unsigned char>(nflags);
    d_gcls = l.take<int>(Gn);
    d_gig = l.take<unsigned char>(ngig);
    d_thrs = l.take<double>(R);
    d_keys[0] = l.take<u64>(N);
    d_keys[1] = l.take<u64>(N);
    d_vals[0] = l.take<unsigned>(N);
    d_vals[1] = l.take<unsigned>(N);
    d_hist = l.take<unsigned>((size_t)256 * tiles);
    d_totals = l.take<unsigned>(256);
    d_seg = l.take<int>((size_t)K + 1);
    d_npig = l.take<u64>((size_t)K * A);
    d_sflags = l.take<unsigned char>(nflags);
    d_sbits = l.take<unsigned char>(N);
    d_prec = l.take<double>(nprec);
    d_rec = l.take<double>(nrec);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  hipStream_t s = hs.stream;
  MNC_HIP_TRY(hs.up(d_cls, dt_class_idx, (size_t)N * 4));
  MNC_HIP_TRY(hs.up(d_score, dt_score, (size_t)N * 4));
  MNC_HIP_TRY(hs.up(d_rank, dt_rank, (size_t)N * 4));
  MNC_HIP_TRY(hs.up(d_flags, dt_flags, nflags));
  MNC_HIP_TRY(hs.up(d_gcls, gt_class_idx, (size_t)Gn * 4));
  MNC_HIP_TRY(hs.up(d_gig, gt_ignore, ngig));
  MNC_HIP_TRY(hs.up(d_thrs, rec_thrs, (size_t)R * 8));
  TimedSpan span(g_accum_timer);
  span.begin(s);
  MNC_HIP_TRY(hipMemsetAsync(d_npig, 0, (size_t)K * A * 8, s));
  const dim3 block(kAccumThreads);
  hipLaunchKernelGGL(accum_keys_kernel, dim3(cdiv(N, kAccumThreads)), block, 0, s, d_cls, d_score, N, K, d_keys[0], d_vals[0]);
  int cur = 0;
  for (int p = 0; p < passes; ++p, cur ^= 1) {
    hipLaunchKernelGGL(accum_hist_kernel, dim3(tiles), block, 0, s, d_keys[cur], N, 8 * p, tiles, d_hist);
    hipLaunchKernelGGL(accum_hist_scan_kernel, dim3(256), block, 0, s, d_hist, tiles, d_totals);
    hipLaunchKernelGGL(accum_scatter_kernel, dim3(tiles), block, 0, s, d_keys[cur], d_vals[cur], N, 8 * p, tiles, d_hist, d_totals,
                       d_keys[cur ^ 1], d_vals[cur ^ 1]);
  }
  hipLaunchKernelGGL(accum_segments_kernel, dim3(cdiv(N + 1, kAccumThreads)), block, 0, s, d_keys[cur], N, K, d_seg);
  hipLaunchKernelGGL(accum_npig_kernel, dim3((unsigned)((ngig + kAccumThreads - 1) / kAccumThreads)), block, 0, s, d_gcls, d_gig, Gn, A,
                     d_npig);
  hipLaunchKernelGGL(accum_gather_kernel, dim3(cdiv(N, kAccumThreads), (unsigned)planes + 1), block, 0, s, d_vals[cur], d_flags, d_rank,
                     N, (int)planes, M, md, d_sflags, d_sbits);
  hipLaunchKernelGGL(accum_cells_kernel, dim3((unsigned)(cells * T)), block, 0, s, d_sflags, d_sbits, d_seg, d_npig, d_thrs, N, K, T, A,
                     M, R, d_prec, d_rec);
  span.end(s);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(precision, d_prec, nprec * 8));
  MNC_HIP_TRY(hs.down(recall, d_rec, nrec * 8));
  if (npig) MNC_HIP_TRY(hs.down(npig, d_npig, (size_t)K * A * 8));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_coco_accum_timing(int on, double* last_ms) { return g_accum_timer.set(on, last_ms); }
