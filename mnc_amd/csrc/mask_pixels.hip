// Pixel statistics and histograms of an image under packed instance masks (include/mnc_hip.h n21), for gfx950, on the PackedMasks
// layout of inst_masks.hip (n5), without unpacking a mask: per instance and channel the count, the sums of v, v^2, x v and y v, the
// least and the greatest value with the position of each, and the histogram of the values.  The statements of the rules are
// mnc_amd/pixels.py:pixel_stats_numpy and histogram_numpy; this file computes the same integers.  There is no floating point.
//
// Both kernels share one walk.  An instance's words are those of its rows and word columns that meet the image, numbered in raster
// order.  A wave owns a run of them (kMpWaveWords; kMhShortRun or kMhLongRun): lane t loads word t of the run once, ANDs it with the
// row's valid columns (padding bits are not trusted) and with the image frame, and the wave then visits the words one after the
// other by a lane read; a word without a bit costs a scalar test and no image access.  In a visited word lane b owns bit b: the 64
// lanes read 64 consecutive pixels of one image row, C values each -- one contiguous stretch of 64 C elements (192 bytes of uint8
// RGB).
//
//   mp_range_kernel     int32 images only: every value of the image against [-2^18, 2^18]; a wave that sees an offender ORs 1 into
//                       a flag word, which the host reads before it writes anything.
//   mp_stats_kernel<T>  a tile of T = 1, 3 or 4 channels (grid z: the tiles of one launch), the per-lane figures in registers: four
//                       64-bit sums and two 64-bit keys per channel.  A key is (value + 2^31) << 32 | position, position = y << 16 |
//                       x for the least value and its complement for the greatest, so that an unsigned minimum resp. maximum of keys
//                       is the extreme value at its lowest (y, x).  After the run: shuffles within the wave, LDS within the
//                       workgroup, one 64-bit atomicAdd / atomicMin / atomicMax per workgroup and figure.  C = 4 q + r channels
//                       take one launch of q tiles of 4 and one of the rest (r = 3: one tile of 3; r = 2: two tiles of 1).
//   mp_hist_kernel      a group of channels whose cells (channels x bins) fit kMhCells uint32 cells of LDS (grid z: the groups).
//                       A lane adds 1 to its cell by an integer LDS atomic -- after the lanes that share the cell of the wave's
//                       first live lane have been counted by a ballot and added at once, so that a constant region costs one LDS
//                       atomic per word and channel, not 64 on one address.  At the end the workgroup adds its non-zero cells to
//                       the zeroed int64 table by 64-bit atomicAdd.
// 1 or 2 launches for the statistics, 1 for the histogram, 1 more for an int32 image, whatever the data.  Every atomic is an integer
// add, minimum or maximum, which commute: the same input gives the same bytes on every run.
//
// Bound: launch and copy latency.  Measured at 100 instances of a 600 x 1000 uint8 RGB image (573 x 10^3 set pixels; 3.3 MB to read:
// the image bytes of the instances' frames plus their words), kernels alone: the statistics 26 us of a 0.14 ms call, the histogram
// of 256 bins 33 us of a 0.21 ms call -- 129 and 102 GB/s of the bytes they must read, far below what HBM gives: a few thousand
// short waves that wait on their own loads, not a stream.  The upload of the 1.8 MB image alone is 0.042 ms, 29 % and 20 % of the
// calls.  At 375 x 500 (445 x 10^3 pixels, 2.4 MB): 20 us of 0.12 ms and 27 us of 0.18 ms, the upload 0.029 ms.  The loop over
// full(i, H, W) of the same run takes 51.8 and 34.4 ms, 28.3 and 14.9 ms: the calls are 362, 166, 244 and 82 times faster
// (profiles/pixel_stats_bench.txt).  Registers, LDS and scratch, from the code object: mp_stats_kernel<4> 119 VGPRs and 800 bytes,
// <3> 91 and 608, <1> 42 and 224; mp_hist_kernel 24 VGPRs and 4 bytes of dynamic LDS per cell; mp_range_kernel 6 VGPRs; no scratch
// in any of them.
#include <climits>
#include <vector>

#include "mask_set.h"

namespace mnc {

constexpr int kMpThreads = 256;
constexpr int kMpWaves = kMpThreads / 64;
constexpr int kMpWaveWords = 16;                         // words of one wave of the statistics, visited in steps of kMpStep
constexpr int kMpStep = 4;                               // words whose image reads are in flight together
constexpr int kMpBlockWords = kMpWaves * kMpWaveWords;
constexpr int kMhShortRun = 16;                          // words of one wave of the histogram: tables of at most kMhSmallTable cells,
constexpr int kMhLongRun = 64;                           // and larger ones, whose zeroing and flushing want more words to pay for them
constexpr int kMhSmallTable = 2048;
constexpr int kMhStep = 4;                               // channels whose image reads are in flight together
constexpr int kMhCells = 16384;                          // uint32 cells of one workgroup: 64 KB, label_pairs.hip's table
constexpr int kMpMaxN = 2048;                            // instances of one call (mnc_mask_moments' limit)
constexpr int kMpMaxExtent = 32768;                      // columns or rows of one bound (mnc_mask_moments' limit)
constexpr int kMpMaxSide = 32768;                        // of the image
constexpr long long kMpMaxPixels = 1ll << 26;            // of the image
constexpr int kMpMaxChannels = 32;
constexpr int kMpMaxValue = 1 << 18;                     // |value| of an int32 image
constexpr int kMhMaxBins = 4096;
constexpr long long kMhMaxTable = 1ll << 24;             // n * C * bins
constexpr u64 kMpNoMin = ~0ull;                          // the keys of no pixel (no value of a permitted image makes them)
constexpr u64 kMpNoMax = 0ull;

// One instance: the words of its rows r0 .. r0 + rows - 1 and word columns j0 .. j0 + cols - 1 meet the image (rows = cols = 0:
// none does).
struct MpInst {
  long long src_words;        // first word of the rows
  int w, strips;
  int x1, y1;
  int r0, rows, j0, cols;
};

// dtype 0 uint8, 1 uint16, 2 int16, 3 int32: element `at` of the image.  The branch is the same for every lane.
__device__ __forceinline__ int mp_load(const void* __restrict__ image, int dtype, size_t at) {
  switch (dtype) {
    case 0: return (int)((const unsigned char*)image)[at];
    case 1: return (int)((const unsigned short*)image)[at];
    case 2: return (int)((const short*)image)[at];
    default: return ((const int*)image)[at];
  }
}

// Word `idx` of instance a's numbering as its lane sees it: the bits inside the row and the image frame, the image row and the
// image column of bit 0 (which may be negative: such bits are cleared).  idx < a.rows * a.cols.
__device__ __forceinline__ u64 mp_word(const MpInst& a, const u64* __restrict__ bits, int idx, int W, int* y, int* xb) {
  const int q = idx / a.cols, r = a.r0 + q, j = a.j0 + (idx - q * a.cols);
  *y = a.y1 + r;
  *xb = a.x1 + (j << 6);
  const int lo = max(0, -*xb), hi = min(64, W - *xb);
  if (hi <= lo) return 0ull;
  const u64 frame = (hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1ull) << lo;
  return mask_word(bits + a.src_words + (long long)r * a.strips, j, a.strips, a.w) & frame;
}

__device__ __forceinline__ u64 mp_lane_read(u64 v, int t) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, t);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), t);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 mp_wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ u64 mp_wave_min(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(v, o); v = t < v ? t : v; }
  return v;
}
__device__ __forceinline__ u64 mp_wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(v, o); v = t > v ? t : v; }
  return v;
}

// grid ceil(total / 1024) at most 4096, block 256.  flag: one word, zero before.
__global__ __launch_bounds__(kMpThreads) void mp_range_kernel(const int* __restrict__ image, size_t total, unsigned* flag) {
  bool bad = false;
  for (size_t p = (size_t)blockIdx.x * kMpThreads + threadIdx.x; p < total; p += (size_t)gridDim.x * kMpThreads) {
    const int v = image[p];
    bad |= v < -kMpMaxValue || v > kMpMaxValue;
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// grid (ceil(most words / kMpBlockWords), n, tiles), block 256.  The tile takes the channels c_first + T z .. + T - 1, all below C.
// count [n], sums [n][C][4], keys [n][C][2]: zero resp. (kMpNoMin, kMpNoMax) before the call's first launch.
template <int T>
__global__ __launch_bounds__(kMpThreads) void mp_stats_kernel(const MpInst* __restrict__ insts, const u64* __restrict__ bits,
                                                              const void* __restrict__ image, int dtype, int W, int C, int c_first,
                                                              u64* __restrict__ count, u64* __restrict__ sums, u64* __restrict__ keys) {
  constexpr int kFigures = 6 * T + 1;                    // per channel four sums and two keys; the count
  __shared__ u64 s_part[kMpWaves][kFigures];
  const MpInst a = insts[blockIdx.y];
  const int words = a.rows * a.cols;                     // (at most 32768 rows of 512 words)
  if ((long long)blockIdx.x * kMpBlockWords >= words) return;          // (the whole workgroup)
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = c_first + (int)blockIdx.z * T;
  const int mine = (int)blockIdx.x * kMpBlockWords + wv * kMpWaveWords + lane;
  int my_y = 0, my_xb = 0;
  u64 my_v = 0ull;
  if (lane < kMpWaveWords && mine < words) my_v = mp_word(a, bits, mine, W, &my_y, &my_xb);
  u64 sum[T], sq[T], sx[T], sy[T], kmin[T], kmax[T], cnt = 0ull;
#pragma unroll
  for (int k = 0; k < T; ++k) { sum[k] = sq[k] = sx[k] = sy[k] = 0ull; kmin[k] = kMpNoMin; kmax[k] = kMpNoMax; }
  if (__ballot(my_v != 0ull) != 0ull) {
#pragma unroll
    for (int t0 = 0; t0 < kMpWaveWords; t0 += kMpStep) {
      int val[kMpStep][T], x[kMpStep], y[kMpStep];
      bool on[kMpStep];
#pragma unroll
      for (int u = 0; u < kMpStep; ++u) {
        const u64 v = mp_lane_read(my_v, t0 + u);
        y[u] = __builtin_amdgcn_readlane(my_y, t0 + u);
        x[u] = __builtin_amdgcn_readlane(my_xb, t0 + u) + lane;
        on[u] = ((v >> lane) & 1ull) != 0ull;
#pragma unroll
        for (int k = 0; k < T; ++k) val[u][k] = 0;
        if (on[u]) {
          const size_t at = ((size_t)y[u] * (size_t)W + (size_t)x[u]) * (size_t)C + (size_t)c0;
#pragma unroll
          for (int k = 0; k < T; ++k) val[u][k] = mp_load(image, dtype, at + k);
        }
      }
#pragma unroll
      for (int u = 0; u < kMpStep; ++u) {
        if (on[u]) {
          const unsigned pos = ((unsigned)y[u] << 16) | (unsigned)x[u];
          cnt += 1ull;
#pragma unroll
          for (int k = 0; k < T; ++k) {
            const long long v = val[u][k];
            sum[k] += (u64)v;
            sq[k] += (u64)(v * v);
            sx[k] += (u64)(v * x[u]);
            sy[k] += (u64)(v * y[u]);
            const u64 hi = (u64)((unsigned)val[u][k] ^ 0x80000000u) << 32;
            const u64 lo_key = hi | pos, hi_key = hi | (unsigned)~pos;
            kmin[k] = lo_key < kmin[k] ? lo_key : kmin[k];
            kmax[k] = hi_key > kmax[k] ? hi_key : kmax[k];
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < T; ++k) {
    sum[k] = mp_wave_sum(sum[k]);
    sq[k] = mp_wave_sum(sq[k]);
    sx[k] = mp_wave_sum(sx[k]);
    sy[k] = mp_wave_sum(sy[k]);
    kmin[k] = mp_wave_min(kmin[k]);
    kmax[k] = mp_wave_max(kmax[k]);
  }
  cnt = mp_wave_sum(cnt);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < T; ++k) {
      s_part[wv][6 * k + 0] = sum[k];
      s_part[wv][6 * k + 1] = sq[k];
      s_part[wv][6 * k + 2] = sx[k];
      s_part[wv][6 * k + 3] = sy[k];
      s_part[wv][6 * k + 4] = kmin[k];
      s_part[wv][6 * k + 5] = kmax[k];
    }
    s_part[wv][6 * T] = cnt;
  }
  __syncthreads();
  const int f = threadIdx.x;
  if (f >= kFigures) return;
  const int k = f / 6, what = f - 6 * k;                 // (f == 6 T: the count, k = T, what = 0)
  u64 t = s_part[0][f];
#pragma unroll
  for (int w2 = 1; w2 < kMpWaves; ++w2) {
    const u64 o = s_part[w2][f];
    t = f == 6 * T || what < 4 ? t + o : what == 4 ? (o < t ? o : t) : (o > t ? o : t);
  }
  const size_t chan = (size_t)blockIdx.y * C + c0 + k;
  if (f == 6 * T) {
    if (c0 == 0 && t) atomicAdd(&count[blockIdx.y], t);
  } else if (what < 4) {
    if (t) atomicAdd(&sums[chan * 4 + what], t);
  } else if (what == 4) {
    if (t != kMpNoMin) atomicMin(&keys[chan * 2], t);
  } else {
    if (t != kMpNoMax) atomicMax(&keys[chan * 2 + 1], t);
  }
}

// grid (ceil(most words / (4 run)), n, groups), block 256, dynamic LDS 4 * group * bins bytes; run <= 64 words a wave.  Group z takes
// the channels group * z .. below min(C, group * (z + 1)); group * bins <= kMhCells.  count [n] and hist [n][C][bins] are zero before.
__global__ __launch_bounds__(kMpThreads) void mp_hist_kernel(const MpInst* __restrict__ insts, const u64* __restrict__ bits,
                                                             const void* __restrict__ image, int dtype, int W, int C, int group,
                                                             int run, int lo, int shift, int bins, u64* __restrict__ count,
                                                             u64* __restrict__ hist) {
  extern __shared__ unsigned s_cells[];
  const MpInst a = insts[blockIdx.y];
  const int words = a.rows * a.cols;
  if ((long long)blockIdx.x * kMpWaves * run >= words) return;         // (the whole workgroup)
  const int c_lo = (int)blockIdx.z * group, c_hi = min(C, c_lo + group), cells = (c_hi - c_lo) * bins;
  for (int c = threadIdx.x; c < cells; c += kMpThreads) s_cells[c] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int mine = ((int)blockIdx.x * kMpWaves + wv) * run + lane;
  int my_y = 0, my_xb = 0;
  u64 my_v = 0ull;
  if (lane < run && mine < words) my_v = mp_word(a, bits, mine, W, &my_y, &my_xb);
  u64 live = __ballot(my_v != 0ull);                     // the words of this wave that have a bit
  unsigned cnt = 0u;
  while (live) {
    const int t = __ffsll((long long)live) - 1;
    live &= live - 1ull;
    const u64 v = mp_lane_read(my_v, t);
    const int y = __builtin_amdgcn_readlane(my_y, t), x = __builtin_amdgcn_readlane(my_xb, t) + lane;
    const bool on = ((v >> lane) & 1ull) != 0ull;
    cnt += (unsigned)__popcll(v);
    const size_t at = ((size_t)y * (size_t)W + (size_t)x) * (size_t)C;
    for (int c = c_lo; c < c_hi; c += kMhStep) {
      int val[kMhStep];
#pragma unroll
      for (int k = 0; k < kMhStep; ++k) val[k] = on && c + k < c_hi ? mp_load(image, dtype, at + c + k) : 0;
#pragma unroll
      for (int k = 0; k < kMhStep; ++k) {
        int cell = -1;
        if (on && c + k < c_hi) {
          const long long d = (long long)val[k] - lo;
          const long long b = d >> shift;
          if (d >= 0 && b < bins) cell = (c + k - c_lo) * bins + (int)b;
        }
        const u64 act = __ballot(cell >= 0);
        if (act == 0ull) continue;
        const int first = __ffsll((long long)act) - 1;
        const int cell0 = __builtin_amdgcn_readlane(cell, first);
        const u64 same = __ballot(cell == cell0);
        if (lane == first) atomicAdd(&s_cells[cell0], (unsigned)__popcll(same));
        if (cell >= 0 && cell != cell0) atomicAdd(&s_cells[cell], 1u);
      }
    }
  }
  if (blockIdx.z == 0 && lane == 0 && cnt) atomicAdd(&count[blockIdx.y], (u64)cnt);
  __syncthreads();
  u64* __restrict__ out = hist + ((size_t)blockIdx.y * C + c_lo) * (size_t)bins;
  for (int c = threadIdx.x; c < cells; c += kMpThreads) {
    const unsigned v = s_cells[c];
    if (v) atomicAdd(&out[c], (u64)v);
  }
}

namespace {

CallTimer g_mp_timer;

// The checked call: the set, the image, the instance table.
struct MpPlan {
  HostMaskSet set;
  std::vector<MpInst> inst;
  int most_words = 0;          // of one instance, inside the image
  size_t elem = 0;             // bytes of one value
  size_t values = 0;           // H * W * C
};

// What both entries refuse, before anything is launched.
int mp_check(const char* who, MpPlan* p, const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n,
             const void* image, int dtype, int H, int W, int C) {
  MNC_REQUIRE(n >= 0 && n <= kMpMaxN, "%s: n=%d not in [0, %d]", who, n, kMpMaxN);
  MNC_REQUIRE(dtype >= 0 && dtype <= 3, "%s: dtype=%d is not 0 (uint8), 1 (uint16), 2 (int16) or 3 (int32)", who, dtype);
  MNC_REQUIRE(H >= 1 && H <= kMpMaxSide && W >= 1 && W <= kMpMaxSide, "%s: H=%d or W=%d not in [1, %d]", who, H, W, kMpMaxSide);
  MNC_REQUIRE((long long)H * W <= kMpMaxPixels, "%s: %lld pixels (limit %lld)", who, (long long)H * W, kMpMaxPixels);
  MNC_REQUIRE(C >= 1 && C <= kMpMaxChannels, "%s: C=%d not in [1, %d]", who, C, kMpMaxChannels);
  MNC_REQUIRE(n == 0 || image, "%s: null image", who);
  const int rc = p->set.check(who, "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
  if (rc) return rc;
  p->elem = dtype == 0 ? 1 : dtype == 3 ? 4 : 2;
  p->values = (size_t)H * (size_t)W * (size_t)C;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = p->set.info[i];
    MpInst m = MpInst();
    if (mask_has_rows(a)) {
      const int w = a.x2 - a.x1 + 1, h = a.y2 - a.y1 + 1;
      MNC_REQUIRE(w <= kMpMaxExtent && h <= kMpMaxExtent, "%s: masks[%d] is %d x %d (limit %d a side)", who, i, w, h, kMpMaxExtent);
      m.src_words = a.offset / 8;
      m.w = w;
      m.strips = mask_strips(w);
      m.x1 = a.x1;
      m.y1 = a.y1;
      const int r0 = a.y1 < 0 ? -a.y1 : 0, r1 = H - a.y1 < h ? H - a.y1 : h;
      if (r1 > r0 && a.x2 >= 0 && a.x1 < W) {
        const int j0 = a.x1 < 0 ? (-a.x1) >> 6 : 0;
        const int j1 = std::min(m.strips, ((W - 1 - a.x1) >> 6) + 1);
        if (j1 > j0) {
          m.r0 = r0; m.rows = r1 - r0; m.j0 = j0; m.cols = j1 - j0;
          if (m.rows * m.cols > p->most_words) p->most_words = m.rows * m.cols;
        }
      }
    }
    p->inst.push_back(m);
  }
  return MNC_OK;
}

inline unsigned mp_blocks(long long count, int per) { return (unsigned)((count + per - 1) / per); }

// The range pass of an int32 image, into the zeroed flag.
void mp_range_launch(hipStream_t s, const void* d_image, size_t values, unsigned* d_flag) {
  const unsigned blocks = (unsigned)std::min<size_t>((values + 4 * kMpThreads - 1) / (4 * kMpThreads), 4096);
  hipLaunchKernelGGL(mp_range_kernel, dim3(blocks), dim3(kMpThreads), 0, s, (const int*)d_image, values, d_flag);
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_pixel_stats(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const void* image,
                         int dtype, int H, int W, int C, long long* count, long long* sums, int* extrema, int device_id) {
  const char* who = "mnc_mask_pixel_stats";
  MNC_REQUIRE(n <= 0 || (count && sums && extrema), "%s: null output pointer", who);
  MpPlan plan;
  int rc = mp_check(who, &plan, bounds, offsets, bits, bytes, n, image, dtype, H, W, C);
  if (rc) return rc;
  // One block goes up and comes back in one copy each way: the range flag (a whole word of 64 bits), the counts, the sums, the keys.
  const size_t chans = (size_t)n * C, at_sums = 1 + (size_t)n, at_keys = at_sums + chans * 4, out_words = at_keys + chans * 2;
  std::vector<u64> h_out(out_words, 0ull);
  u64 *h_count = h_out.data() + 1, *h_sums = h_out.data() + at_sums, *h_keys = h_out.data() + at_keys;
  for (size_t k = 0; k < chans; ++k) { h_keys[2 * k] = kMpNoMin; h_keys[2 * k + 1] = kMpNoMax; }
  if (plan.most_words > 0) {
    MpInst* d_inst; u64* d_out; unsigned char* d_image;
    auto layout = [&](WsLayout l) {
      plan.set.take(l);
      d_image = l.take<unsigned char>(plan.values * plan.elem);
      d_inst = l.take<MpInst>(n);
      d_out = l.take<u64>(out_words);
      return l.bytes();
    };
    HostScope hs;
    rc = hs.open(device_id, layout(WsLayout()));
    if (rc) return rc;
    layout(WsLayout(hs.buf));
    MNC_HIP_TRY(plan.set.upload(hs));
    MNC_HIP_TRY(hs.up(d_image, image, plan.values * plan.elem));
    MNC_HIP_TRY(hs.up(d_inst, plan.inst.data(), (size_t)n * sizeof(MpInst)));
    MNC_HIP_TRY(hs.up(d_out, h_out.data(), out_words * sizeof(u64)));
    unsigned* d_flag = (unsigned*)d_out;
    u64 *d_count = d_out + 1, *d_sums = d_out + at_sums, *d_keys = d_out + at_keys;
    TimedSpan span(g_mp_timer);
    span.begin(hs.stream);
    if (dtype == 3) mp_range_launch(hs.stream, d_image, plan.values, d_flag);
    const unsigned gx = mp_blocks(plan.most_words, kMpBlockWords);
    const int q = C / 4, r = C % 4;
    if (q)
      hipLaunchKernelGGL(mp_stats_kernel<4>, dim3(gx, (unsigned)n, (unsigned)q), dim3(kMpThreads), 0, hs.stream, d_inst,
                         plan.set.d_bits, d_image, dtype, W, C, 0, d_count, d_sums, d_keys);
    if (r == 3)
      hipLaunchKernelGGL(mp_stats_kernel<3>, dim3(gx, (unsigned)n, 1u), dim3(kMpThreads), 0, hs.stream, d_inst, plan.set.d_bits,
                         d_image, dtype, W, C, 4 * q, d_count, d_sums, d_keys);
    else if (r)
      hipLaunchKernelGGL(mp_stats_kernel<1>, dim3(gx, (unsigned)n, (unsigned)r), dim3(kMpThreads), 0, hs.stream, d_inst,
                         plan.set.d_bits, d_image, dtype, W, C, 4 * q, d_count, d_sums, d_keys);
    span.end(hs.stream);
    MNC_HIP_TRY(hipGetLastError());
    MNC_HIP_TRY(hs.down(h_out.data(), d_out, out_words * sizeof(u64)));
    MNC_HIP_TRY(hs.sync());
    span.keep();
    MNC_REQUIRE(!h_out[0], "%s: an int32 image value not in [%d, %d]", who, -kMpMaxValue, kMpMaxValue);
  }
  for (int i = 0; i < n; ++i) {
    count[i] = (long long)h_count[i];
    for (int c = 0; c < C; ++c) {
      const size_t ch = (size_t)i * C + c;
      for (int f = 0; f < 4; ++f) sums[ch * 4 + f] = (long long)h_sums[ch * 4 + f];
      int* e = extrema + ch * 6;
      if (h_count[i] == 0) {
        e[0] = 0; e[1] = -1; e[2] = -1; e[3] = 0; e[4] = -1; e[5] = -1;
        continue;
      }
      const u64 lo_key = h_keys[ch * 2], hi_key = h_keys[ch * 2 + 1];
      const unsigned lo_pos = (unsigned)lo_key, hi_pos = ~(unsigned)hi_key;
      e[0] = (int)((unsigned)(lo_key >> 32) ^ 0x80000000u);
      e[1] = (int)(lo_pos & 0xffffu);
      e[2] = (int)(lo_pos >> 16);
      e[3] = (int)((unsigned)(hi_key >> 32) ^ 0x80000000u);
      e[4] = (int)(hi_pos & 0xffffu);
      e[5] = (int)(hi_pos >> 16);
    }
  }
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_histogram(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const void* image,
                       int dtype, int H, int W, int C, int lo, int shift, int bins, long long* count, long long* hist,
                       int device_id) {
  const char* who = "mnc_mask_histogram";
  MNC_REQUIRE(n <= 0 || (count && hist), "%s: null output pointer", who);
  MNC_REQUIRE(bins >= 1 && bins <= kMhMaxBins, "%s: bins=%d not in [1, %d]", who, bins, kMhMaxBins);
  MNC_REQUIRE(shift >= 0 && shift <= 31, "%s: shift=%d not in [0, 31]", who, shift);
  MpPlan plan;
  int rc = mp_check(who, &plan, bounds, offsets, bits, bytes, n, image, dtype, H, W, C);
  if (rc) return rc;
  const size_t cells = (size_t)n * C * bins;
  MNC_REQUIRE((long long)cells <= kMhMaxTable, "%s: n * C * bins = %zu (limit %lld)", who, cells, kMhMaxTable);
  if (plan.most_words == 0) {
    for (int i = 0; i < n; ++i) count[i] = 0;
    for (size_t k = 0; k < cells; ++k) hist[k] = 0;
    clear_error();
    return MNC_OK;
  }
  MpInst* d_inst; u64* d_blk; unsigned char* d_image;               // one block, zeroed by one fill: the range flag, the counts, the table
  auto layout = [&](WsLayout l) {
    plan.set.take(l);
    d_image = l.take<unsigned char>(plan.values * plan.elem);
    d_inst = l.take<MpInst>(n);
    d_blk = l.take<u64>(1 + (size_t)n + cells);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(plan.set.upload(hs));
  MNC_HIP_TRY(hs.up(d_image, image, plan.values * plan.elem));
  MNC_HIP_TRY(hs.up(d_inst, plan.inst.data(), (size_t)n * sizeof(MpInst)));
  MNC_HIP_TRY(hipMemsetAsync(d_blk, 0, (1 + (size_t)n + cells) * sizeof(u64), hs.stream));
  unsigned* d_flag = (unsigned*)d_blk;
  u64 *d_count = d_blk + 1, *d_hist = d_blk + 1 + n;
  TimedSpan span(g_mp_timer);
  span.begin(hs.stream);
  if (dtype == 3) mp_range_launch(hs.stream, d_image, plan.values, d_flag);
  const int group = std::min(C, kMhCells / bins), groups = (C + group - 1) / group;
  const int run = group * bins <= kMhSmallTable ? kMhShortRun : kMhLongRun;
  hipLaunchKernelGGL(mp_hist_kernel, dim3(mp_blocks(plan.most_words, kMpWaves * run), (unsigned)n, (unsigned)groups), dim3(kMpThreads),
                     (size_t)group * bins * sizeof(unsigned), hs.stream, d_inst, plan.set.d_bits, d_image, dtype, W, C, group, run, lo,
                     shift, bins, d_count, d_hist);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  if (dtype == 3) {                                        // the flag first: an image that is refused leaves the outputs as they were
    unsigned flag = 0u;
    MNC_HIP_TRY(hs.down(&flag, d_flag, sizeof(unsigned)));
    MNC_HIP_TRY(hs.sync());
    MNC_REQUIRE(!flag, "%s: an int32 image value not in [%d, %d]", who, -kMpMaxValue, kMpMaxValue);
  }
  MNC_HIP_TRY(hs.down(count, d_count, (size_t)n * sizeof(u64)));
  MNC_HIP_TRY(hs.down(hist, d_hist, cells * sizeof(u64)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_pixels_timing(int on, double* last_ms) { return g_mp_timer.set(on, last_ms); }
