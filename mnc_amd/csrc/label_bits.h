// The values of an integer label map as ranks, shared by mask_labels.hip (n19) and label_pairs.hip (n20): the 16-byte load of a lane's
// pixels, the presence bitmap of the values (one bit per value, 32-bit words), the popcounts of its words, the rank of a value from
// the words' prefix sum (scan.h) and the ids written back at their ranks.  Internal to libmnc_hip.so.  The kernels are static: each
// translation unit that includes this header gets its own copy of the few it launches.  All arithmetic is integer; the only atomic
// is an integer or.
#pragma once
#include "mask_set.h"
#include "scan.h"

namespace mnc {

constexpr int kLbThreads = 256;
constexpr int kLbRun = 4;                          // pixels of one lane in the passes over a flat map
constexpr int kLbMaxId = 1 << 24;                  // label values lie in [0, kLbMaxId)
constexpr int kLbMaxWords = kLbMaxId / 32;         // 2^19 words of the presence bitmap
constexpr int kLbMaxSide = 32768;
constexpr long long kLbMaxPixels = 1ll << 26;
constexpr int kLbMaxSkip = 8;

struct LbSkip {
  int v[kLbMaxSkip];
  int n;
};

// The (at most kLbRun) values of the flat array from p on -> how many there are.
__device__ __forceinline__ int lb_load(const int* __restrict__ a, long long p, long long total, int& v0, int& v1, int& v2, int& v3) {
  if (p + kLbRun <= total) {
    const int4 q = *reinterpret_cast<const int4*>(a + p);  // p is a multiple of 4 and the map starts on a 256-byte boundary
    v0 = q.x; v1 = q.y; v2 = q.z; v3 = q.w;
    return kLbRun;
  }
  const int count = (int)(total - p);
  v0 = a[p];
  v1 = count > 1 ? a[p + 1] : 0;
  v2 = count > 2 ? a[p + 2] : 0;
  v3 = 0;
  return count;
}

// A relaxed look at a word that others join atomically.  The joins are monotone (bits are only set, a minimum only falls, a maximum
// only rises), so a stale value can only make the caller issue an atomic it did not need, never skip one it did.
template <class T>
__device__ __forceinline__ T lb_peek(T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// grid ceil(total / 1024), block 256.  The wave shares its atomics: for each of the lanes' kLbRun positions, the lanes whose value
// changes there are balloted value by value and the first lane of each value sets its bit.  A value that has no word in the bitmap
// sets no bit; with `bad` (may be null) one lane of a wave that holds such a value joins 1 into *bad, where a look does not show it.
static __global__ __launch_bounds__(kLbThreads) void lb_presence_kernel(const int* __restrict__ label, long long total, int words,
                                                                        unsigned* present, unsigned* bad) {
  const long long p = ((long long)blockIdx.x * kLbThreads + threadIdx.x) * kLbRun;
  const int lane = threadIdx.x & 63;
  int v[kLbRun] = {-1, -1, -1, -1};
  const int count = p < total ? lb_load(label, p, total, v[0], v[1], v[2], v[3]) : 0;
  int prev = -1;
  bool outside = false;
#pragma unroll
  for (int e = 0; e < kLbRun; ++e) {
    const bool inside = (unsigned)(v[e] >> 5) < (unsigned)words;
    outside |= e < count && !inside;
    const bool fresh = e < count && v[e] != prev && inside;
    u64 rest = __ballot(fresh);
    while (rest) {
      const int first = __ffsll((long long)rest) - 1;
      const int lv = __shfl(v[e], first);
      rest &= ~__ballot(fresh && v[e] == lv);
      const unsigned bit = 1u << (lv & 31);
      if (lane == first && !(lb_peek(present + (lv >> 5)) & bit)) atomicOr(present + (lv >> 5), bit);
    }
    prev = e < count ? v[e] : prev;
  }
  if (bad) {
    const u64 any = __ballot(outside);
    if (any && lane == __ffsll((long long)any) - 1 && !lb_peek(bad)) atomicOr(bad, 1u);
  }
}

// grid ceil(words / 256), block 256.
static __global__ __launch_bounds__(kLbThreads) void lb_count_kernel(unsigned* __restrict__ present, int words, LbSkip skip,
                                                                     int* __restrict__ cnt) {
  const int w = blockIdx.x * kLbThreads + threadIdx.x;
  if (w >= words) return;
  unsigned m = present[w];
#pragma unroll
  for (int k = 0; k < kLbMaxSkip; ++k)
    if (k < skip.n && (skip.v[k] >> 5) == w) m &= ~(1u << (skip.v[k] & 31));
  present[w] = m;
  cnt[w] = __popc(m);
}

// The rank of value v among the set bits, -1 when its bit is not set.
__device__ __forceinline__ int lb_rank(const unsigned* __restrict__ present, int words, const Scanned& pre, int v) {
  const int w = v >> 5;
  if ((unsigned)w >= (unsigned)words) return -1;
  const unsigned m = present[w], bit = 1u << (v & 31);
  return (m & bit) ? pre.at(w) + __popc(m & (bit - 1u)) : -1;
}

// grid ceil(words / 256), block 256.
static __global__ __launch_bounds__(kLbThreads) void lb_ids_kernel(const unsigned* __restrict__ present, int words, Scanned pre, int cap,
                                                                   int* __restrict__ ids) {
  const int w = blockIdx.x * kLbThreads + threadIdx.x;
  if (w >= words) return;
  unsigned m = present[w];
  for (int k = pre.at(w); m && k < cap; ++k) {
    ids[k] = w * 32 + (__ffs((int)m) - 1);
    m &= m - 1u;
  }
}

}  // namespace mnc
