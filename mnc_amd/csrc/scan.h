// The prefix sums the mask kernels share: the 64-lane shuffle scan, and the two-level exclusive scan of an int array (tiles of 1024
// entries, then the tiles) with the accessor that reads its result.  Internal to libmnc_hip.so; the kernels are scan.hip's.
#pragma once
#include <hip/hip_runtime.h>

namespace mnc {

constexpr int kScanTile = 1024;                 // entries of one scan tile: 4 per thread of a workgroup of 256

inline int scan_tiles(long long count) { return (int)((count + kScanTile - 1) / kScanTile); }

// The inclusive prefix sum over the 64 lanes of a wave, every lane of which comes here (int, unsigned, long long).
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// A scanned array as scan_launch leaves it: the exclusive prefix inside tiles of kScanTile entries, and the exclusive prefix of
// the tiles' sums (tile[tiles] = the total).
struct Scanned {
  const int* in_tile;   // [count]
  const int* tile;      // [tiles + 1]
  int count, tiles;
  // the sum of the entries before k, 0 <= k < count
  __device__ __forceinline__ int at(int k) const { return in_tile[k] + tile[k / kScanTile]; }
  // the same for 0 <= k <= count: the total at k == count
  __device__ __forceinline__ int upto(int k) const { return k < count ? at(k) : tile[tiles]; }
};

// The exclusive scan of count >= 1 entries, two launches on `s` and nothing else: a [count] in place, resp. byte flags [count]
// into in_tile [count]; tile [scan_tiles(count) + 1], whose last entry is the total afterwards.
Scanned scan_launch(hipStream_t s, int* a, int count, int* tile);
Scanned scan_launch(hipStream_t s, const unsigned char* flags, int count, int* in_tile, int* tile);

}  // namespace mnc
