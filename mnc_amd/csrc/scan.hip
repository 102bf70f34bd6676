// The two-level exclusive scan of scan.h for gfx950: one workgroup per tile of 1024 entries, then one workgroup over the tiles'
// sums.  Integer sums only.  mask_components.hip, mask_contours.hip, contour_simplify.hip
// and mask_surface.hip, among others, launch it.
#include "scan.h"

namespace mnc {

constexpr int kScanThreads = 256;
static_assert(kScanTile == 4 * kScanThreads, "four entries per thread");

// grid ceil(count / 1024), block 256.  in [count] -> in_tile [count], its exclusive prefix inside the tile; tile[blockIdx.x] = the
// tile's sum.  in_tile may be in itself: a thread reads its four entries before it writes them, and no other thread touches them.
template <class T>
__global__ __launch_bounds__(kScanThreads) void scan_tiles_kernel(const T* in, int count, int* in_tile, int* __restrict__ tile) {
  __shared__ int s_wave[kScanThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long k0 = (long long)blockIdx.x * kScanTile + threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = k0 + e < count ? (int)in[k0 + e] : 0;
  const int sum = v[0] + v[1] + v[2] + v[3];
  const int incl = wave_incl_scan(sum, lane);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int before = incl - sum;
  for (int k = 0; k < wave; ++k) before += s_wave[k];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (k0 + e < count) in_tile[k0 + e] = before;
    before += v[e];
  }
  if (threadIdx.x == kScanThreads - 1) tile[blockIdx.x] = before;
}

// grid 1, block 256.  tile [tiles] -> its exclusive prefix; tile[tiles] = the total.
__global__ __launch_bounds__(kScanThreads) void scan_top_kernel(int* __restrict__ tile, int tiles) {
  __shared__ int s_wave[kScanThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int t0 = 0; t0 < tiles; t0 += kScanThreads) {
    const int t = t0 + threadIdx.x;
    const int v = t < tiles ? tile[t] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = incl - v, all = 0;
    for (int k = 0; k < kScanThreads / 64; ++k) {
      if (k < wave) before += s_wave[k];
      all += s_wave[k];
    }
    if (t < tiles) tile[t] = base + before;
    base += all;
    __syncthreads();                                     // s_wave is written again
  }
  if (threadIdx.x == 0) tile[tiles] = base;
}

template <class T>
static Scanned scan_launch_of(hipStream_t s, const T* in, int count, int* in_tile, int* tile) {
  const int tiles = scan_tiles(count);
  hipLaunchKernelGGL(scan_tiles_kernel<T>, dim3(tiles), dim3(kScanThreads), 0, s, in, count, in_tile, tile);
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kScanThreads), 0, s, tile, tiles);
  return {in_tile, tile, count, tiles};
}

Scanned scan_launch(hipStream_t s, int* a, int count, int* tile) { return scan_launch_of<int>(s, a, count, a, tile); }

Scanned scan_launch(hipStream_t s, const unsigned char* flags, int count, int* in_tile, int* tile) {
  return scan_launch_of<unsigned char>(s, flags, count, in_tile, tile);
}

}  // namespace mnc
