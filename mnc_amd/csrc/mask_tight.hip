// The parts of the tight-result protocol (mask_tight.h) that are no template: the kernel between the two passes of a family, and
// the window check.  All arithmetic is integer.  14 VGPRs, no LDS and no scratch.
#include "mask_tight.h"

namespace mnc {

// grid ceil(n / 256), block 256: the extents in place into the tight bounds, and the words of their rows.
__global__ __launch_bounds__(kTightThreads) void tight_size_kernel(const TightFrame* __restrict__ frames, int stride, int n,
                                                                   TightBox* __restrict__ box, int* __restrict__ words) {
  const int o = blockIdx.x * kTightThreads + threadIdx.x;
  if (o >= n) return;
  const TightFrame j = frames[(size_t)o * stride];
  const TightBox e = box[o];
  TightBox b = {0, 0, -1, -1};
  int count = 0;
  if (j.fw >= 1 && j.fh >= 1 && e.x2 >= 0) {
    b.x1 = j.fx + e.x1; b.y1 = j.fy + e.y1; b.x2 = j.fx + e.x2; b.y2 = j.fy + e.y2;
    count = (e.y2 - e.y1 + 1) * mask_strips(e.x2 - e.x1 + 1);      // (at most the 2^27 words of the call's loose frames)
  }
  box[o] = b;
  words[o] = count;
}

void tight_size_launch(hipStream_t s, const TightFrame* d_frames, int stride, int n, TightBox* d_box, int* d_words) {
  hipLaunchKernelGGL(tight_size_kernel, dim3((unsigned)((n + kTightThreads - 1) / kTightThreads)), dim3(kTightThreads), 0, s, d_frames,
                     stride, n, d_box, d_words);
}

int tight_check_window(const char* who, const int* window) {
  for (int k = 0; k < 4; ++k)
    MNC_REQUIRE(window[k] > -kTightMaxCoord && window[k] < kTightMaxCoord, "%s: window coordinate %d out of range", who, window[k]);
  MNC_REQUIRE(window[2] >= window[0] && window[3] >= window[1], "%s: the window (%d, %d, %d, %d) is empty", who, window[0], window[1],
              window[2], window[3]);
  return MNC_OK;
}

}  // namespace mnc
