// cv2.resize(..., INTER_LINEAR) of an S x S float32 mask, restated for the device (oracle/host.py:resize_bilinear_cv_to,
// mnc_amd/prep.py:linear_taps).  Shared by the image-space voting (mv_image.hip) and the SDS evaluation (sds_eval.hip); both are
// compiled with -ffp-contract=off, so every expression here is evaluated in the reference's operation order and is bit-exact.
#pragma once
#include <hip/hip_runtime.h>

namespace mnc {

// One axis of cv2.resize(src, dsize) INTER_LINEAR for destination index d (resize_bilinear_cv_to's taps): the source coordinate
// ((d + 0.5) * (1 / f) - 0.5) in float64, rounded to float32; floor; fraction in float32; clamped at both ends.  inv = 1.0 / f,
// f = dst_size / src_size in float64.
struct CvTap { int i0, i1; float a; };
__device__ __forceinline__ CvTap cv_tap(int d, double inv, int n_src) {
  const float src = (float)(((double)d + 0.5) * inv - 0.5);
  int i0 = (int)floorf(src);
  float a = src - (float)i0;
  if (i0 < 0) { a = 0.0f; i0 = 0; }
  if (i0 >= n_src - 1) { a = 0.0f; i0 = n_src - 1; }
  return {i0, min(i0 + 1, n_src - 1), a};
}

// the inverse scale factor 1.0 / (float(dst) / src) of one axis
__device__ __forceinline__ double cv_inv(int dst, int src) { return 1.0 / ((double)dst / (double)src); }

// Value of an S x S mask resized to (bh, bw) at (dy, dx): horizontal pass, then vertical, in float32.
__device__ __forceinline__ float cv_px(const float* __restrict__ mk, int S, int dy, int dx, double ifx, double ify) {
  const CvTap tx = cv_tap(dx, ifx, S), ty = cv_tap(dy, ify, S);
  const float* r0 = mk + ty.i0 * S;
  const float* r1 = mk + ty.i1 * S;
  const float bx = 1.0f - tx.a, by = 1.0f - ty.a;
  const float h0 = r0[tx.i0] * bx + r0[tx.i1] * tx.a;
  const float h1 = r1[tx.i0] * bx + r1[tx.i1] * tx.a;
  return h0 * by + h1 * ty.a;
}

}  // namespace mnc
