// Image-space mask voting for gfx950 -- cfg.TEST.USE_GPU_MASK_MERGE = False, the reference's cpu_mask_voting +
// mask_aggregation (lib/transform/mask_transform.py:107-210).  The rows, candidate sets and weights come from the same device
// sequence as the `mv` rule (mv.hip: mv_order / NMS / mv_select with its tie flag / mv_candidates); only the voting differs:
//   each candidate mask is resized to its ROUNDED box with cv2's INTER_LINEAR rule, binarised (>= float32(thr)), and the
//   binary masks times their weights are summed on a float64 image canvas; the bounds are where the canvas is >= thr (double),
//   and the bounded region, cast to float32, is resized to S x S with the same cv2 rule.
// As in mv.hip the canvas  A_r(y, x) = sum_j [x0_j <= x <= x1_j, y0_j <= y <= y1_j] * bin_j(y - y0_j, x - x0_j) * w_j  is a pure
// function of (r, y, x) and is never stored:
//   kernel 1  mv_image_bounds   : grid (R, splits).  Each block walks a slab of the union of result r's rounded candidate boxes
//                                 (outside it the canvas is 0 < thr), evaluates A_r per pixel with the candidate descriptors in
//                                 LDS, and reduces "A_r >= thr" to min/max x, y with wave shuffles + one atomicMin/Max per block.
//   kernel 2  mv_image_resample : grid R, 448 threads.  Re-evaluates A_r at the <= 4 canvas pixels each of the S*S output samples
//                                 needs and writes the record row.
// cv2's taps of a candidate at a pixel depend only on (pixel - box corner, box size), so they are recomputed where needed: the
// per-candidate inverse scale factors (a float64 division each) are the only precomputation and live in LDS.
//
// Compiled with -ffp-contract=off: every expression is evaluated in the reference's operation order (numpy float32 / float64
// element-wise arithmetic, oracle/host.py:resize_bilinear_cv_to for cv2.resize), so the outputs are bit-exact.
#include <climits>

#include "cv_resize.h"
#include "mnc_internal.h"

namespace mnc {

constexpr int kMaxImCandLds = 1024;   // candidate descriptors staged in LDS per result (44 KB); more -> read from global memory

struct ImCandLds {
  int x0[kMaxImCandLds], y0[kMaxImCandLds], x1[kMaxImCandLds], y1[kMaxImCandLds], m[kMaxImCandLds];
  double w[kMaxImCandLds], ifx[kMaxImCandLds], ify[kMaxImCandLds];
};

// np.round (half to even) of a float32 box
__device__ __forceinline__ void round_box(const float* __restrict__ b, int& x0, int& y0, int& x1, int& y1) {
  x0 = (int)rintf(b[0]); y0 = (int)rintf(b[1]); x1 = (int)rintf(b[2]); y1 = (int)rintf(b[3]);
}

// A_r(y, x) from the LDS descriptors: candidates in list order, acc += binary * w (mask_aggregation's `+= mask * mask_weight`)
__device__ __forceinline__ double canvas_px(const ImCandLds& cl, int nc, const float* __restrict__ masks, int S, float mthr,
                                            int y, int x) {
  double acc = 0.0;
  for (int j = 0; j < nc; ++j) {
    if (x < cl.x0[j] || x > cl.x1[j] || y < cl.y0[j] || y > cl.y1[j]) continue;
    const float v = cv_px(masks + (long)cl.m[j] * S * S, S, y - cl.y0[j], x - cl.x0[j], cl.ifx[j], cl.ify[j]);
    acc += (v >= mthr ? 1.0 : 0.0) * cl.w[j];
  }
  return acc;
}

// Slow path for results with more than kMaxImCandLds candidates: descriptors straight from global memory.
__device__ double canvas_px_global(const float* __restrict__ boxes, const float* __restrict__ masks, const int* __restrict__ inds,
                                   const float* __restrict__ wts, int c0, int c1, int S, float mthr, int y, int x) {
  double acc = 0.0;
  for (int j = c0; j < c1; ++j) {
    const int m = inds[j];
    int x0, y0, x1, y1;
    round_box(boxes + (long)m * 4, x0, y0, x1, y1);
    if (x < x0 || x > x1 || y < y0 || y > y1) continue;
    const float v = cv_px(masks + (long)m * S * S, S, y - y0, x - x0, cv_inv(x1 - x0 + 1, S), cv_inv(y1 - y0 + 1, S));
    acc += (v >= mthr ? 1.0 : 0.0) * (double)wts[j];
  }
  return acc;
}

__device__ __forceinline__ void stage_im_cands(ImCandLds& cl, const float* __restrict__ boxes, const int* __restrict__ inds,
                                               const float* __restrict__ wts, int c0, int nc, int S) {
  for (int i = threadIdx.x; i < nc; i += blockDim.x) {
    const int m = inds[c0 + i];
    int x0, y0, x1, y1;
    round_box(boxes + (long)m * 4, x0, y0, x1, y1);
    cl.x0[i] = x0; cl.y0[i] = y0; cl.x1[i] = x1; cl.y1[i] = y1;
    cl.m[i] = m;
    cl.w[i] = (double)wts[c0 + i];
    // (an empty box -- x1 < x0 -- covers no pixel; its factors are never used)
    cl.ifx[i] = x1 >= x0 ? cv_inv(x1 - x0 + 1, S) : 0.0;
    cl.ify[i] = y1 >= y0 ? cv_inv(y1 - y0 + 1, S) : 0.0;
  }
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// bounds [R][4] = (min x, min y, max x, max y) of {A_r >= cthr}, pre-set to (INT_MAX, INT_MAX, -1, -1) (mv_candidates_kernel).
// Rows r = blockIdx.x, + gridDim.x, ... < *rcount (or R).
__global__ __launch_bounds__(256) void mv_image_bounds_kernel(const float* __restrict__ boxes, const float* __restrict__ masks,
                                                              int S, const int* __restrict__ inds, const int* __restrict__ begins,
                                                              const int* __restrict__ ends, const float* __restrict__ wts, int H,
                                                              int W, float mthr, double cthr, const int* __restrict__ rcount,
                                                              int R, int* __restrict__ bounds) {
  __shared__ ImCandLds cl;
  __shared__ int red[4][4];
  __shared__ int ubox[4];
  const int Rv = rcount ? *rcount : R;
  for (int r = blockIdx.x; r < Rv; r += gridDim.x) {
    __syncthreads();                      // the previous row's LDS contents are dead from here on
    const int c0 = begins[r], c1 = ends[r];
    const int nc = c1 - c0;
    if (nc <= 0) continue;
    const bool in_lds = nc <= kMaxImCandLds;
    if (in_lds) stage_im_cands(cl, boxes, inds, wts, c0, nc, S);
    if (threadIdx.x == 0) { ubox[0] = INT_MAX; ubox[1] = INT_MAX; ubox[2] = -1; ubox[3] = -1; }
    __syncthreads();
    // union of the rounded boxes, clipped to the canvas
    {
      int lx = INT_MAX, ly = INT_MAX, hx = -1, hy = -1;
      for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        int x0, y0, x1, y1;
        if (in_lds) { x0 = cl.x0[i]; y0 = cl.y0[i]; x1 = cl.x1[i]; y1 = cl.y1[i]; }
        else round_box(boxes + (long)inds[c0 + i] * 4, x0, y0, x1, y1);
        x0 = max(x0, 0); y0 = max(y0, 0); x1 = min(x1, W - 1); y1 = min(y1, H - 1);
        if (x0 <= x1 && y0 <= y1) { lx = min(lx, x0); ly = min(ly, y0); hx = max(hx, x1); hy = max(hy, y1); }
      }
      lx = wave_min_i(lx); ly = wave_min_i(ly); hx = wave_max_i(hx); hy = wave_max_i(hy);
      if ((threadIdx.x & 63) == 0) {
        atomicMin(&ubox[0], lx); atomicMin(&ubox[1], ly); atomicMax(&ubox[2], hx); atomicMax(&ubox[3], hy);
      }
    }
    __syncthreads();
    const int ux1 = ubox[0], uy1 = ubox[1], ux2 = ubox[2], uy2 = ubox[3];
    if (ux2 < ux1 || uy2 < uy1) continue;
    const int uw = ux2 - ux1 + 1, uh = uy2 - uy1 + 1;
    const int rows_per = (uh + gridDim.y - 1) / gridDim.y;
    const int ya = uy1 + blockIdx.y * rows_per, yb = min(uy2 + 1, ya + rows_per);
    int lx = INT_MAX, ly = INT_MAX, hx = -1, hy = -1;
    const long npx = (long)uw * max(0, yb - ya);
    for (long p = threadIdx.x; p < npx; p += blockDim.x) {
      const int y = ya + (int)(p / uw), x = ux1 + (int)(p % uw);
      const double v = in_lds ? canvas_px(cl, nc, masks, S, mthr, y, x)
                              : canvas_px_global(boxes, masks, inds, wts, c0, c1, S, mthr, y, x);
      if (v >= cthr) {  // np.where(im_mask >= cfg.BINARIZE_THRESH), float64
        lx = min(lx, x); hx = max(hx, x); ly = min(ly, y); hy = max(hy, y);
      }
    }
    lx = wave_min_i(lx); ly = wave_min_i(ly); hx = wave_max_i(hx); hy = wave_max_i(hy);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = lx; red[wave][1] = ly; red[wave][2] = hx; red[wave][3] = hy; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < 4; ++k) {
        lx = min(lx, red[k][0]); ly = min(ly, red[k][1]); hx = max(hx, red[k][2]); hy = max(hy, red[k][3]);
      }
      if (hx >= 0) {
        atomicMin(&bounds[r * 4 + 0], lx); atomicMin(&bounds[r * 4 + 1], ly);
        atomicMax(&bounds[r * 4 + 2], hx); atomicMax(&bounds[r * 4 + 3], hy);
      }
    }
  }
}

// block 448 (7 waves; S*S <= 448 active for S = 21), rows as in mv_image_bounds_kernel.  Finalises the box (no pixel reached the
// threshold: the Python-2 centre pixel (W // 2, H // 2), mask_transform.py:124-128) and resizes canvas[y0:y1+1, x0:x1+1] cast to
// float32 to S x S (:204).  Writes the records (x1, y1, x2, y2, score, class id 1..B, S*S mask values), rows from the count up to
// record_cap zero, as mv_resample_kernel does.
__global__ __launch_bounds__(448) void mv_image_resample_kernel(const float* __restrict__ boxes, const float* __restrict__ masks,
                                                                int S, const int* __restrict__ inds,
                                                                const int* __restrict__ begins, const int* __restrict__ ends,
                                                                const float* __restrict__ wts, int H, int W, float mthr,
                                                                const int* __restrict__ bounds, const int* __restrict__ rcount,
                                                                int R, float* __restrict__ records,
                                                                const float* __restrict__ rscore, const int* __restrict__ rows,
                                                                int record_cap) {
  __shared__ ImCandLds cl;
  const int Rv = rcount ? *rcount : R;
  const int D = 6 + S * S;
  for (int r = Rv + blockIdx.x; r < record_cap; r += gridDim.x)
    for (int i = threadIdx.x; i < D; i += blockDim.x) records[(long)r * D + i] = 0.0f;
  for (int r = blockIdx.x; r < Rv && r < record_cap; r += gridDim.x) {
    __syncthreads();
    const int c0 = begins[r], c1 = ends[r];
    const int nc = max(c1 - c0, 0);
    const bool in_lds = nc <= kMaxImCandLds;
    if (in_lds) stage_im_cands(cl, boxes, inds, wts, c0, nc, S);
    __syncthreads();
    int bx1 = bounds[r * 4 + 0], by1 = bounds[r * 4 + 1], bx2 = bounds[r * 4 + 2], by2 = bounds[r * 4 + 3];
    if (bx2 < 0 || by2 < 0) { bx1 = bx2 = W / 2; by1 = by2 = H / 2; }
    float* rec = records + (long)r * D;
    if (threadIdx.x == 0) {
      rec[0] = (float)bx1; rec[1] = (float)by1; rec[2] = (float)bx2; rec[3] = (float)by2;
      rec[4] = rscore[r];
      rec[5] = (float)(rows[2 * r + 1] + 1);
    }
    const int ww = bx2 - bx1 + 1, hh = by2 - by1 + 1;
    const double ifx = cv_inv(S, ww), ify = cv_inv(S, hh);
    for (int idx = threadIdx.x; idx < S * S; idx += blockDim.x) {
      const int ox = idx % S, oy = idx / S;
      const CvTap tx = cv_tap(ox, ifx, ww), ty = cv_tap(oy, ify, hh);
#define MNC_CANVAS(yy, xx) (float)(in_lds ? canvas_px(cl, nc, masks, S, mthr, by1 + (yy), bx1 + (xx)) \
                                          : canvas_px_global(boxes, masks, inds, wts, c0, c1, S, mthr, by1 + (yy), bx1 + (xx)))
      const float a00 = MNC_CANVAS(ty.i0, tx.i0), a01 = MNC_CANVAS(ty.i0, tx.i1);
      const float a10 = MNC_CANVAS(ty.i1, tx.i0), a11 = MNC_CANVAS(ty.i1, tx.i1);
#undef MNC_CANVAS
      const float bx = 1.0f - tx.a, by = 1.0f - ty.a;
      const float h0 = a00 * bx + a01 * tx.a;
      const float h1 = a10 * bx + a11 * tx.a;
      rec[6 + idx] = h0 * by + h1 * ty.a;
    }
  }
}

// The image-space voting of rows [0, *d_rcount) (<= R): candidate sets d_inds / d_wts[d_begins[r] .. d_ends[r]), boxes [n][4],
// masks [n][S][S]; d_bounds pre-set by mv_candidates_kernel.  grid_rows workgroups stride over the rows.
int mv_image_launch(hipStream_t stream, const float* d_boxes, const float* d_masks, int S, const int* d_inds, const int* d_begins,
                    const int* d_ends, const float* d_wts, int H, int W, double thresh, int R, const int* d_rcount, int grid_rows,
                    int* d_bounds, float* d_records, const float* d_rscore, const int* d_rows, int record_cap) {
  if (R <= 0 || grid_rows <= 0) return MNC_OK;
  int splits = 2048 / grid_rows;
  if (splits < 1) splits = 1;
  if (splits > 32) splits = 32;
  // a float32 mask is compared with the threshold in float32 (numpy value-based casting), the float64 canvas in float64
  const float mthr = (float)thresh;
  hipLaunchKernelGGL(mv_image_bounds_kernel, dim3(grid_rows, splits), dim3(256), 0, stream, d_boxes, d_masks, S, d_inds, d_begins,
                     d_ends, d_wts, H, W, mthr, thresh, d_rcount, R, d_bounds);
  hipLaunchKernelGGL(mv_image_resample_kernel, dim3(grid_rows), dim3(448), 0, stream, d_boxes, d_masks, S, d_inds, d_begins,
                     d_ends, d_wts, H, W, mthr, d_bounds, d_rcount, R, d_records, d_rscore, d_rows, record_cap);
  return MNC_OK;
}

}  // namespace mnc
