// Backward passes of the per-RoI layers of csrc/roi.hip for gfx950: ROIWarping (w.r.t. the feature map and w.r.t. the box), the
// MAX 2x2/2 pooling behind it, MaskResize and MaskPooling -- include/mnc_hip.h n24; the statements are mnc_amd/backward.py.
//
// Every kernel here is the adjoint of a forward kernel of roi.hip under the SPEC's default conventions (oracle/SPEC.md 1-3), and
// the sample geometry (x1s .. ay) is written with the forward's own float32 expressions in the forward's order: the file is
// compiled with -ffp-contract=off like roi.hip, so the bilinear weights are the forward's bits.
//
// No floating-point atomics.  The sums whose order the rule fixes (dfeat of the warp, din of MaskResize) are GATHERS: the thread
// that owns an output element walks the contributions in the stated order.  The two reductions whose order is the launch's
// (drois, dmask) run through one fixed shuffle / LDS tree: the same bytes on every run.
#include <climits>

#include "mnc_internal.h"

namespace mnc {

__device__ __forceinline__ float4 bw_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void bw_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// The forward's geometry of one RoI (roi_warp_kernel, unfused: the grid is PH x PW), expression for expression.
struct WarpBox {
  float x1s, y1s, bw, bh;
  bool free_w, free_h;             // the max(., 1) clamp of the width / height is inactive or tied: the far edge moves the samples
};
__device__ __forceinline__ WarpBox warp_box(const float* __restrict__ roi, float scale, int PH, int PW) {
  WarpBox b;
  const float x1s = roi[1] * scale, y1s = roi[2] * scale, x2s = roi[3] * scale, y2s = roi[4] * scale;
  const float ew = x2s - x1s + 1.0f, eh = y2s - y1s + 1.0f;
  const float rw = fmaxf(ew, 1.0f), rh = fmaxf(eh, 1.0f);
  b.x1s = x1s; b.y1s = y1s;
  b.bw = rw / (float)PW; b.bh = rh / (float)PH;
  b.free_w = ew >= 1.0f; b.free_h = eh >= 1.0f;
  return b;
}
__device__ __forceinline__ int warp_cell(float lo, float bin, int g) { return (int)floorf(lo + (float)g * bin); }

// ---- dfeat of the warp, pre-pass: which samples of a RoI touch a column / a row ---------------------------------------------
// Column x receives a tap of sample column pw iff x0(pw) is x - 1 or x.  x0(pw) = floor(x1s + pw * bw) does not decrease with pw
// (bw > 0, float32 rounding is monotone), so those pw are one contiguous range [first pw with x0 >= x - 1, first pw with x0 > x):
// found by binary search over the forward's own expression -- an algebraic inversion would have to reproduce its rounding.
// One thread per (roi, column) and per (roi, row); tables [R][W][2] and [R][H][2] of int16 (PH, PW < 32768: checked).
__device__ __forceinline__ int warp_first_cell_ge(float lo, float bin, int G, int cell) {
  int a = 0, b = G;                        // first g in [0, G] with warp_cell(g) >= cell
  while (a < b) {
    const int m = (a + b) >> 1;
    if (warp_cell(lo, bin, m) >= cell) b = m; else a = m + 1;
  }
  return a;
}
__global__ __launch_bounds__(256) void warp_ranges_kernel(const float* __restrict__ rois, int R, int H, int W, int PH, int PW,
                                                          float scale, short* __restrict__ xr, short* __restrict__ yr) {
  const int per = W + H;
  const long total = (long)R * per;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int r = (int)(idx / per), k = (int)(idx % per);
    const WarpBox b = warp_box(rois + (long)r * 5, scale, PH, PW);
    if (k < W) {
      short* o = xr + ((long)r * W + k) * 2;
      o[0] = (short)warp_first_cell_ge(b.x1s, b.bw, PW, k - 1);
      o[1] = (short)warp_first_cell_ge(b.x1s, b.bw, PW, k + 1);
    } else {
      const int y = k - W;
      short* o = yr + ((long)r * H + y) * 2;
      o[0] = (short)warp_first_cell_ge(b.y1s, b.bh, PH, y - 1);
      o[1] = (short)warp_first_cell_ge(b.y1s, b.bh, PH, y + 1);
    }
  }
}

// ---- dfeat of the warp, main kernel ------------------------------------------------------------------------------------------
// One wave owns one cell (y, x) and 64 four-channel groups (two waves per cell at C = 512).  It walks the RoIs in ascending order,
// 64 at a time: every lane fetches the four range ends of one RoI, a ballot leaves the RoIs whose two ranges are both non-empty
// (few: most RoIs do not reach the cell), and those are visited lowest first.  Inside a RoI: ph, then pw, ascending; a sample's
// cell (y0, x0) is recomputed with the forward's expression and the one tap that lands on (y, x) is selected -- the tables only
// shorten the walk, they decide nothing -- and the weight, formed as in the forward, times the float4 of dtop is added.  That is the
// statement's order (r, ph, pw; the four taps of one sample land on four different cells), so the sum is its bits.  Channels are
// fastest in [R][PH][PW][C]: a wave reads a contiguous kilobyte per sample.  Every cell is written, zeros included.
__global__ __launch_bounds__(256) void warp_dfeat_kernel(const float* __restrict__ dtop, const float* __restrict__ rois,
                                                         const short* __restrict__ xr, const short* __restrict__ yr, int C, int H,
                                                         int W, int R, int PH, int PW, float scale, float* __restrict__ dfeat_hwc) {
  const int C4 = C >> 2, lane = threadIdx.x & 63;
  const int chunks = (C4 + 63) >> 6;
  const unsigned nitems = (unsigned)H * W * chunks;
  const unsigned nwaves = (gridDim.x * blockDim.x) >> 6;
  for (unsigned it = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; it < nitems; it += nwaves) {
    const unsigned item = __builtin_amdgcn_readfirstlane(it);
    const int chunk = (int)(item % (unsigned)chunks);
    const unsigned cell = item / (unsigned)chunks;
    const int x = (int)(cell % (unsigned)W), y = (int)(cell / (unsigned)W);
    const int c4 = chunk * 64 + lane;
    const bool have = c4 < C4;                                       // (a ragged last chunk: the lanes past C only take part in the ballot)
    const float* g0 = dtop + (have ? c4 * 4 : 0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r0 = 0; r0 < R; r0 += 64) {
      const int rr = r0 + lane;
      int xl = 0, xh = 0, yl = 0, yh = 0;
      if (rr < R) {
        const short* px = xr + ((long)rr * W + x) * 2;
        const short* py = yr + ((long)rr * H + y) * 2;
        xl = px[0]; xh = px[1]; yl = py[0]; yh = py[1];
      }
      unsigned long long live = __ballot(xl < xh && yl < yh);
      while (live) {
        const int b = __ffsll((long long)live) - 1;
        live &= live - 1;
        const int r = r0 + b;
        const int pw0 = __builtin_amdgcn_readlane(xl, b), pw1 = __builtin_amdgcn_readlane(xh, b);
        const int ph0 = __builtin_amdgcn_readlane(yl, b), ph1 = __builtin_amdgcn_readlane(yh, b);
        const WarpBox bx = warp_box(rois + (long)r * 5, scale, PH, PW);
        for (int ph = ph0; ph < ph1; ++ph) {
          const float sy = bx.y1s + (float)ph * bx.bh;
          const int y0 = (int)floorf(sy);
          const float ay = sy - (float)y0;
          if (y != y0 && y != y0 + 1) continue;
          const bool low = y != y0;                                  // the tap of the sample's second row
          const float* grow = g0 + ((long)r * PH + ph) * PW * C;
          for (int pw = pw0; pw < pw1; ++pw) {
            const float sx = bx.x1s + (float)pw * bx.bw;
            const int x0 = (int)floorf(sx);
            const float ax = sx - (float)x0;
            if (x != x0 && x != x0 + 1) continue;
            const bool right = x != x0;
            const float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay), w10 = (1.0f - ax) * ay, w11 = ax * ay;
            const float w = low ? (right ? w11 : w10) : (right ? w01 : w00);
            if (have) {
              const float4 g = bw_ld4(grow + (long)pw * C);
              acc.x = acc.x + w * g.x; acc.y = acc.y + w * g.y; acc.z = acc.z + w * g.z; acc.w = acc.w + w * g.w;
            }
          }
        }
      }
    }
    if (have) bw_st4(dfeat_hwc + ((long)y * W + x) * C + c4 * 4, acc);
  }
}

// pixel-major [H][W][C] -> c8 [C/8][H][W][8]: the mirror of roi.hip's c8_to_hwc_kernel
__global__ __launch_bounds__(256) void hwc_to_c8_kernel(const float* __restrict__ in, float* __restrict__ out, int CB, long HW) {
  const long total = HW * CB * 2;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int half = (int)(idx & 1);
    const long t = idx >> 1;
    const int cb = (int)(t % CB);
    const long p = t / CB;
    bw_st4(out + ((long)cb * HW + p) * 8 + half * 4, bw_ld4(in + (p * CB + cb) * 8 + half * 4));
  }
}

// ---- drois of the warp -------------------------------------------------------------------------------------------------------
// One workgroup per RoI.  Thread t takes the items t, t + 256, ... of the RoI's (sample, four-channel group) list, channels
// fastest; per item the slopes of the bilinear blend along x and along y times g, summed over its four channels, weighted with
// (1 - t) and t of the sample and added to the thread's four partial sums.  The four sums are then reduced by shuffles within the
// wave and through LDS across the four waves, in one fixed tree; thread 0 applies the scale and writes the RoI's five floats.
__global__ __launch_bounds__(256) void warp_drois_kernel(const float* __restrict__ feat_hwc, const float* __restrict__ dtop,
                                                         const float* __restrict__ rois, int C, int H, int W, int PH, int PW,
                                                         float scale, float* __restrict__ drois) {
  __shared__ float part[4][4];
  const int r = blockIdx.x;
  const unsigned C4 = (unsigned)C >> 2;
  const unsigned nitems = (unsigned)PH * PW * C4;                    // < 2^31: checked by the launcher
  const WarpBox bx = warp_box(rois + (long)r * 5, scale, PH, PW);
  const float* g0 = dtop + (long)r * PH * PW * C;
  float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
  for (unsigned idx = threadIdx.x; idx < nitems; idx += 256) {
    const int c4 = (int)(idx % C4);
    const unsigned pos = idx / C4;
    const int pw = (int)(pos % (unsigned)PW), ph = (int)(pos / (unsigned)PW);
    const float sx = bx.x1s + (float)pw * bx.bw, sy = bx.y1s + (float)ph * bx.bh;
    const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
    const float ax = sx - (float)x0, ay = sy - (float)y0;
    const bool vy0 = y0 >= 0 && y0 < H, vy1 = y0 + 1 >= 0 && y0 + 1 < H;
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x0 + 1 >= 0 && x0 + 1 < W;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* p00 = feat_hwc + ((long)y0 * W + x0) * C + c4 * 4;  // dereferenced only where the tap is inside the map
    const float* p10 = p00 + (long)W * C;
    const float4 f00 = (vy0 && vx0) ? bw_ld4(p00) : z, f01 = (vy0 && vx1) ? bw_ld4(p00 + C) : z;
    const float4 f10 = (vy1 && vx0) ? bw_ld4(p10) : z, f11 = (vy1 && vx1) ? bw_ld4(p10 + C) : z;
    const float4 g = bw_ld4(g0 + (long)idx * 4);                     // == ((ph * PW + pw) * C + c4 * 4)
#define MNC_DSX(f) (g.f * ((1.0f - ay) * (f01.f - f00.f) + ay * (f11.f - f10.f)))
#define MNC_DSY(f) (g.f * ((1.0f - ax) * (f10.f - f00.f) + ax * (f11.f - f01.f)))
    const float gx = ((MNC_DSX(x) + MNC_DSX(y)) + MNC_DSX(z)) + MNC_DSX(w);
    const float gy = ((MNC_DSY(x) + MNC_DSY(y)) + MNC_DSY(z)) + MNC_DSY(w);
#undef MNC_DSX
#undef MNC_DSY
    const float tx = bx.free_w ? (float)pw / (float)PW : 0.0f, ty = bx.free_h ? (float)ph / (float)PH : 0.0f;
    s1 += (1.0f - tx) * gx; s3 += tx * gx;
    s2 += (1.0f - ty) * gy; s4 += ty * gy;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s1 += __shfl_down(s1, d, 64); s2 += __shfl_down(s2, d, 64); s3 += __shfl_down(s3, d, 64); s4 += __shfl_down(s4, d, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { part[wave][0] = s1; part[wave][1] = s2; part[wave][2] = s3; part[wave][3] = s4; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = drois + (long)r * 5;
    o[0] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[1 + k] = scale * (((part[0][k] + part[1][k]) + part[2][k]) + part[3][k]);
  }
}

// ---- MAX 2x2/2 on [R][PH][PW][C], backward -----------------------------------------------------------------------------------
// thread = (roi, oh, ow, four-channel group), as maxpool2_rhwc_kernel.  The argmax is recomputed from the forward's input in its
// max4 order (0,0), (0,1), (1,0), (1,1): a later element wins only when strictly greater (Caffe's rule); the winner gets the
// output's gradient, the other three +0.0f -- all four input cells of the window are written.
__device__ __forceinline__ int first_max(float a, float b, float c, float d) {
  int k = 0;
  float m = a;
  if (b > m) { m = b; k = 1; }
  if (c > m) { m = c; k = 2; }
  if (d > m) { m = d; k = 3; }
  return k;
}
__global__ __launch_bounds__(256) void maxpool2_rhwc_backward_kernel(const float* __restrict__ in, const float* __restrict__ dout,
                                                                     float* __restrict__ din, int R, int PH, int PW, int C4) {
  const int OH = PH / 2, OW = PW / 2;
  const unsigned total = (unsigned)R * OH * OW * C4;               // < 2^31 (checked by the launcher)
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int c4 = (int)(idx % (unsigned)C4);
    unsigned t = idx / (unsigned)C4;
    const int ow = (int)(t % (unsigned)OW);
    t /= (unsigned)OW;
    const int oh = (int)(t % (unsigned)OH);
    const long r = t / (unsigned)OH;
    const long o00 = (((r * PH + 2 * oh) * PW + 2 * ow) * C4 + c4) * 4;
    const long o01 = o00 + (long)C4 * 4, o10 = o00 + (long)PW * C4 * 4, o11 = o10 + (long)C4 * 4;
    const float4 a = bw_ld4(in + o00), b = bw_ld4(in + o01), c = bw_ld4(in + o10), d = bw_ld4(in + o11);
    const float4 g = bw_ld4(dout + (long)idx * 4);
    const int kx = first_max(a.x, b.x, c.x, d.x), ky = first_max(a.y, b.y, c.y, d.y);
    const int kz = first_max(a.z, b.z, c.z, d.z), kw = first_max(a.w, b.w, c.w, d.w);
#define MNC_SEL(k) make_float4(kx == k ? g.x : 0.0f, ky == k ? g.y : 0.0f, kz == k ? g.z : 0.0f, kw == k ? g.w : 0.0f)
    bw_st4(din + o00, MNC_SEL(0));
    bw_st4(din + o01, MNC_SEL(1));
    bw_st4(din + o10, MNC_SEL(2));
    bw_st4(din + o11, MNC_SEL(3));
#undef MNC_SEL
  }
}

// ---- MaskResize backward (SPEC.md 2, the default mode) -----------------------------------------------------------------------
// thread = one input cell (r, iy, ix): it walks the output cells h, then w, ascending, recomputes the forward's source cell and
// fractions and adds weight * dout where one of the cell's taps is its own -- the bilinear four, or weight 1 on the nearest cell
// when the forward took the last source row / column.
__global__ __launch_bounds__(256) void mask_resize_backward_kernel(const float* __restrict__ dout, float* __restrict__ din, int R,
                                                                   int IH, int IW, int OH, int OW) {
  const long total = (long)R * IH * IW;
  const float rh = (float)IH / (float)OH, rw = (float)IW / (float)OW;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int ix = (int)(idx % IW), iy = (int)((idx / IW) % IH);
    const long r = idx / ((long)IW * IH);
    const float* g = dout + r * OH * OW;
    float acc = 0.0f;
    for (int h = 0; h < OH; ++h) {
      const float fy0 = (float)h * rh;
      const int sy = (int)floorf(fy0);
      if (iy != sy && iy != sy + 1) continue;
      const float fy = fy0 - (float)sy;
      for (int w = 0; w < OW; ++w) {
        const float fx0 = (float)w * rw;
        const int sx = (int)floorf(fx0);
        if (ix != sx && ix != sx + 1) continue;
        const float v = g[h * OW + w];
        if (sx == IW - 1 || sy == IH - 1) {
          if (ix == sx && iy == sy) acc = acc + v;
        } else {
          const float fx = fx0 - (float)sx;
          const float wgt = iy == sy ? (ix == sx ? (1.0f - fx) * (1.0f - fy) : fx * (1.0f - fy))
                                     : (ix == sx ? (1.0f - fx) * fy : fx * fy);
          acc = acc + wgt * v;
        }
      }
    }
    din[idx] = acc;
  }
}

// ---- MaskPooling backward (SPEC.md 3, the continuous mask) -------------------------------------------------------------------
// One wave per position (r, h, w); the lanes stride over the four-channel groups.  dfeat = dtop * mask, element by element;
// dmask = sum over the channels of dtop * feat: per lane in channel order, then the shuffle tree, lane 0 writes.
__global__ __launch_bounds__(256) void mask_pool_backward_kernel(const float* __restrict__ feat, const float* __restrict__ mask,
                                                                 const float* __restrict__ dtop, float* __restrict__ dfeat,
                                                                 float* __restrict__ dmask, unsigned npos, int C4) {
  const int lane = threadIdx.x & 63;
  const unsigned nwaves = (gridDim.x * blockDim.x) >> 6;
  for (unsigned p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < npos; p += nwaves) {
    const unsigned pos = __builtin_amdgcn_readfirstlane(p);
    const float mk = dfeat ? mask[pos] : 0.0f;
    const long base = (long)pos * C4 * 4;
    float s = 0.0f;
    for (int c4 = lane; c4 < C4; c4 += 64) {
      const float4 d = bw_ld4(dtop + base + c4 * 4);
      if (dfeat) bw_st4(dfeat + base + c4 * 4, make_float4(d.x * mk, d.y * mk, d.z * mk, d.w * mk));
      if (dmask) {
        const float4 f = bw_ld4(feat + base + c4 * 4);
        s += ((d.x * f.x + d.y * f.y) + d.z * f.z) + d.w * f.w;
      }
    }
    if (dmask) {
#pragma unroll
      for (int k = 32; k >= 1; k >>= 1) s += __shfl_down(s, k, 64);
      if (lane == 0) dmask[pos] = s;
    }
  }
}

static int bw_grid(long total) {
  long g = (total + 255) / 256;
  if (g > 256 * 64) g = 256 * 64;
  if (g < 1) g = 1;
  return (int)g;
}

static size_t bw_align(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace mnc

using namespace mnc;

#define MNC_SPEC_ONLY(cond, ...)       \
  do {                                 \
    if (!(cond)) {                     \
      mnc::set_error(__VA_ARGS__);     \
      return MNC_ERR_UNSUPPORTED;      \
    }                                  \
  } while (0)

extern "C" {

int mnc_roi_warp_backward(mnc_ctx* ctx, const float* d_feat, int C, int H, int W, const float* d_rois, int R, int PH, int PW,
                          float scale, const float* d_dtop, float* d_dfeat, float* d_drois) {
  MNC_REQUIRE(ctx && (d_dfeat || d_drois) && (R == 0 || (d_rois && d_dtop)) && (!d_drois || R == 0 || d_feat),
              "mnc_roi_warp_backward: null pointer");
  MNC_REQUIRE(C > 0 && C % 8 == 0 && H > 0 && W > 0 && R >= 0 && PH > 0 && PW > 0, "mnc_roi_warp_backward: bad shape");
  MNC_REQUIRE(PH < 32768 && PW < 32768, "mnc_roi_warp_backward: PH, PW must be below 32768");
  const long total = (long)R * PH * PW * (C / 4);
  MNC_REQUIRE(total < (1L << 31), "mnc_roi_warp_backward: %ld gradients exceed the kernels' 32-bit index range", total * 4);
  MNC_REQUIRE((double)H * W * C < 2.0e9, "mnc_roi_warp_backward: feature map too large for 32-bit offsets");
  MNC_SPEC_ONLY(!(ctx->conv.warp_sample || ctx->conv.warp_round_edges || ctx->conv.warp_no_plus_one || ctx->conv.warp_oob),
                "mnc_roi_warp_backward: only the SPEC's ROIWarping conventions have a backward pass");
  const size_t map_bytes = (size_t)C * H * W * 4;
  if (R == 0) {
    (void)hipSetDevice(ctx->device);
    if (d_dfeat) MNC_HIP_TRY(hipMemsetAsync(d_dfeat, 0, map_bytes, ctx->stream));
    clear_error();
    return MNC_OK;
  }
  // scratch: [feat, pixel-major (drois)] [dfeat, pixel-major] [column ranges] [row ranges]
  const size_t o_feat = 0, o_dfeat = o_feat + (d_drois ? bw_align(map_bytes) : 0);
  const size_t o_xr = o_dfeat + (d_dfeat ? bw_align(map_bytes) : 0), o_yr = o_xr + (d_dfeat ? bw_align((size_t)R * W * 4) : 0);
  const size_t need = o_yr + (d_dfeat ? bw_align((size_t)R * H * 4) : 0);
  int rc = ensure_scratch(ctx, need);
  if (rc) return rc;
  char* ws = (char*)ctx->scratch.p;
  if (d_dfeat) {
    float* hwc = (float*)(ws + o_dfeat);
    short* xr = (short*)(ws + o_xr);
    short* yr = (short*)(ws + o_yr);
    {
      LaunchScope ls(ctx, "roi_warp_bw_ranges");
      hipLaunchKernelGGL(warp_ranges_kernel, dim3(bw_grid((long)R * (W + H))), dim3(256), 0, ctx->stream, d_rois, R, H, W, PH, PW,
                         scale, xr, yr);
      rc = ls.finish("warp_ranges_kernel");
      if (rc) return rc;
    }
    {
      LaunchScope ls(ctx, "roi_warp_bw_dfeat", 0.0, 4.0 * (4.0 * R * PH * PW * (double)C + (double)C * H * W));
      const long waves = (long)H * W * ((C / 4 + 63) / 64);
      hipLaunchKernelGGL(warp_dfeat_kernel, dim3(bw_grid(waves * 64)), dim3(256), 0, ctx->stream, d_dtop, d_rois, xr, yr, C, H, W,
                         R, PH, PW, scale, hwc);
      rc = ls.finish("warp_dfeat_kernel");
      if (rc) return rc;
    }
    {
      LaunchScope ls(ctx, "hwc_to_c8", 0.0, 8.0 * C * (double)H * W);
      hipLaunchKernelGGL(hwc_to_c8_kernel, dim3(bw_grid((long)H * W * (C / 8) * 2)), dim3(256), 0, ctx->stream, hwc, d_dfeat, C / 8,
                         (long)H * W);
      rc = ls.finish("hwc_to_c8_kernel");
      if (rc) return rc;
    }
  }
  if (d_drois) {
    float* hwc = (float*)(ws + o_feat);
    rc = c8_to_hwc_launch(ctx, d_feat, hwc, C, H, W);
    if (rc) return rc;
    LaunchScope ls(ctx, "roi_warp_bw_drois", 0.0, 4.0 * 5.0 * R * PH * PW * (double)C);
    hipLaunchKernelGGL(warp_drois_kernel, dim3(R), dim3(256), 0, ctx->stream, hwc, d_dtop, d_rois, C, H, W, PH, PW, scale, d_drois);
    rc = ls.finish("warp_drois_kernel");
    if (rc) return rc;
  }
  clear_error();
  return MNC_OK;
}

int mnc_maxpool2_rhwc_backward(mnc_ctx* ctx, const float* d_in, const float* d_dout, float* d_din, int R, int PH, int PW, int C) {
  MNC_REQUIRE(ctx && d_in && d_dout && d_din && R >= 0 && PH > 0 && PW > 0 && PH % 2 == 0 && PW % 2 == 0 && C > 0 && C % 4 == 0,
              "mnc_maxpool2_rhwc_backward: bad argument (PH, PW must be even, C%%4==0)");
  if (R == 0) return MNC_OK;
  MNC_REQUIRE((long)R * PH * PW * (C / 4) < (1L << 31), "mnc_maxpool2_rhwc_backward: tensor exceeds the kernel's 32-bit index range");
  LaunchScope ls(ctx, "maxpool2_rhwc_bw", 0.0, 4.0 * R * (double)C * PH * PW * 2.25);
  hipLaunchKernelGGL(maxpool2_rhwc_backward_kernel, dim3(bw_grid((long)R * (PH / 2) * (PW / 2) * (C / 4))), dim3(256), 0, ctx->stream,
                     d_in, d_dout, d_din, R, PH, PW, C / 4);
  return ls.finish("maxpool2_rhwc_backward_kernel");
}

int mnc_mask_resize_backward(mnc_ctx* ctx, const float* d_dout, float* d_din, int R, int IH, int IW, int OH, int OW) {
  MNC_REQUIRE(ctx && d_dout && d_din && R >= 0 && IH > 1 && IW > 1 && OH > 0 && OW > 0, "mnc_mask_resize_backward: bad argument");
  MNC_SPEC_ONLY(ctx->conv.resize_mode == 0, "mnc_mask_resize_backward: only the SPEC's MaskResize convention has a backward pass");
  if (R == 0) return MNC_OK;
  LaunchScope ls(ctx, "mask_resize_bw");
  hipLaunchKernelGGL(mask_resize_backward_kernel, dim3(bw_grid((long)R * IH * IW)), dim3(256), 0, ctx->stream, d_dout, d_din, R, IH,
                     IW, OH, OW);
  return ls.finish("mask_resize_backward_kernel");
}

int mnc_mask_pool_backward(mnc_ctx* ctx, const float* d_feat, const float* d_mask, const float* d_dtop, float* d_dfeat,
                           float* d_dmask, int R, int PH, int PW, int C) {
  MNC_REQUIRE(ctx && d_dtop && (d_dfeat || d_dmask) && (!d_dfeat || d_mask) && (!d_dmask || d_feat) && R >= 0 && PH > 0 && PW > 0 &&
                  C > 0 && C % 4 == 0,
              "mnc_mask_pool_backward: bad argument");
  MNC_SPEC_ONLY(ctx->conv.maskpool_binary == 0,
                "mnc_mask_pool_backward: only the SPEC's MaskPooling convention (the continuous mask) has a backward pass");
  if (R == 0) return MNC_OK;
  MNC_REQUIRE((long)R * PH * PW * (C / 4) < (1L << 31), "mnc_mask_pool_backward: tensor exceeds the kernel's 32-bit index range");
  LaunchScope ls(ctx, "mask_pool_bw", 0.0, 4.0 * R * (double)C * PH * PW * ((d_dfeat ? 2.0 : 1.0) + (d_dmask ? 1.0 : 0.0)));
  const long npos = (long)R * PH * PW;
  hipLaunchKernelGGL(mask_pool_backward_kernel, dim3(bw_grid(npos * 64)), dim3(256), 0, ctx->stream, d_feat, d_mask, d_dtop, d_dfeat,
                     d_dmask, (unsigned)npos, C / 4);
  return ls.finish("mask_pool_backward_kernel");
}

}  // extern "C"
