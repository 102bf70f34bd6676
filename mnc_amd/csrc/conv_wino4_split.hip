// 3x3 convolution (pad 1, stride 1) by Winograd's F(4x4, 3x3) in three launches: input transform, the 36 transform positions as ONE
// batched InnerProduct launch, output transform.  conv_wino4.hip's arithmetic (its header: B^T, G, A^T, interpolation points 0, +-1,
// +-2; filter transform in double, rounded once; input and output transforms as fp32 fma chains), unfused.
//
// Why.  In the Winograd domain every transform position p is a plain GEMM  M_p[tile][co] = sum_ci V_p[tile][ci] U_p[co][ci]: the
// tile is the row, the output channel the column, K = Cin -- an InnerProduct.  The fused kernel cuts the small 512-channel maps of the
// trunk (75 x 125: 320 workgroups of 512 slots; 38 x 63: 80) into K ranges that each pay a prologue, a 64 KB slab and a last-arriver
// reduction; fc_mfma_dma16_kernel runs the same contraction as whole-CU workgroups of 320 rows x 128 columns without any cut
// (gemm.hip, BATCH: a 75 x 125 map is 19 x 32 = 608 tiles = two row blocks of 304).  The price is the V and M tensors' trip through
// memory: 36 / 16 = 2.25 floats per input and per output value, written once and read once.
//
// Layouts: V[p][tile][ci] and M[p][tile][co] (p = 6 i + j: row i, column j of the 6 x 6 transform; tile = ty * tiles_x + tx over 4 x 4
// output tiles; channels contiguous), U[p][co][ci].  V and M live in a workspace of the caller's (mnc_conv3x3_wino4_split_ws_bytes): a net sizes it
// with its activation buffers, so nothing is allocated while its launch sequence is captured.
#include "mnc_internal.h"

namespace mnc {

typedef float s4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ s4f fma4(float s, s4f a, s4f b) {
  return s4f{fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z), fmaf(s, a.w, b.w)};
}

// One dimension of B^T d (conv_wino4.hip: f4_bt_col's forms).
__device__ __forceinline__ void bt6(const s4f (&d)[6], s4f (&x)[6]) {
  const s4f a = fma4(-4.f, d[2], d[4]), b = fma4(-4.f, d[1], d[3]), c = d[4] - d[2], e = d[3] - d[1];
  x[0] = fma4(4.f, d[0], fma4(-5.f, d[2], d[4]));
  x[1] = a + b;
  x[2] = a - b;
  x[3] = fma4(2.f, e, c);
  x[4] = fma4(-2.f, e, c);
  x[5] = fma4(4.f, d[1], fma4(-5.f, d[3], d[5]));
}

// One dimension of A^T m.
__device__ __forceinline__ void at6(const s4f (&m)[6], s4f (&y)[4]) {
  const s4f s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
  y[0] = (m[0] + s12) + s34;
  y[1] = fma4(2.f, d34, d12);
  y[2] = fma4(4.f, s34, s12);
  y[3] = fma4(8.f, d34, d12) + m[5];
}

// c8 activations [Cin/8][H][W][8] -> V[36][ntiles][Cin].  One thread per (tile, four channels): lanes walk the channels, so every
// store instruction writes whole rows of V; the 6 x 6 window's pixels outside the image are zero.
__global__ __launch_bounds__(256) void wino4_split_input_kernel(const float* __restrict__ in, float* __restrict__ V, int H, int W, int Cin,
                                                                int tiles_x, int ntiles) {
  const int c4n = Cin >> 2;
  const long total = (long)ntiles * c4n;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % c4n), tile = (int)(idx / c4n);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = 4 * ty - 1, x0 = 4 * tx - 1;
  const float* src = in + (long)(c4 >> 1) * H * W * 8 + (c4 & 1) * 4;
  s4f t[6][6];                                       // B^T d: first dimension down the window's columns
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    s4f d[6], x[6];
    const int xx = x0 + j;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int yy = y0 + i;
      d[i] = s4f{0.f, 0.f, 0.f, 0.f};
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) d[i] = *reinterpret_cast<const s4f*>(src + ((long)yy * W + xx) * 8);
    }
    bt6(d, x);
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i][j] = x[i];
  }
  float* dst = V + (long)tile * Cin + c4 * 4;
  const long pstride = (long)ntiles * Cin;
#pragma unroll
  for (int i = 0; i < 6; ++i) {                      // second dimension along the rows
    s4f x[6];
    bt6(t[i], x);
#pragma unroll
    for (int j = 0; j < 6; ++j) *reinterpret_cast<s4f*>(dst + (long)(6 * i + j) * pstride) = x[j];
  }
}

// M[36][ntiles][Cout] -> Y = A^T M A + bias (ReLU) in the c8 layout; POOL: followed by the Pooling MAX 2x2/2 with Caffe's ceil rule (a
// 4 x 4 tile holds four whole windows; the last window of an odd-sized map is clipped), as conv_wino4.hip's epilogue.  One thread per
// (tile, four channels); lanes 2k and 2k + 1 store the two 16-byte halves of a pixel.
template <int POOL>
__global__ __launch_bounds__(256) void wino4_split_output_kernel(const float* __restrict__ Mt, const float* __restrict__ bias,
                                                                 float* __restrict__ out, int H, int W, int Cout, int relu, int tiles_x,
                                                                 int ntiles) {
  const int c4n = Cout >> 2;
  const long total = (long)ntiles * c4n;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % c4n), tile = (int)(idx / c4n);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int oy = 4 * ty, ox = 4 * tx;
  const float* src = Mt + (long)tile * Cout + c4 * 4;
  const long pstride = (long)ntiles * Cout;
  s4f z[4][6];                                       // A^T M: first dimension down the columns
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    s4f m[6], y[4];
#pragma unroll
    for (int i = 0; i < 6; ++i) m[i] = *reinterpret_cast<const s4f*>(src + (long)(6 * i + j) * pstride);
    at6(m, y);
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i][j] = y[i];
  }
  const s4f bv = *reinterpret_cast<const s4f*>(bias + c4 * 4);
  s4f y[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    at6(z[i], y[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      y[i][j] += bv;
      if (relu) y[i][j] = s4f{fmaxf(y[i][j].x, 0.f), fmaxf(y[i][j].y, 0.f), fmaxf(y[i][j].z, 0.f), fmaxf(y[i][j].w, 0.f)};
    }
  }
  const int cb = c4 >> 1, half = (c4 & 1) * 4;
  if (!POOL) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (oy + i < H && ox + j < W) *reinterpret_cast<s4f*>(out + (((long)cb * H + oy + i) * W + ox + j) * 8 + half) = y[i][j];
  } else {
    const int OH = (H + 1) >> 1, OW = (W + 1) >> 1;
#pragma unroll
    for (int pi = 0; pi < 2; ++pi)
#pragma unroll
      for (int pj = 0; pj < 2; ++pj) {
        const int py = oy + 2 * pi, px = ox + 2 * pj;
        if (py >= H || px >= W) continue;
        s4f best = y[2 * pi][2 * pj];
#pragma unroll
        for (int di = 0; di < 2; ++di)
#pragma unroll
          for (int dj = 0; dj < 2; ++dj)
            if (py + di < H && px + dj < W) {
              const s4f o = y[2 * pi + di][2 * pj + dj];
              best = s4f{fmaxf(best.x, o.x), fmaxf(best.y, o.y), fmaxf(best.z, o.z), fmaxf(best.w, o.w)};
            }
        *reinterpret_cast<s4f*>(out + (((long)cb * OH + (py >> 1)) * OW + (px >> 1)) * 8 + half) = best;
      }
  }
}

// OIHW fp32 [Cout][Cin][3][3] -> U[36][Cout][Cin] = G g G^T, evaluated in double on whole-number 24 G and divided by 576 once
// (pack_conv3x3_wino4_kernel's evaluation: no representation error of 1/6, 1/12, 1/24), rounded once.
__global__ __launch_bounds__(256) void pack_conv3x3_wino4_split_kernel(const float* __restrict__ w, float* __restrict__ U, int Cout,
                                                                       int Cin) {
  const double G[6][3] = {{6.0, 0.0, 0.0}, {-4.0, -4.0, -4.0}, {-4.0, 4.0, -4.0}, {1.0, 2.0, 4.0}, {1.0, -2.0, 4.0}, {0.0, 0.0, 24.0}};
  const long total = (long)Cout * Cin;
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < total; r += (long)gridDim.x * blockDim.x) {
    const float* f = w + r * 9;
    for (int a = 0; a < 6; ++a) {
      double tmp[3];                                 // row a of 24 G f
#pragma unroll
      for (int b = 0; b < 3; ++b) tmp[b] = G[a][0] * (double)f[b] + G[a][1] * (double)f[3 + b] + G[a][2] * (double)f[6 + b];
#pragma unroll
      for (int b = 0; b < 6; ++b)
        U[(long)(6 * a + b) * total + r] = (float)((tmp[0] * G[b][0] + tmp[1] * G[b][1] + tmp[2] * G[b][2]) / 576.0);
    }
  }
}

bool wino4_split_supported(int H, int W, int Cin, int Cout) {
  return H > 0 && W > 0 && Cin > 0 && Cin % 32 == 0 && Cout > 0 && Cout % 32 == 0 &&
         36.0 * cdiv(H, 4) * (double)cdiv(W, 4) * (Cin > Cout ? Cin : Cout) * 4.0 < 2.0e9;
}

// Which layers the throughput plan runs in the split form (WINO_SPLIT = 1): see DESIGN.md section 4 and profiles/wino_split.txt.
bool wino4_split_selected(const mnc_ctx* ctx, int H, int W, int Cin, int Cout) {
  const int v = tune(ctx, T_WINO_SPLIT, kWinoSplitDefault);
  if (v == 0 || !wino4_split_supported(H, W, Cin, Cout)) return false;
  if (v == 2) return true;
  if (plan_latency(ctx)) return false;               // three dependent launches per layer: not for one image alone
  return wino4_split_plan_channels(Cin, Cout) && cdiv(H, 4) * cdiv(W, 4) >= 304;
}

static size_t wino4_split_v_bytes(int H, int W, int Cin) {
  return ((size_t)36 * cdiv(W, 4) * cdiv(H, 4) * Cin * 4 + 255) & ~(size_t)255;
}

static int wino4_split_impl(mnc_ctx* ctx, const float* d_in, const float* d_u, const float* d_bias, float* d_out, void* d_ws, int H,
                            int W, int Cin, int Cout, int relu, int pool) {
  MNC_REQUIRE(ctx && d_in && d_u && d_bias && d_out && d_ws, "mnc_conv3x3_wino4_split: null pointer");
  MNC_REQUIRE((reinterpret_cast<uintptr_t>(d_ws) & 15) == 0, "mnc_conv3x3_wino4_split: workspace not 16-byte aligned");
  MNC_REQUIRE(wino4_split_supported(H, W, Cin, Cout),
              "mnc_conv3x3_wino4_split: unsupported shape H=%d W=%d Cin=%d Cout=%d (need Cin%%32==0, Cout%%32==0)", H, W, Cin, Cout);
  const int tiles_x = cdiv(W, 4), ntiles = tiles_x * cdiv(H, 4);
  float* V = (float*)d_ws;
  float* Mt = (float*)((char*)d_ws + wino4_split_v_bytes(H, W, Cin));
  const double flops = 2.0 * H * W * 9.0 * Cin * Cout;           // ALGORITHMIC work of the convolution (direct form), as wino4_impl books it
  const double out_px = pool ? (double)((H + 1) / 2) * ((W + 1) / 2) : (double)H * W;
  const double bytes = 4.0 * ((double)H * W * Cin + out_px * Cout + 9.0 * Cin * Cout);
  LaunchScope ls(ctx, "conv3x3_wino4_mfma", flops, bytes);
  const long in_items = (long)ntiles * (Cin >> 2), out_items = (long)ntiles * (Cout >> 2);
  hipLaunchKernelGGL(wino4_split_input_kernel, dim3((unsigned)((in_items + 255) / 256)), dim3(256), 0, ctx->stream, d_in, V, H, W, Cin,
                     tiles_x, ntiles);
  int rc = fc_batch_launch(ctx, V, (long)ntiles * Cin, d_u, (long)Cout * Cin, Mt, (long)ntiles * Cout, 36, ntiles, Cout, Cin, Cout);
  if (rc) {
    (void)ls.finish("conv3x3_wino4_split");          // (closes the profile record)
    return rc;
  }
  if (pool)
    hipLaunchKernelGGL(wino4_split_output_kernel<1>, dim3((unsigned)((out_items + 255) / 256)), dim3(256), 0, ctx->stream, Mt, d_bias,
                       d_out, H, W, Cout, relu, tiles_x, ntiles);
  else
    hipLaunchKernelGGL(wino4_split_output_kernel<0>, dim3((unsigned)((out_items + 255) / 256)), dim3(256), 0, ctx->stream, Mt, d_bias,
                       d_out, H, W, Cout, relu, tiles_x, ntiles);
  return ls.finish("conv3x3_wino4_split");
}

}  // namespace mnc

using namespace mnc;

extern "C" {

int mnc_pack_conv3x3_wino4_split(mnc_ctx* ctx, const float* d_oihw, float* d_packed, int Cout, int Cin) {
  MNC_REQUIRE(ctx && d_oihw && d_packed && Cin > 0 && Cin % 32 == 0 && Cout > 0 && Cout % 32 == 0,
              "mnc_pack_conv3x3_wino4_split: bad argument (Cin%%32==0, Cout%%32==0)");
  LaunchScope ls(ctx, "pack_conv3x3_wino4_split");
  long g = ((long)Cout * Cin + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(pack_conv3x3_wino4_split_kernel, dim3((int)g), dim3(256), 0, ctx->stream, d_oihw, d_packed, Cout, Cin);
  return ls.finish("pack_conv3x3_wino4_split_kernel");
}

size_t mnc_conv3x3_wino4_split_ws_bytes(int H, int W, int Cin, int Cout) {
  if (!wino4_split_supported(H, W, Cin, Cout)) return 0;
  return wino4_split_v_bytes(H, W, Cin) + (size_t)36 * cdiv(W, 4) * cdiv(H, 4) * Cout * 4;
}

int mnc_conv3x3_wino4_split_selected(mnc_ctx* ctx, int H, int W, int Cin, int Cout) {
  return ctx && wino4_split_selected(ctx, H, W, Cin, Cout) ? 1 : 0;
}

int mnc_conv3x3_wino4_split(mnc_ctx* ctx, const float* d_in, const float* d_u, const float* d_bias, float* d_out, void* d_ws, int H,
                            int W, int Cin, int Cout, int relu) {
  return wino4_split_impl(ctx, d_in, d_u, d_bias, d_out, d_ws, H, W, Cin, Cout, relu, 0);
}

int mnc_conv3x3_wino4_split_pool(mnc_ctx* ctx, const float* d_in, const float* d_u, const float* d_bias, float* d_out_pooled,
                                 void* d_ws, int H, int W, int Cin, int Cout, int relu) {
  MNC_REQUIRE(H >= 2 && W >= 2, "mnc_conv3x3_wino4_split_pool: map %dx%d too small for MAX 2x2/2", H, W);
  return wino4_split_impl(ctx, d_in, d_u, d_bias, d_out_pooled, d_ws, H, W, Cin, Cout, relu, 1);
}

}  // extern "C"
