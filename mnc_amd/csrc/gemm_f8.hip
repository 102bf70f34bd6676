// InnerProduct on the block-scaled fp8 matrix instruction of gfx950 (the "f8" math mode): OCP e4m3fn operands, fp32 accumulation.
//
// Numerics (stated in plain numpy in mnc_amd/f8.py; these kernels follow it bit for bit except for the summation order):
//   * every operand ROW carries one power-of-two scale 2^e: amax = f * 2^p (f in [0.5, 1)), e = p - 9 when f <= 0.875, else p - 8,
//     clamped to [-64, 64], 0 for a zero row -- the scaled row's maximum lies in (224, 448]; codes = e4m3(x * 2^-e), nearest even;
//   * v_mfma_scale_f32_32x32x64_f8f6f4 multiplies the codes with BOTH hardware block scales at 1.0 (E8M0 127); the row exponents are
//     applied in the epilogue, after all K ranges are summed: out = act(ldexp(acc, ea[m] + ew[n]) + bias[n]) -- exact scaling.
//   * weights are quantised per output row once at load (mnc_pack_fc_f8), activations per RoI row on every call
//     (mnc_fc_pack_act_f8: from fp32 rows, or from the fp16 stage-major panel the producers of the f16 mode write).
//
// Product kernel: fc_lowp_dma_kernel's structure (gemm_x3.hip) with one-byte operands.  A stage is 128 bytes per row = 128 K values =
// two 32x32x64 MFMA steps; 256-column tiles, eight waves (2 along M x 4 along N), operand panels global -> LDS by LDS-DMA into the
// XOR-swizzled row images (row r keeps its 16-byte chunk c in slot c ^ ((r >> 1) & 7)), double-buffered.  MFMA shape: 32x32x64 and
// 16x16x128 run the same cycles per flop (MI355X_MICROARCH.md: twice the cycles of the bf16 form of the same M x N at 4x the K) and
// read the same fragment bytes per stage ((rows + columns) x 128 B per wave either way: 28 ds_read_b128); 32x32x64 issues half as
// many MFMAs and keeps fc_lowp_dma_kernel's accumulator map and epilogue.
// Operand lane map: lane (j = lane & 31, h = lane >> 5) hands the instruction 32 bytes of row j; both operands take the SAME 32 bytes
// of a K step (bytes [32 h, 32 h + 32) of its 64), so whichever K index the hardware gives element i of half h, it is the same for A
// and B and the step sums every K value once -- tests/test_gpu_fc_f8.py checks rows, columns and coverage with exact integer data
// (identity-like A against an asymmetric W).
#include "fc_f8_plan.h"
#include "mnc_internal.h"

namespace mnc {

typedef float f8_f32x16 __attribute__((ext_vector_type(16)));
typedef int f8_i32x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float f8_act(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return 1.0f / (1.0f + expf(-v));
  return v;
}

// ---- quantisers ------------------------------------------------------------------------------------------------------------
// fp32 -> OCP e4m3fn code, nearest even; |y| >= 448 saturates at +-448 (0x7E), NaN -> 0x7F; the sign of zero is kept.
__device__ __forceinline__ unsigned f8_encode(float y) {
  const unsigned b = __float_as_uint(y), s = (b >> 24) & 0x80u, ab = b & 0x7FFFFFFFu;
  unsigned code;
  if (ab > 0x7F800000u) code = 0x7Fu;
  else if (ab >= 0x43E00000u) code = 0x7Eu;                                  // 448
  else if (ab < 0x3C800000u) code = (unsigned)rintf(fabsf(y) * 512.0f);      // below 2^-6: multiples of 2^-9 (8 = the smallest normal)
  else code = ((ab + 0x7FFFFu + ((ab >> 20) & 1u)) >> 20) - (120u << 3);     // 23 -> 3 mantissa bits on the fp32 bits, bias 127 -> 7
  return code | s;
}
// the row exponent from the bits of amax (>= 0, finite)
__device__ __forceinline__ int f8_row_exp(unsigned ab) {
  if (ab == 0) return 0;
  const int be = (int)(ab >> 23);
  if (be == 0) return -64;                                   // an fp32 subnormal: far below the clamp
  const int p = be - 126;                                    // amax = f * 2^p, f = 1.mantissa / 2
  const int e = (ab & 0x7FFFFFu) <= 0x600000u ? p - 9 : p - 8;       // f <= 0.875
  return e < -64 ? -64 : e > 64 ? 64 : e;
}

// One workgroup per row (padding rows of the last tile included: zero codes, exponent 0).  SRC 0: fp32 rows [rows][K]; SRC 1: the
// fp16 stage-major panel [K/64][in_stride][64] (format 1), whose row is spread over K/64 stages.  Two passes over the row: amax over
// the finite values (an integer maximum of the magnitudes' bits through LDS -- no float atomics), then the codes, written stage-major with 128-value
// stages: out[((tile * K/128 + k/128) * tile_rows + r) * 128 + k % 128], row = tile * tile_rows + r.
template <int SRC>
__global__ __launch_bounds__(256) void f8_quant_rows_kernel(const void* __restrict__ in, long in_stride, unsigned char* __restrict__ out,
                                                            int* __restrict__ exps, int rows, int K, int tile_rows) {
  __shared__ unsigned s_amax;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int tile = row / tile_rows, r = row - tile * tile_rows;
  const int groups = K >> 3;                                 // 8 values each
  const long S = K >> 7;
  auto load8 = [&](int g, float* x) {
    if (SRC == 0) {
      const float4* p = reinterpret_cast<const float4*>((const float*)in + (long)row * K + (long)g * 8);
      const float4 a = p[0], b = p[1];
      x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
      typedef _Float16 h8 __attribute__((ext_vector_type(8)));
      const uint4 u = ((const uint4*)in)[((long)(g >> 3) * in_stride + row) * 8 + (g & 7)];
      const h8 h = __builtin_bit_cast(h8, u);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = (float)h[e];
    }
  };
  auto dst = [&](int g) {
    const long k = (long)g * 8;
    return reinterpret_cast<uint2*>(out + (((long)tile * S + (k >> 7)) * tile_rows + r) * 128 + (k & 127));
  };
  if (row >= rows) {                                         // (block-uniform)
    for (int g = tid; g < groups; g += 256) *dst(g) = make_uint2(0u, 0u);
    if (tid == 0) exps[row] = 0;
    return;
  }
  if (tid == 0) s_amax = 0u;
  __syncthreads();
  unsigned m = 0u;
  for (int g = tid; g < groups; g += 256) {
    float x[8];
    load8(g, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned ab = __float_as_uint(x[e]) & 0x7FFFFFFFu;
      if (ab < 0x7F800000u && ab > m) m = ab;                // finite values only (f8.py): inf saturates, NaN stays NaN
    }
  }
  atomicMax(&s_amax, m);
  __syncthreads();
  const int e = f8_row_exp(s_amax);
  if (tid == 0) exps[row] = e;
  const float scale = __uint_as_float((unsigned)(127 - e) << 23);      // 2^-e, a normal fp32 for every e of the clamp
  for (int g = tid; g < groups; g += 256) {
    float x[8];
    load8(g, x);
    unsigned lo = 0u, hi = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      lo |= f8_encode(x[i] * scale) << (8 * i);
      hi |= f8_encode(x[4 + i] * scale) << (8 * i);
    }
    *dst(g) = make_uint2(lo, hi);
  }
}

// ---- product ---------------------------------------------------------------------------------------------------------------
// Workgroup = 32 kMT rows x 256 columns x one K range; wave (wm, wn) owns kMT/2 row tiles x columns [64 wn, 64 wn + 64).  The
// accumulators stay in architectural registers ("+v"; see fc_lowp_dma_kernel: a 512-thread workgroup leaves a wave 256 registers of the
// unified file, and MFMA reads and writes them at the same rate as AGPRs on gfx950).  One fragment set (56 registers beside 160
// accumulators at kMT = 10): two waves share each SIMD, one wave's fragment reads run under its partner's MFMAs.
// fused != 0 (one K range): the epilogue applies exponents, bias and activation and writes out (and osm).  Otherwise the raw sums go
// to part[range][M][N] and f8_reduce_kernel finishes them.
// DEC != 0 (products shorter than four stages, fc_f8_plan.h; 64-row workgroups only): the same panels, fragments and epilogue, but the
// codes are decoded to fp16 in registers -- exactly: every e4m3 value is an fp16 value -- and multiplied on v_mfma_f32_32x32x16_f16,
// four steps of 16 K values per 64.  The scaled instruction does not add its products fp32-wise: inside a lane's group of K values a
// product 2^16 below the largest one is dropped (measured; the f16 and bf16 forms keep it down to 2^-22), an error of up to 2^-16 of
// sum |qa||qw| whatever K is -- more than an fp32 summation of fewer than 512 terms may cost, and nothing against one over the
// thousands of terms this kernel is made for.
typedef _Float16 f8_f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f8_f16x8 __attribute__((ext_vector_type(8)));
// 4 codes -> 4 halves: sign and the 7 low bits moved to the fp16 fields give the value / 2^8 (fp16's exponent bias is 15, e4m3's 7;
// subnormal codes land on fp16 subnormals, also 2^8 too small); the product by 256 is exact.
__device__ __forceinline__ uint2 f8_to_f16x4(unsigned w) {
  const unsigned lo = ((w & 0x7Fu) << 7) | ((w & 0x80u) << 8) | ((w & 0x7F00u) << 15) | ((w & 0x8000u) << 16);
  const unsigned v = w >> 16;
  const unsigned hi = ((v & 0x7Fu) << 7) | ((v & 0x80u) << 8) | ((v & 0x7F00u) << 15) | ((v & 0x8000u) << 16);
  const f8_f16x2 k = {(_Float16)256.0f, (_Float16)256.0f};
  return make_uint2(__builtin_bit_cast(unsigned, __builtin_bit_cast(f8_f16x2, lo) * k),
                    __builtin_bit_cast(unsigned, __builtin_bit_cast(f8_f16x2, hi) * k));
}
template <int kMT, int DEC = 0>
__global__ __launch_bounds__(512) void fc_f8_kernel(const uint4* __restrict__ Aq, const uint4* __restrict__ Wq, const int* __restrict__ aexp,
                                                   const int* __restrict__ wexp, const float* __restrict__ bias, float* __restrict__ out,
                                                   float* __restrict__ part, _Float16* __restrict__ osm, long osm_rows, int M, int N, int K,
                                                   int ldc, int kper, int act, int fused, int tn_, int splits_, int tm_, int mstride) {
  constexpr int kBM = 32 * kMT;
  constexpr int kRows = kBM + kF8BN;                 // operand rows per stage: activations, then weights
  constexpr int kBuf = kRows * 128;                  // bytes per stage buffer
  constexpr int kPieces = kRows / 8;                 // 1 KB DMA pieces per stage (8 rows each)
  constexpr int kPer = kPieces / 8;                  // per wave
  constexpr int kPerA = kBM / 64;                    // of them activation pieces
  constexpr int TR = kMT / 2;                        // row tiles per wave
  static_assert(kMT % 2 == 0 && kPieces % 8 == 0 && kBM % 64 == 0, "wave grid / whole pieces per operand");
  extern __shared__ __attribute__((aligned(1024))) char s_f8[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave & 3, wm = wave >> 2;
  const int j = lane & 31, kb = lane >> 5;
  int bn, split, bmz;
  xcd_decode(blockIdx.x, tn_, splits_, tm_, bn, split, bmz);
  const int n0 = bn * kF8BN, m0 = bmz * kBM;
  const int S = K / kF8Stage;
  const int kbeg = split * kper, kend = min(K, kbeg + kper);
  const int stage0 = kbeg / kF8Stage, nstages = (kend - kbeg) / kF8Stage;
  const int mrows = min(M - m0, kBM);
  const int mtiles = (mrows + 31) >> 5;

  // Piece p = wave + 8 i covers buffer bytes [1024 p, 1024 p + 1024): lane L fills slot L & 7 of row r = 8 p + (L >> 3), i.e. it
  // fetches chunk (L & 7) ^ ((r >> 1) & 7) of that row, and (r >> 1) & 7 = 4 (wave & 1) + (L >> 4) for every i.  r = r0 + 64 i:
  // pieces i < kPerA are activation rows (stage stride mstride x 128 B; rows past M re-read the last valid row and are never stored),
  // the others rows r0 + 64 k of this column tile's weight panel (stage stride 256 x 128 B; the panel is padded to whole tiles).
  const int r0 = wave * 8 + (lane >> 3);
  const int cch = (lane & 7) ^ ((wave & 1) * 4 + (lane >> 4));
  const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) char*)s_f8;
  typedef int i32x4d __attribute__((ext_vector_type(4)));
  auto make_rsrc = [](const uint4* base) {
    const unsigned long a = (unsigned long)base;
    i32x4d r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xFFFFu));
    r.z = 0x70000000;                                // (no lane relies on the range check: rows and stages are clamped)
    r.w = 0x00020000;
    return r;
  };
  int voff_a[kPerA];
#pragma unroll
  for (int i = 0; i < kPerA; ++i) voff_a[i] = min(r0 + 64 * i, mrows - 1) * 128 + cch * 16;
  const int voff_w = r0 * 128 + cch * 16;            // + k x 8 KB
  // the stage is the copy's SCALAR offset: st x mstride x 128 bytes into the activations (< 4 GB: the launcher checks), st x 32 KB
  // into the weight panel
  const i32x4d ra = make_rsrc(Aq + (((long)stage0 * mstride + m0) << 3));
  const i32x4d rw = make_rsrc(Wq + (((long)bn * S + stage0) << 11));
  const unsigned a_stage_bytes = (unsigned)mstride * 128u;
  auto dma_stage = [&](int s, int buf_byte) {
    const unsigned st = (unsigned)min(s, nstages - 1);  // past the end: the last stage once more, never multiplied
    const unsigned so_a = st * a_stage_bytes, so_w = st << 15;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const unsigned l = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)buf_byte + (unsigned)(wave + 8 * i) * 1024u);
      if (i < kPerA) {
        asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff_a[i]), "s"(ra), "s"(so_a), "s"(l) : "memory");
      } else {
        const int vo = voff_w + (i - kPerA) * 8192;
        asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(rw), "s"(so_w), "s"(l) : "memory");
      }
    }
  };
  auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  f8_f32x16 acc[TR][2];
#pragma unroll
  for (int t = 0; t < TR; ++t)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][c][e] = 0.f;

  // MFMA step q (64 K values, 2 per stage) is chunks 4 q .. 4 q + 3 of a row; lane half kb takes chunks 4 q + 2 kb and + 1 (32 bytes).
  // Tile offsets (32 rows = 4 KB) leave (r >> 1) & 7 = (j >> 1) & 7 unchanged.  Byte offsets inside a buffer.
  const int swz = (j >> 1) & 7;
  int coff[2][2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < 2; ++i) coff[q][i] = ((4 * q + 2 * kb + i) ^ swz) * 16;
  const int a_row = (wm * TR * 32 + j) * 128, b_row = (kBM + wn * 64 + j) * 128;
  struct Frags { f8_i32x8 a[TR]; f8_i32x8 b[2]; };
  auto read_frag = [&](const char* row, int q) {
    const uint4 lo = *reinterpret_cast<const uint4*>(row + coff[q][0]), hi = *reinterpret_cast<const uint4*>(row + coff[q][1]);
    f8_i32x8 v = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    return v;
  };
  auto read_frags = [&](int buf_byte, int q, Frags& f) {
    const char* base = s_f8 + buf_byte;
    f.b[0] = read_frag(base + b_row, q);
    f.b[1] = read_frag(base + b_row + 4096, q);
#pragma unroll
    for (int t = 0; t < TR; ++t) f.a[t] = read_frag(base + a_row + t * 4096, q);
  };
  // both block scales 1.0: E8M0 127 in every byte of the scale operands, so the byte the instruction selects does not matter
  constexpr int kOne = 0x7F7F7F7F;
  auto dec8 = [](const f8_i32x8& v, int s) {         // codes 8 s .. 8 s + 7 of the lane's 32 as one fp16 fragment
    const uint2 x = f8_to_f16x4((unsigned)v[2 * s]), y = f8_to_f16x4((unsigned)v[2 * s + 1]);
    return __builtin_bit_cast(f8_f16x8, make_uint4(x.x, x.y, y.x, y.y));
  };
  auto mfmas = [&](const Frags& f) {
    if constexpr (DEC != 0) {
      static_assert(DEC == 0 || kMT == 2, "the decoding build is the 64-row one");
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const f8_f16x8 b0 = dec8(f.b[0], s), b1 = dec8(f.b[1], s);
#pragma unroll
        for (int t = 0; t < TR; ++t) {
          const f8_f16x8 a = dec8(f.a[t], s);
          acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b0, acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b1, acc[t][1], 0, 0, 0);
        }
      }
      return;
    }
#pragma unroll
    for (int t = 0; t < TR; ++t)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        acc[t][c] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(f.a[t], f.b[c], acc[t][c], 0, 0, 0, kOne, 0, kOne);
  };
  auto pin_acc = [&]() {
#pragma unroll
    for (int t = 0; t < TR; ++t)
#pragma unroll
      for (int c = 0; c < 2; ++c) asm volatile("" : "+v"(acc[t][c]));
  };

  if (nstages > 0) {
    dma_stage(0, 0);
    dma_stage(1, kBuf);
    dma_wait();
    __syncthreads();
    int cur = 0;                                     // byte offset of the buffer stage s sits in
    Frags f;
    for (int s = 0; s < nstages; ++s) {
      read_frags(cur, 0, f);
      mfmas(f);
      read_frags(cur, 1, f);
      pin_acc();
      dma_wait();                                    // stage s + 1 has landed ...
      __syncthreads();                               // ... for every wave, and every wave holds its last fragments of buffer `cur`
      __builtin_amdgcn_sched_barrier(0);
      dma_stage(s + 2, cur);                         // refill the buffer just released: a whole stage to land
      __builtin_amdgcn_sched_barrier(0);
      mfmas(f);                                      // the last step
      pin_acc();
      cur = kBuf - cur;
    }
    dma_wait();                                      // the copies issued by the last two stages have landed before the LDS is released
    __syncthreads();
  }

#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int n = n0 + wn * 64 + c * 32 + j;
    if (n >= N) continue;
    const float bv = fused ? bias[n] : 0.f;
    const int en = fused ? wexp[n] : 0;
#pragma unroll
    for (int t = 0; t < TR; ++t) {
      const int tile = wm * TR + t;
      if (tile < mtiles) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = m0 + tile * 32 + (e & 3) + 8 * (e >> 2) + 4 * kb;
          if (m < M) {
            if (fused) {
              const float v = f8_act(ldexpf(acc[t][c][e], aexp[m] + en) + bv, act);
              out[(long)m * ldc + n] = v;
              if (osm) osm[((long)(n >> 6) * osm_rows + m) * 64 + (n & 63)] = (_Float16)v;
            } else {
              part[((long)split * M + m) * N + n] = acc[t][c][e];
            }
          }
        }
      }
    }
  }
}

// The K ranges' partial sums added in range order (the same bits from run to run), then exponents, bias and activation; the rows a
// second time as fp16 in the stage-major format 1 of the next InnerProduct when osm != nullptr.
__global__ void f8_reduce_kernel(const float* __restrict__ part, const int* __restrict__ aexp, const int* __restrict__ wexp,
                                 const float* __restrict__ bias, float* __restrict__ out, _Float16* __restrict__ osm, long osm_rows,
                                 int M, int N, int ldc, int splits, int act) {
  const long total = (long)M * N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / N), n = (int)(i - (long)m * N);
    float s = part[i];
    for (int sp = 1; sp < splits; ++sp) s += part[sp * total + i];
    const float v = f8_act(ldexpf(s, aexp[m] + wexp[n]) + bias[n], act);
    out[(long)m * ldc + n] = v;
    if (osm) osm[((long)(n >> 6) * osm_rows + m) * 64 + (n & 63)] = (_Float16)v;
  }
}

static int f8_quant_launch(mnc_ctx* ctx, const char* name, const float* d_rows, const void* d_sm, long sm_stride, void* d_q, int* d_exp,
                           int rows, int K, int tile_rows, int tiles) {
  LaunchScope ls(ctx, name, 0.0, (d_rows ? 9.0 : 5.0) * rows * (double)K);
  if (d_rows)
    hipLaunchKernelGGL(f8_quant_rows_kernel<0>, dim3(tiles * tile_rows), dim3(256), 0, ctx->stream, (const void*)d_rows, 0L,
                       (unsigned char*)d_q, d_exp, rows, K, tile_rows);
  else
    hipLaunchKernelGGL(f8_quant_rows_kernel<1>, dim3(tiles * tile_rows), dim3(256), 0, ctx->stream, d_sm, sm_stride, (unsigned char*)d_q,
                       d_exp, rows, K, tile_rows);
  return ls.finish("f8_quant_rows_kernel");
}

// The launcher behind mnc_fc_f8 / mnc_fc_f8_ex.  Activations: fp32 rows (d_a), an fp16 stage-major panel (d_a_sm, m_stride rows per
// stage) -- both quantised into the scratch arena first -- or codes and exponents made by mnc_fc_pack_act_f8 (d_q, d_aexp).
static int fc_f8_run(mnc_ctx* ctx, const char* what, const float* d_a, const void* d_a_sm, const void* d_q, const int* d_aexp, int mstride,
                     const void* d_w_packed, const int* d_wexp, const float* d_bias, float* d_out, int M, int N, int K, int ldc, int act,
                     void* d_osm) {
  if (M == 0) return MNC_OK;
  const bool quantise_here = d_q == nullptr;
  const F8Plan p = fc_f8_plan(M, N, K, mstride, quantise_here, ctx->tune);
  MNC_REQUIRE(p.in_range, "%s: a K range of %d stages over %d rows per stage is beyond the copies' 32-bit offset", what, p.kper / kF8Stage,
              quantise_here ? M : mstride);
  int rc = ensure_scratch(ctx, p.part_bytes + p.q_bytes + p.exp_bytes);
  if (rc) return rc;
  float* part = p.splits > 1 ? (float*)ctx->scratch.p : nullptr;
  if (quantise_here) {
    char* q = (char*)ctx->scratch.p + p.part_bytes;
    int* ex = (int*)(q + p.q_bytes);
    rc = f8_quant_launch(ctx, "fc_f8_quantise", d_a, d_a_sm, mstride, q, ex, M, K, M, 1);
    if (rc) return rc;
    d_q = q;
    d_aexp = ex;
    mstride = M;
  }
  {
    LaunchScope ls(ctx, "fc_f8", 2.0 * M * (double)N * K, (double)N * K + (double)M * K + 4.0 * (double)M * N);
    const int fused = p.splits == 1 ? 1 : 0;
#define MNC_F8_LAUNCH(MT, DEC)                                                                                                            \
  do {                                                                                                                                 \
    constexpr int lds = 2 * (32 * MT + kF8BN) * 128;                                                                                   \
    MNC_HIP_TRY((lds_limit_once<fc_f8_kernel<MT, DEC>>(ctx->device, lds)));                                                  \
    hipLaunchKernelGGL((fc_f8_kernel<MT, DEC>), dim3(p.tn * p.splits * p.tm), dim3(512), lds, ctx->stream, (const uint4*)d_q,          \
                       (const uint4*)d_w_packed, d_aexp, d_wexp, d_bias, d_out, part, fused ? (_Float16*)d_osm : (_Float16*)nullptr,   \
                       (long)M, M, N, K, ldc, p.kper, act, fused, p.tn, p.splits, p.tm, mstride);                                      \
  } while (0)
    if (p.decode) MNC_F8_LAUNCH(2, 1);
    else if (p.mt == 2) MNC_F8_LAUNCH(2, 0);
    else MNC_F8_LAUNCH(10, 0);
#undef MNC_F8_LAUNCH
    rc = ls.finish("fc_f8_kernel");
    if (rc) return rc;
  }
  if (p.splits > 1) {
    LaunchScope ls(ctx, "fc_f8_reduce", 0.0, 4.0 * ((double)p.splits + 1.0) * M * N);
    long g = ((long)M * N + 255) / 256;
    if (g > 65536) g = 65536;
    hipLaunchKernelGGL(f8_reduce_kernel, dim3((int)g), dim3(256), 0, ctx->stream, (const float*)part, d_aexp, d_wexp, d_bias, d_out,
                       (_Float16*)d_osm, (long)M, M, N, ldc, p.splits, act);
    return ls.finish("f8_reduce_kernel");
  }
  return MNC_OK;
}

}  // namespace mnc

using namespace mnc;

extern "C" {

size_t mnc_pack_fc_f8_bytes(int N, int K) { return N > 0 && K > 0 ? fc_f8_packed_bytes(N, K) : 0; }

int mnc_pack_fc_f8(mnc_ctx* ctx, const float* d_w, void* d_packed, int* d_wexp, int N, int K) {
  MNC_REQUIRE(ctx && d_w && d_packed && d_wexp && N > 0 && K > 0 && K % kF8Stage == 0, "mnc_pack_fc_f8: bad argument (K%%128==0)");
  return f8_quant_launch(ctx, "pack_fc_f8", d_w, nullptr, 0, d_packed, d_wexp, N, K, kF8BN, cdiv(N, kF8BN));
}

int mnc_fc_pack_act_f8(mnc_ctx* ctx, const float* d_a, const void* d_a_sm, int m_stride, void* d_q, int* d_aexp, int M, int K) {
  MNC_REQUIRE(ctx && (d_a != nullptr) != (d_a_sm != nullptr) && d_q && d_aexp, "mnc_fc_pack_act_f8: null pointer / both inputs");
  MNC_REQUIRE(M > 0 && K > 0 && K % kF8Stage == 0 && (d_a || m_stride >= M), "mnc_fc_pack_act_f8: unsupported shape M=%d (stride %d) K=%d (need K%%128==0)",
              M, m_stride, K);
  return f8_quant_launch(ctx, "fc_f8_quantise", d_a, d_a_sm, m_stride, d_q, d_aexp, M, K, M, 1);
}

int mnc_fc_f8(mnc_ctx* ctx, const float* d_a, const void* d_w_packed, const int* d_wexp, const float* d_bias, float* d_out, int M, int N,
              int K, int ldc, int act) {
  MNC_REQUIRE(ctx && d_a && d_w_packed && d_wexp && d_bias && d_out, "mnc_fc_f8: null pointer");
  MNC_REQUIRE(M >= 0 && N > 0 && K > 0 && K % kF8Stage == 0 && ldc >= N && act >= 0 && act <= 2,
              "mnc_fc_f8: unsupported shape M=%d N=%d K=%d ldc=%d act=%d (need K%%128==0)", M, N, K, ldc, act);
  return fc_f8_run(ctx, "mnc_fc_f8", d_a, nullptr, nullptr, nullptr, M, d_w_packed, d_wexp, d_bias, d_out, M, N, K, ldc, act, nullptr);
}

int mnc_fc_f8_ex(mnc_ctx* ctx, const float* d_a, const void* d_a_sm, int m_stride, const void* d_w_packed, const int* d_wexp,
                 const float* d_bias, float* d_out, int M, int N, int K, int ldc, int act, void* d_out_sm, int out_sm_fmt) {
  MNC_REQUIRE(ctx && (d_a != nullptr) != (d_a_sm != nullptr) && d_w_packed && d_wexp && d_bias && d_out, "mnc_fc_f8_ex: null pointer / both inputs");
  MNC_REQUIRE(M >= 0 && (d_a || m_stride >= M) && N > 0 && K > 0 && K % kF8Stage == 0 && ldc >= N && act >= 0 && act <= 2 &&
                  (!d_out_sm || (out_sm_fmt == 1 && N % 64 == 0)),
              "mnc_fc_f8_ex: unsupported shape M=%d N=%d K=%d ldc=%d act=%d out_sm_fmt=%d (need K%%128==0; the second output is format 1)", M,
              N, K, ldc, act, out_sm_fmt);
  return fc_f8_run(ctx, "mnc_fc_f8_ex", d_a, d_a_sm, nullptr, nullptr, d_a ? M : m_stride, d_w_packed, d_wexp, d_bias, d_out, M, N, K, ldc, act,
                   d_out_sm);
}

int mnc_fc_f8_pre(mnc_ctx* ctx, const void* d_q, const int* d_aexp, int m_stride, const void* d_w_packed, const int* d_wexp,
                  const float* d_bias, float* d_out, int M, int N, int K, int ldc, int act) {
  MNC_REQUIRE(ctx && d_q && d_aexp && d_w_packed && d_wexp && d_bias && d_out, "mnc_fc_f8_pre: null pointer");
  MNC_REQUIRE(M >= 0 && m_stride >= M && N > 0 && K > 0 && K % kF8Stage == 0 && ldc >= N && act >= 0 && act <= 2,
              "mnc_fc_f8_pre: unsupported shape M=%d (stride %d) N=%d K=%d ldc=%d act=%d (need K%%128==0)", M, m_stride, N, K, ldc, act);
  return fc_f8_run(ctx, "mnc_fc_f8_pre", nullptr, nullptr, d_q, d_aexp, m_stride, d_w_packed, d_wexp, d_bias, d_out, M, N, K, ldc, act, nullptr);
}

}  // extern "C"
