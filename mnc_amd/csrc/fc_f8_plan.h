// Launch plan of the e4m3 InnerProduct (gemm_f8.hip: mnc_fc_f8, mnc_fc_f8_ex) as a pure function of the call's shape and the
// context's tuning array, like fc_plan.h: tile height, column tiles, K ranges, scratch bytes.  The number of K ranges fixes how the
// fp32 partial sums are grouped and so the last bits of the result.  No HIP include: tests/test_f8_host.py compiles this header for
// the host.
#pragma once
#include "fc_plan.h"

namespace mnc {

constexpr int kF8Stage = 128;       // K values (= bytes per row) of one stage: two 32x32x64 MFMA steps
constexpr int kF8BN = 256;          // columns per workgroup, the weight panel's tile height
constexpr int kF8MinStages = 4;     // a K range is at least 512 K values long
constexpr int kF8ScaledStages = 4;  // products of fewer stages decode to fp16 (below)

struct F8Plan {
  int mt = 0;                       // 32-row tiles per workgroup: 2 (M <= 64, and every decoding product) or 10
  bool decode = false;              // fewer than kF8MinStages stages: the codes decoded to fp16, fp16 MFMA (fp32-wise summation)
  int tn = 0, tm = 0;               // column tiles of 256 and row blocks of 32 mt
  int splits = 1, kper = 0;         // K ranges and K values per range (a multiple of 128; the last range may be shorter)
  size_t part_bytes = 0;            // [range][M][N] fp32 partial sums at the head of the scratch arena (0 with one range)
  size_t q_bytes = 0;               // behind them: the activations' codes, [K/128][M][128] bytes (0: they arrive quantised)
  size_t exp_bytes = 0;             // behind those: the activation rows' exponents, M int32
  bool in_range = true;             // a range's stages x row stride x 128 bytes fit the copies' 32-bit scalar offset
};

// packed weights: cdiv(N, 256) column tiles x K/128 stages x 256 rows x 128 bytes; exponents: one int32 per padded row
inline size_t fc_f8_packed_bytes(int N, int K) { return (size_t)cdiv(N, kF8BN) * kF8BN * (size_t)K; }
inline size_t fc_f8_exp_count(int N) { return (size_t)cdiv(N, kF8BN) * kF8BN; }

// mstride: rows per stage of the activation panel the product kernel reads (M when the codes are made here).  quantise_here: the
// activations arrive as fp32 rows or as an fp16 panel and are quantised into the scratch arena first.
inline F8Plan fc_f8_plan(int M, int N, int K, int mstride, bool quantise_here, const int* t) {
  F8Plan p;
  // 64-row workgroups up to 64 rows (half the LDS, a fifth of the MFMAs on clamped rows); otherwise 320-row blocks, the weights
  // streamed once per block
  p.mt = M <= 64 ? 2 : 10;
  // A product over fewer than four stages decodes its codes to fp16 (exact) and multiplies them on the fp16 MFMA, in 64-row
  // workgroups: the scaled fp8 instruction drops products far below the largest of their K group (gemm_f8.hip), an error of up to
  // 2^-16 of sum |qa||qw| that an fp32 summation of so few terms does not make.  No product of a net is that short (2MNK >= 2e9).
  p.decode = K / kF8Stage < kF8ScaledStages;
  if (p.decode) p.mt = 2;
  p.tn = cdiv(N, kF8BN);
  p.tm = cdiv(M, 32 * p.mt);
  const int stages = K / kF8Stage;
  // K ranges: the reduced-precision single-product rule (fc_lowp_ranges: CU time, not launch time -- ranges of at least 2048 K
  // values and no more of them than fill half the chip), below the full cut that gives every CU a workgroup
  int full = cdiv(256, p.tn * p.tm);
  if (full > stages / kF8MinStages) full = stages / kF8MinStages;
  if (full < 1) full = 1;
  int splits = p.tm == 1 ? fc_lowp_ranges(t, full, K, p.tn) : full;
  if (splits < 1) splits = 1;
  p.kper = cdiv(stages, splits) * kF8Stage;
  p.splits = cdiv(K, p.kper);
  if (p.splits > 1) p.part_bytes = fc_up256((size_t)p.splits * M * N * 4);
  if (quantise_here) {
    p.q_bytes = fc_up256((size_t)M * K);
    p.exp_bytes = fc_up256((size_t)M * 4);
  }
  p.in_range = fc_wide_in_range(p.kper / kF8Stage, quantise_here ? M : mstride);
  return p;
}

}  // namespace mnc
