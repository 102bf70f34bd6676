// Launch plans of the InnerProduct entry points (gemm.hip: mnc_fc, mnc_fc_pair; gemm_x3.hip: fc_lowp, fc_lowp_pair) as pure
// functions of the call's shape and the context's tuning array: which kernel, tile height, K ranges, block order, scratch bytes.
// The number of K ranges fixes how partial sums are grouped and so the last bits of every head blob; the launchers only carry a
// plan out.  A pair plan is a question to the single plan wherever its rule is "what the single launcher would do".  No HIP
// include: tests/test_fc_plan.py compiles this header for the host and holds it to a table of plans.
#pragma once
#include <cstddef>

#include "tune.h"

namespace mnc {

// K-split count of a GEMM whose `tiles` output tiles do not fill the chip on their own, by a small cost model instead of
// "tiles x splits ~ #CUs": workgroups run in rounds of `slots` (the CUs x workgroups per CU), a split of `per` stages costs
// per * stage_us, and every split adds a pass over the M x N partial sums (mn_bytes each way at ~3 TB/s) to the reduction.
// Used when there are several row blocks (M > one block: the CFM / ResNet configurations), where rounding the split count up
// could leave a second, nearly empty round (96 tiles x 3 splits = 288 workgroups on 256 CUs: 72 instead of 100 TFLOP/s).
static inline int choose_splits(int tiles, int stages, int min_stages, int slots, double stage_us, double mn_bytes) {
  int best = 1;
  double best_cost = 1e300;
  const int smax = stages / min_stages > 1 ? stages / min_stages : 1;
  for (int s = 1; s <= smax && s <= 1024; ++s) {
    const int per = cdiv(stages, s);
    if (cdiv(stages, per) != s) continue;                    // this count is not reachable after rounding `per` up
    const double rounds = (double)cdiv((long)tiles * s, slots);
    const double cost = rounds * per * stage_us + (s > 1 ? 3.0 + 2.0 * s * mn_bytes / 3.0e6 : 0.0);
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  return best;
}

// K ranges of a reduced-precision InnerProduct over ONE row block (round 6, profiles/r06_fc_ranges.txt).  Rounds 2-5 cut K so that
// tiles x ranges filled all 256 CUs -- the shortest launch when the product has the chip to itself.  With several images in flight it
// does not: other images' kernels run on the CUs a launch leaves free, and what a product costs is its CU TIME.  Every range pays a
// prologue, an epilogue that writes 300 KB of partial sums, and its share of the reduction pass -- fc7 + fc7_mask in fp16: 17 us of
// MFMA loop inside 38 us + a 16 us reduction with 8 ranges of 8 stages.  So: ranges of at least 2048 K values (pairs: 12288, below), and
// no more ranges than fill HALF the chip (first: fc6 + fc6_mask 8 -> 4 ranges, fc7 + fc7_mask 8 -> 2; then 2 and 1).  Four images in flight: f16 870 -> 914 images/s, bf16
// 841 -> 902, mixed 553 -> 579, bf16x3 451 -> 472; one image at a time f16 566 -> 555, bf16x3 372 -> 322 (the price: a launch is
// longer).  One range for fc7 is the same throughput and 5-8 % more latency.  The fp32 InnerProducts keep the full cut (their loops
// are 10x longer than their fixed costs: 266 -> 260 images/s with half the ranges).
// FC_SPLIT_DIV (A/B): 0 = the full cut everywhere; otherwise the full cut divided by the low decimal digit (K > 8192) / the high
// digit (K <= 8192; 0 = the low digit), fp32 included.
inline int fc_split_div(const int* t, int splits, int K) {
  const int v = tune(t, T_FC_SPLIT_DIV, 1), lo = v % 10, hi = (v / 10) % 10 ? (v / 10) % 10 : lo, top = (v / 100) % 10 ? (v / 100) % 10 : lo;
  const int d = K <= 8192 ? hi : K > 50000 ? top : lo;      // (hundreds digit: K > 50000, fc6_maskest)
  return d > 1 && splits > 1 ? (splits / d > 1 ? splits / d : 1) : splits;
}
inline int fc_lowp_ranges(const int* t, int splits, int K, int tiles, bool pair = false) {
  if (tune_set(t, T_FC_SPLIT_DIV)) return fc_split_div(t, splits, K);
  if (plan_latency(t)) return splits;
  // pairs (fc6 + fc6_mask, fc7 + fc7_mask): ranges of >= 12288 K values -- 2 ranges for the fc6 pair, none for the fc7 pair (no
  // partial sums, no reduction launch): with the images in flight on 16 hardware queues (12 in flight) f16 1087 -> 1118 images/s,
  // mixed 652 -> 660, bf16x3 506 -> 513; with four in flight 1078 -> 1072 / 638 -> 645 / 499 -> 499; no cut at all (32768): 1119 /
  // 662 / 515 with twelve but 984 / 627 / 457 with four.  A single product (fc6_maskest: one column tile) keeps 2048.  FC_RANGE_K.
  const int per = pair ? tune(t, T_FC_RANGE_K, 12288) : 2048, part = 128;
  int r = K / per > 1 ? K / per : 1;
  const int half = (part + tiles - 1) / tiles;
  if (r > half) r = half;
  return r < splits ? r : splits;
}

// What a launcher is called with, as far as its plan depends on it.
struct FcCall {
  FcCall(int M_, int N_, int K_, int ldc_) : M(M_), N(N_), K(K_), ldc(ldc_) {}
  int M, N, K, ldc;
  int f16 = 0;                    // reduced precision: 0 = split bf16 (32-deep stages), 1 = fp16, 2 = plain bf16 (64-deep)
  bool osm[2] = {false, false};   // reduced precision: the result is wanted a second time in stage-major form (pair: per product) ...
  long osm_rows = 0, osm_row0 = 0;    // ... as rows [osm_row0, osm_row0 + M) of a panel of osm_rows rows
  bool pre[2] = {false, false};   // reduced precision: the activations arrive in stage-major form (pair: per product) ...
  int mstride = 0;                // ... with this many rows per stage
  bool defer_reduce = false;      // fp32: the context's defer_reduce
  bool aligned16 = true;          // mnc_fc_pair: outputs and biases of both products on 16-byte boundaries
};
enum FcKernel {
  kFcStaged,    // fc_mfma_kernel<mt, sk>: fp32, register-staged, 128 columns
  kFcDma16,     // fc_mfma_dma16_kernel<10, 0, buf>: fp32, eight waves, LDS-DMA, 128 columns
  kFcX3,        // fc_x3_kernel<mt, mt == 5 ? 1 : 2, 0, f16>: reduced precision, register-staged, 128 columns
  kFcWide       // fc_lowp_dma_kernel<mt, f16>: reduced precision, LDS-DMA, 256 columns
};
constexpr int kFcBN = 128, kFcWideBN = 256;
constexpr size_t kFcSlabBytes = 163840;     // one tile's accumulators of one K range in register layout (kFcDma16)

struct FcPlan {
  // head > 0: rows [0, head) and [head, M) are two launches, each with a plan of its own (the launcher calls itself; nothing else
  // of this plan is set).  two_singles (pair plans): the products run as two single calls, each with its single plan.
  int head = 0;
  bool two_singles = false;
  bool small = false;             // below the 2 GFLOP bar (the profile records carry it in their name)
  FcKernel kernel = kFcStaged;
  int mt = 0, sk = 0;             // row tiles of 32 rows per workgroup, K values per stage
  int tn = 0, tm = 0;             // column tiles (pair: of both products) and row blocks
  int tm_arg = 0;                 // tm as the kernel takes it: negative = row block fastest in the block order
  int splits = 1, kper = 0;       // K ranges and K values per range
  bool slab = false;              // the ranges' partial sums as slabs in register layout; else as [range][M][N] rows
  bool buf = false;               // kFcDma16: copies through buffer descriptors
  int drop = 0;                   // kFcDma16: the last 16-row sub-tile holds no live row
  size_t part_bytes = 0;          // partial sums in the scratch arena (0 with one range)
  size_t conv_bytes = 0;          // behind them: ONE activation panel converted to its 2-byte form here (0: none arrives as fp32)
};

// small problems (< 2 GFLOP) use 64-row workgroups so that rows, column tiles and K splits together fill the chip
inline bool fc_small(int M, int N, int K) { return 2.0 * M * (double)N * K < 2.0e9; }

// Several 320-row blocks with a ragged tail (the CFM / ResNet configurations: 500-2000 RoIs per call): every block
// multiplies all of its row tiles, so the full blocks and the tail are two launches, each with the tile height and split
// count that suit it (M = 760: 2 x 320 + one 160-row block instead of 3 x 320).  Same stream: the second launch re-uses
// the split-K scratch after the first one's reduction.  MNC_FC_NOTAIL=1 keeps one launch.  -> the head's rows, or 0.
inline int fc_head_rows(const int* t, int M, int N, int K) {
  return M > 320 && M % 320 != 0 && M % 320 <= 160 && !fc_small(M, N, K) && !tune(t, T_FC_NOTAIL, 0) ? M / 320 * 320 : 0;
}

// one row block whose last 16-row sub-tile holds no live row (300 RoIs = 18 sub-tiles + 12 rows): its MFMAs are skipped
inline int fc_dma16_drop(int M, int tm) { return tm == 1 && M > 288 && M <= 304 ? 1 : 0; }

// mnc_fc
inline FcPlan fc_plan(const FcCall& c, const int* t, bool tuning) {
  const int M = c.M, N = c.N, K = c.K;
  FcPlan p;
  p.head = fc_head_rows(t, M, N, K);
  if (p.head) return p;
  // the large ones use the smallest of {160, 320} rows that covers M in one block (weights streamed once).  Measured at M = 300
  // (round 1): 320 rows x 32-deep stages, one workgroup per CU, and 160 rows x 16-deep stages, two per CU, are within 1 %
  // of each other on every FC of the heads (MNC_FC_TILE=5|10 overrides).
  const bool small = fc_small(M, N, K);
  int mt = small ? 2 : (M <= 160 ? 5 : 10);            // row tiles per workgroup (all of them are always multiplied)
  // When the K splits of the 320-row variant would be shorter than 64 stages (fc7, fc6_maskest), 160-row blocks were a few per
  // cent faster than the REGISTER-STAGED 320-row kernel (round 1: 107 vs 112 us, 160 vs 169 us).  Against the LDS-DMA kernel
  // (K % 64 == 0) they lose: fc7 105.7 -> 100.7 us, fc6_maskest 159.6 -> 153.5 us on the 320-row DMA kernel (round 3,
  // kernel_bench fc), and the weights are streamed once instead of once per row block -- so the rule only applies without it.
  if (mt == 10 && (K % 64 != 0 || tune(t, T_FC_DMA, 1) == 0) && (K / 32) / cdiv(256, cdiv(N, kFcBN) * cdiv(M, 320)) < 64) mt = 5;
  if (tune_set(t, T_FC_TILE)) {
    const int v = tune(t, T_FC_TILE, 0);
    if (!small && (v == 5 || v == 10)) mt = v;
  }
  const int sk = mt == 5 ? 16 : 32;                    // K values per stage
  const int bm = 32 * mt;
  const int tn = cdiv(N, kFcBN), tm = cdiv(M, bm), stages = K / sk;
  // enough splits to give every CU its workgroups (two per CU except for the 320-row variant), but at least 64 K values
  // (8 stages for the large variants) per split
  int splits = cdiv(mt == 10 ? 256 : 512, tn * tm);
  // small variant: deep K (the N = 126 heads, K = 8192) gets at least 8 stages per split -- 32 splits instead of 103 cut
  // its reduction from 24 to 11 us and the total from 44 to 29 us; shallow K (mask_pred, K = 256) keeps 2
  const int min_stages = small ? (stages >= 64 ? 8 : 2) : (mt == 5 ? 16 : 8);
  if (splits > stages / min_stages) splits = stages / min_stages;
  // a small GEMM over at most 8 stages (mask_pred: K = 256) is not cut at all: four ranges of two stages each cost 9.5 us + a
  // 6.3 us reduction launch (kernel_bench fc, round 5) for 0.07 GFLOP; one range of eight stages writes the result itself
  if (small && stages <= 8) splits = 1;
  if (splits < 1) splits = 1;
  if (!small && tm == 1) splits = fc_split_div(t, splits, K);
  if (tm > 1 && !small)      // several row blocks: pick the split count by cost (see choose_splits); one block: as tuned above
    splits = choose_splits(tn * tm, stages, min_stages, mt == 10 ? 256 : 512,
                           (double)bm * kFcBN * sk * 2.0 / 460.0e3 * (mt == 10 ? 1.0 : 2.0), 4.0 * M * (double)N);
  int kper = cdiv(stages, splits) * sk;
  // LDS-DMA build of the 320-row kernel (fc_mfma_dma16_kernel; MNC_FC_DMA=0: the register-staged one).  Its loop walks one stage per
  // iteration, so a K range may hold an odd number of stages (rounds 3-5 rounded the ranges up to even counts, a leftover of the first
  // DMA build: fc6_maskest then ran 121 ranges of 26 stages on 242 CUs where 126 ranges of 25 fit 252 -- profiles/r06_fc_maskest.txt)
  const bool dma = mt == 10 && K % 64 == 0 && !tune_set(t, T_FC_ABL) && tune(t, T_FC_DMA, 1) != 0;
  if (dma && tune(t, T_FC_EVEN, 0)) kper = cdiv(kper, 64) * 64;
  splits = cdiv(K, kper);
  // (In-launch reduction of the K ranges by each tile's last arriver: built and measured in round 5 -- a loss here, the last arriver
  // reads 8 x 160 KB on one CU while 224 idle, profiles/r05_inlaunch_reduce.txt -- and removed in round 6.)
  // the eight-wave 16x16x4 kernel leaves its K ranges as SLABS (its accumulators in register layout, 160 KB per tile and range:
  // fc_reduce_slab_kernel); every other kernel as [range][M][N] rows (fc_reduce_kernel)
  p.slab = dma;
  if (tuning && dma && tune(t, T_FC_DMA_ABL, 0) < 16 &&
      (tune(t, T_FC_MFMA16, 1) == 0 || tune(t, T_FC_DMA_WAVES, 8) == 4 || tune(t, T_FC_DMA_ABL, 0)))
    p.slab = false;                                    // (the 32x32x2 builds of the tuning library)
  p.small = small;
  p.kernel = dma ? kFcDma16 : kFcStaged;
  p.mt = mt; p.sk = sk; p.tn = tn; p.tm = p.tm_arg = tm; p.splits = splits; p.kper = kper;
  p.drop = dma ? fc_dma16_drop(M, tm) : 0;
  // copies through buffer descriptors (32-bit lane offsets from the workgroup's first row: 320 rows of K floats must stay
  // below the descriptor's range) -- same bytes to the same places, bit-identical results, 2-4 % faster than 64-bit lane
  // addresses (kernel_bench fc, MNC_FC_DMA_ABL=20 against 16: fc6 511 -> 500 us, fc7 92.9 -> 89.2, fc6_maskest 142 -> 137)
  p.buf = dma && 320.0 * (double)K * 4.0 < 1.8e9;
  if (splits > 1) p.part_bytes = p.slab ? (size_t)tn * tm * splits * kFcSlabBytes : (size_t)splits * M * N * 4;
  return p;
}

// mnc_fc_pair: ONE launch of the eight-wave LDS-DMA kernel when mnc_fc would run each product as one launch of that kernel
// (so: fp32, >= 2 GFLOP, 160 < M, no ragged tail, K % 64 == 0); otherwise two singles.
inline FcPlan fc_pair_plan(const FcCall& c, const int* t, bool tuning) {
  const int M = c.M, N = c.N, K = c.K;
  const FcPlan s = fc_plan(c, t, tuning);
  // Where the pair's rule is its own: the paired launch has only the buffer-descriptor instantiation (s.buf) and vector epilogues
  // (N and ldc multiples of 4, 16-byte aligned outputs and biases); any FC_TILE value, also the 10 that mnc_fc obeys, and a deferred
  // reduction (one set of partial sums per product) keep the singles.
  bool fast = !s.head && s.kernel == kFcDma16 && s.buf && N % 4 == 0 && c.ldc % 4 == 0 && c.aligned16 && !tune_set(t, T_FC_TILE) &&
              !c.defer_reduce;
  // (tuning builds: every ablation or superseded-kernel key keeps the singles, also FC_DMA_ABL >= 16, which mnc_fc runs on slabs)
  if (tuning && (tune(t, T_FC_MFMA16, 1) == 0 || tune(t, T_FC_DMA_WAVES, 8) == 4 || tune(t, T_FC_DMA_ABL, 0))) fast = false;
  FcPlan p;
  if (!fast) {
    p.two_singles = true;
    return p;
  }
  // HALF as many ranges as mnc_fc would cut (twice the column tiles fill the chip), always of an even number of 32-deep stages
  // (mnc_fc: only with FC_EVEN)
  const int tn = cdiv(N, kFcBN), tm = cdiv(M, 320), stages = K / 32;
  int splits = cdiv(256, 2 * tn * tm);
  if (splits > stages / 8) splits = stages / 8;
  if (splits < 1) splits = 1;
  if (tm > 1) splits = choose_splits(2 * tn * tm, stages, 8, 256, 320.0 * kFcBN * 32 * 2.0 / 460.0e3, 8.0 * M * (double)N);
  else splits = fc_split_div(t, splits, K);
  const int kper = cdiv(cdiv(stages, splits) * 32, 64) * 64;
  splits = cdiv(K, kper);
  p.kernel = kFcDma16;
  p.mt = 10; p.sk = 32; p.tn = 2 * tn; p.tm = p.tm_arg = tm; p.splits = splits; p.kper = kper;
  p.slab = p.buf = true;
  p.drop = fc_dma16_drop(M, tm);
  if (splits > 1) p.part_bytes = (size_t)2 * tn * tm * splits * kFcSlabBytes;
  return p;
}

// ---- reduced precision (gemm_x3.hip) ----
inline int fc_lowp_stage(int f16) { return f16 ? 64 : 32; }
// the 256-column kernel's bar: K ranges of at least this many stages (fc7 at 300 RoIs would get 4: prologue and epilogue of a
// workgroup then outweigh the traffic saved)
inline int fc_wide_min_stages(int f16) { return f16 ? 8 : 16; }
// (the 256-column kernel addresses a stage of the activations by a 32-bit scalar offset: stages x m_stride x 128 bytes)
inline bool fc_wide_in_range(int stages, int rows) { return (double)stages * (double)rows * 128.0 < 4.0e9; }
inline int fc_lowp_min_stages(int f16, int mt) { return f16 ? (mt == 2 ? 1 : 4) : (mt == 2 ? 2 : 8); }
inline double fc_lowp_stage_us(int f16, int bm, int bn) { return (double)bm * bn * fc_lowp_stage(f16) * 2.0 / (f16 ? 2000.0e3 : 1050.0e3); }
inline size_t fc_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Several row blocks (M > 320: the 1000-RoI ResNet configuration, CFM): every block streams its whole weight panel, so a
// block costs about (rows + 128) -- measured: the 40-row tail of M = 1000 took 0.19 of the time of the 960 rows before it.
// 256-row blocks (fc_x3_kernel<8, 2>) in ONE launch when that is cheaper than 320-row blocks plus a tail launch:
// M = 1000: 4 x (256 + 128) = 1536 against 3 x 448 + 288 = 1632; M = 960 or 2000 stay on 320-row blocks.
inline bool fc_lowp_rows256(const int* t, int M, int N, int K) {
  if (M <= 320 || fc_small(M, N, K)) return false;
  const int tail = M % 320;
  const long cost320 = (long)(M / 320) * 448 + (tail == 0 ? 0 : tail <= 160 ? 288 : 448);
  const long cost256 = (long)cdiv(M, 256) * 384;
  return cost256 < cost320 && !tune(t, T_FC_NO256, 0);
}

// full 320-row blocks and a ragged tail of at most 160 rows are two launches, each with its own tile height (fc_head_rows), unless
// 256-row blocks take all rows in one
inline int fc_lowp_head_rows(const int* t, int M, int N, int K) { return fc_lowp_rows256(t, M, N, K) ? 0 : fc_head_rows(t, M, N, K); }

// fc_lowp
inline FcPlan fc_lowp_plan(const FcCall& c, const int* t) {
  const int M = c.M, N = c.N, K = c.K, f16 = c.f16, kStage = fc_lowp_stage(f16);
  FcPlan p;
  p.head = fc_lowp_head_rows(t, M, N, K);
  if (p.head) return p;
  const bool rows256 = fc_lowp_rows256(t, M, N, K);
  // row tiles per workgroup: 2 (64 rows) for the small GEMMs, else the smallest of {5, 10} that covers M in one block
  const bool small = fc_small(M, N, K);
  int mt = small ? 2 : (M <= 160 ? 5 : 10);
  // 320-row blocks stream the weights once but need many K splits to fill the chip; when a split would be shorter than 64 stages
  // (bf16x3; 32 for fp16), 160-row blocks (twice the tiles, half the splits and half the partial-sum traffic) are faster
  // (measured at M = 300, bf16x3: fc7 59 vs 69 us, fc6_maskest 132 vs 151 us, fc6 274 vs 262 us)
  // Round 6, throughput plan: ONE row block runs on the 256-column LDS-DMA kernel from N = 256 on, in fc_lowp_ranges' K ranges, split
  // bf16 included -- fc6_maskest (N = 256, K = 100352): one column tile x 49 ranges of 2048 K values on 49 CUs, each operand read
  // once (111 MB), instead of 2 x 2 tiles x 64 ranges on the 160-row register-staged kernel.  The launch is longer (fp16 37 -> 67 us,
  // split bf16 65 -> 159) and costs a fifth of the CU time: f16 985 -> 991 images/s, mixed 616 -> 620, bf16x3 488 -> 491 (two runs
  // each, profiles/r06_fc_ranges.txt); the latency plan keeps the old choice.
  const bool wide1 = tune(t, T_FCX3_WIDE, 1) != 0 && !tune_set(t, T_FCX3_TILE) && !plan_latency(t) && mt == 10 && M <= 320 && N % 256 == 0 && N >= 256 &&
                     (K / kStage) / fc_lowp_ranges(t, 256, K, N / 256) >= fc_wide_min_stages(f16);
  if (!wide1 && mt == 10 && (K / kStage) / cdiv(256, cdiv(N, kFcBN) * cdiv(M, 320)) < (f16 ? 32 : 64)) mt = 5;
  if (rows256) mt = 8;
  if (tune_set(t, T_FCX3_TILE)) {
    const int v = tune(t, T_FCX3_TILE, 0);
    if (v == 2 || v == 5 || v == 8 || v == 10) mt = v;
  }
  const int bm = 32 * mt;
  const int stages = K / kStage, tm = cdiv(M, bm);
  // 256- or 320-row blocks, N a multiple of 256: the 256-column LDS-DMA kernel (fc_lowp_dma_kernel) -- half the activation
  // bytes per flop (the reduced-precision pipe is power limited, DESIGN.md section 9 item 4: bytes are energy) -- when its K splits
  // keep fc_wide_min_stages.  FCX3_WIDE=0: off.
  bool wide = false;
  // (throughput plan, round 6: from N = 256 on -- one column tile per row block; ResNet-50 configuration, fc6_maskest at 1000 RoIs:
  // f16 260.5 -> 264.6 images/s, mixed 130.2 -> 134.2)
  if ((mt == 8 || mt == 10) && N % 256 == 0 && N >= (plan_latency(t) ? 512 : 256) && tune(t, T_FCX3_WIDE, 1) != 0) {
    const int sp = cdiv(256, (N / 256) * tm);
    wide = stages / (sp > 0 ? sp : 1) >= fc_wide_min_stages(f16);
    // split bf16 at one row block (300 RoIs): three MFMAs per term make the operand bytes a smaller share of the work, and the doubled
    // K splits cost in the reduction what the kernel gains (fc6: 213.9 + 10.8 us vs 204.5 + 16.9 us) -- the 128-column kernel stays
    if (!f16 && tm == 1 && !tune_set(t, T_FCX3_WIDE)) wide = false;
  }
  if (wide1) wide = true;
  if (wide && !fc_wide_in_range(stages, c.pre[0] ? c.mstride : M)) wide = false;
  const int bn_w = wide ? kFcWideBN : kFcBN;
  const int tn = cdiv(N, bn_w);
  int splits = cdiv(mt == 2 ? 512 : 256, tn * tm);
  const int min_stages = fc_lowp_min_stages(f16, mt);
  if (splits > stages / min_stages) splits = stages / min_stages;
  if (splits < 1) splits = 1;
  if (tm == 1 && mt != 2) {
    const int full = splits;
    splits = fc_lowp_ranges(t, splits, K, tn);      // (round 6: CU time, not launch time)
    // (a second output in stage-major form is written by the reduction pass; without one only dense rows can be converted)
    if (splits == 1 && full > 1 && c.osm[0] && (c.ldc != N || c.osm_rows != M || c.osm_row0 != 0)) splits = 2;
  }
  if (tm > 1 && mt != 2)     // several row blocks: split count by cost (choose_splits)
    // (round 6, throughput plan: the K ranges fill HALF the chip here too -- ResNet-50 configuration, 1000 RoIs, four images in
    // flight: f16 249 -> 262 images/s, mixed 126.5 -> 131.6 with 128 slots, 259 with 64; FC_SLOTS overrides)
    splits = choose_splits(tn * tm, stages, min_stages, tune(t, T_FC_SLOTS, plan_latency(t) ? 256 : 128),
                           fc_lowp_stage_us(f16, bm, bn_w), 4.0 * M * (double)N);
  const int kper = cdiv(stages, splits) * kStage;
  splits = cdiv(K, kper);
  // Block order with several row blocks: row block fastest, so the workgroups that multiply the same weight panel are
  // neighbours on one XCD and stream it from L2 together instead of once per row block from HBM (measured, fp16, M = 960:
  // N = 4096, K = 50176: 612 -> 555 us; M = 2000, K = 25088: 302 -> 282 us; with two column tiles (N = 256) it is 3 % slower,
  // so only from 8 column tiles on).  MNC_FC_ORDER=0 / 1 forces the column-tile-fastest / row-block-fastest order.
  const bool rows_fastest = tune_set(t, T_FC_ORDER) ? tune(t, T_FC_ORDER, 0) == 1 : tn >= 8;
  p.small = small;
  p.kernel = wide ? kFcWide : kFcX3;
  p.mt = mt; p.sk = kStage; p.tn = tn; p.tm = tm; p.tm_arg = (rows_fastest && tm > 1) ? -tm : tm; p.splits = splits; p.kper = kper;
  if (splits > 1) p.part_bytes = fc_up256((size_t)splits * M * N * 4);
  if (!c.pre[0]) p.conv_bytes = (size_t)M * K * (f16 ? 2 : 4);
  return p;
}

// fc_lowp_pair: ONE launch of the 256-column kernel over one row block of 161..320 rows or, in the throughput plan, over the row
// blocks fc_lowp would run in one launch; otherwise two singles.
inline FcPlan fc_lowp_pair_plan(const FcCall& c, const int* t) {
  const int M = c.M, N = c.N, K = c.K, f16 = c.f16, kStage = fc_lowp_stage(f16);
  const int stages = K / kStage, tn = N / kFcWideBN;
  const bool osm = c.osm[0] || c.osm[1];
  // Several row blocks (round 6, throughput plan only; the ResNet-50 configuration's 1000 RoIs): the pair runs as ONE launch too when
  // fc_lowp would run each product as one launch -- 256-row blocks, or 320-row blocks without a ragged tail of <= 160 rows.  The pair
  // asks fc_lowp for no more than that: it runs the 256-column kernel on whole 256- or 320-row blocks also where fc_lowp alone would
  // take 160-row blocks of the 128-column kernel (fc7 at 640 rows), because twice the column tiles keep its K ranges long enough.
  int mt = 10, tm = 1;
  bool one_launch = M <= 320;
  if (M > 320 && !plan_latency(t)) {
    one_launch = !fc_lowp_head_rows(t, M, N, K);        // (the first question of fc_lowp_plan)
    mt = fc_lowp_rows256(t, M, N, K) ? 8 : 10;
    tm = cdiv(M, 32 * mt);
  }
  // The pair's own bars: N >= 512 (fc_lowp: 256 -- a pair of one-column-tile products is not worth a launch form of its own), any
  // FCX3_TILE value keeps the singles, FUSE_SMALL=0 switches pairing off, and the scalar-offset range counts the shared row stride.
  bool paired = M > 160 && one_launch && N % 256 == 0 && N >= 512 && !fc_small(M, N, K) && tune(t, T_FCX3_WIDE, 1) != 0 &&
                fc_wide_in_range(stages, (c.pre[0] || c.pre[1]) ? c.mstride : M) && !tune_set(t, T_FCX3_TILE) &&
                tune(t, T_FUSE_SMALL, 1) != 0;
  // (one launch reads both panels with ONE row stride: a panel converted here has M rows per stage, so a single pre-packed panel
  // of another stride keeps the singles -- decided here, before the launcher enqueues a conversion)
  if (c.pre[0] != c.pre[1] && c.mstride != M) paired = false;
  const int min_stages = fc_lowp_min_stages(f16, mt);
  int splits = 1;
  if (paired && tm > 1) {
    splits = choose_splits(2 * tn * tm, stages, min_stages, tune(t, T_FC_SLOTS, 128), fc_lowp_stage_us(f16, 32 * mt, kFcWideBN),
                           8.0 * M * (double)N);
    paired = stages / splits >= fc_wide_min_stages(f16);
    if (splits == 1 && stages >= 2 * fc_wide_min_stages(f16) && osm && c.ldc != N) splits = 2;
  } else if (paired) {
    splits = cdiv(256, 2 * tn);
    if (splits > stages / min_stages) splits = stages / min_stages;
    if (splits < 1) splits = 1;
    paired = stages / splits >= fc_wide_min_stages(f16);
    const int full = splits;
    splits = fc_lowp_ranges(t, splits, K, 2 * tn, true);     // (round 6: CU time, not launch time)
    // (a second output in stage-major form is written by the reduction pass; without one only dense rows can be converted)
    if (splits == 1 && full > 1 && osm && c.ldc != N) splits = 2;
  }
  FcPlan p;
  if (!paired) {
    p.two_singles = true;
    return p;
  }
  const int kper = cdiv(stages, splits) * kStage;
  splits = cdiv(K, kper);
  p.kernel = kFcWide;
  // (several row blocks: row block fastest, so that the workgroups sharing a weight panel are neighbours on one XCD -- fc_lowp_plan)
  p.mt = mt; p.sk = kStage; p.tn = 2 * tn; p.tm = tm; p.tm_arg = tm > 1 ? -tm : 1; p.splits = splits; p.kper = kper;
  if (splits > 1) p.part_bytes = fc_up256((size_t)2 * splits * M * N * 4);
  if (!c.pre[0] || !c.pre[1]) p.conv_bytes = fc_up256((size_t)M * K * (f16 ? 2 : 4));
  return p;
}

}  // namespace mnc
