// The launchers' tuning keys, read from a context's `tune` array.  No HIP include: the launch plans built on it (fc_plan.h) are
// compiled for the host by the tests.  mnc_internal.h forwards the mnc_ctx* forms.
#pragma once
#include <climits>

namespace mnc {
// Per-context overrides of the launchers' own choices (tile shapes, kernel variants, plan switches): mnc_ctx_set_tuning(ctx, "FC_TILE", 5)
// or, once, at context creation, the environment variable MNC_<NAME>.  They exist so that every variant a launcher can pick by
// shape is reachable from a test at a small shape, and for A/B measurements; no launch path calls getenv.  Ablation and
// superseded kernel builds (FC_ABL, FC_DMA_ABL, FCX3_ABL, CONV_ABL, WINO_V = 1, WINO_VAR != 7) are only compiled with -DMNC_TUNING.
#define MNC_TUNE_KEYS(X)                                                                                                          \
  X(CONV_COT) X(CONV_ROWS) X(CONV_KSPLIT) X(CONV_ABL) X(CONV1X1_TILE) X(CONV2D_WIDE) X(WINO_ROWS) X(WINO_TAIL) X(WINO_V) X(WINO_VAR)  \
  X(WINO_DMA) X(WINO_XCD) X(CONVX3_TILE) X(FC_NOTAIL) X(FC_TILE) X(FC_ABL) X(FC_DMA) X(PLAN) X(FC_RANGE_K) X(FC_SLOTS) X(FC_EVEN) X(FC_SPLIT_DIV) X(WINO_FILL) X(CONVX3_P0MIN) X(CONVX3_P1MIN) X(FC_DMA_ABL) X(FC_DMA_WAVES)    \
  X(FC_NO256) X(FCX3_TILE) X(FC_ORDER) X(FCX3_ABL) X(FC_SM) X(PACKED_ACT) X(FUSE_POOLS) X(BRANCH_STREAMS) X(TOPK_SINGLE_WG)           \
  X(ROI_SM_VARIANT) X(ROI_WARP_VARIANT) X(FC_REDUCE) X(WINO_F4) X(FUSE_SMALL) X(FCX3_WIDE) X(FC_HALF) X(WINO_STREAM) X(FC_MFMA16) X(WINO_MFMA16) X(ROI_ROW_SEGS) X(WINO_SPLIT)
enum TuneKey {
#define MNC_TUNE_ENUM(n) T_##n,
  MNC_TUNE_KEYS(MNC_TUNE_ENUM)
#undef MNC_TUNE_ENUM
  T_COUNT
};
constexpr int kTuneUnset = INT_MIN;

inline bool tune_set(const int* t, TuneKey k) { return t[k] != kTuneUnset; }
inline int tune(const int* t, TuneKey k, int dflt) { return t[k] != kTuneUnset ? t[k] : dflt; }
// PLAN (round 6, profiles/r06_fc_ranges.txt): what the launchers' plans minimise.  0 (default) = the CU TIME of a launch -- the
// deployment the headline measures, several images in flight per GPU: the CUs a launch leaves free run the other images' kernels.
// 1 = the DURATION of a launch (rounds 1-5: every product cut until it fills the chip) -- one image at a time, latency.  One value
// per context (MNC_PLAN=1 or mnc_ctx_set_tuning(ctx, "PLAN", "1")); the nets that share results bit for bit must share it.
inline bool plan_latency(const int* t) { return tune(t, T_PLAN, 0) == 1; }

// WINO_SPLIT: the fp32 F(4x4, 3x3) layers as three launches -- input transform, one batched InnerProduct launch over the 36 transform
// positions, output transform (conv_wino4_split.hip) -- instead of the fused kernel.  0 = never, 1 = the layers the throughput plan
// selects (none under PLAN = 1), 2 = every layer the split form supports (tests, A/B).  Read when a net packs its weights and at
// every trunk layer; the nets that share results bit for bit must share it.
constexpr int kWinoSplitDefault = 1;
// the layers WINO_SPLIT = 1 moves, by channel counts (the map's size is checked at the call: at least one full row block of tiles)
inline bool wino4_split_plan_channels(int Cin, int Cout) { return Cin >= 512 && Cout >= 512; }

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
}  // namespace mnc
