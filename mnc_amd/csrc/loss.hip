// The loss layers of the training graph for gfx950: SoftmaxWithLoss, SmoothL1Loss, SigmoidCrossEntropyLoss -- the value and the
// gradient with respect to the prediction -- and the backward passes of ReLU and Sigmoid; include/mnc_hip.h n25, the statements
// are mnc_amd/losses.py.
//
// The file is compiled with -ffp-contract=off and every exp of a float32 is np_exp_f32 (np_exp.h), so a probability and every
// gradient element is formed by the statement's operations in the statement's order: the same bits.  The only function that is
// not numpy's is logf, in the terms of the softmax and the sigmoid loss (a few ulps, not bit for bit).
//
// Reductions: no floating-point atomics.  A launch has a fixed geometry (a function of the shape alone); every workgroup leaves
// one partial {sum of its terms, valid count, status} in the context's scratch, formed in a fixed order (per lane ascending, one
// shuffle tree, the four waves in order); loss_finalize_kernel, one workgroup, loads them into LDS and one lane adds them in index
// order and writes the 16-byte result.  The counts are integers: ballots and integer adds.  The softmax gradient is a third
// launch that reads the normaliser from that result: the count exists on the device before the gradient is scaled, and the host
// never sees it.
#include <cfloat>

#include "mnc_internal.h"
#include "np_exp.h"

namespace mnc {

constexpr int kLossMaxGroups = 256;       // workgroups of a loss launch, and so partials in the scratch, at most

struct LossPartial {
  float sum;
  int count, status, pad;
};
struct LossResult {                       // d_result of the entries: 16 bytes
  float loss, normalizer;
  int count, status;
};

std::atomic<int> g_softmax_plan{0};       // mnc_softmax_loss_plan

// The workgroup's partial from its waves' values (sum: per lane; count, status: wave-uniform).
__device__ __forceinline__ void loss_write_partial(float sum, int count, int status, LossPartial* __restrict__ part) {
  __shared__ float s_sum[4];
  __shared__ int s_cnt[4], s_st[4];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_sum[wave] = sum; s_cnt[wave] = count; s_st[wave] = status; }
  __syncthreads();
  if (threadIdx.x == 0) {
    LossPartial p;
    p.sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    p.count = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    p.status = s_st[0] | s_st[1] | s_st[2] | s_st[3];
    p.pad = 0;
    part[blockIdx.x] = p;
  }
}

// One workgroup: it brings the partials into LDS together, then one lane adds them in index order (the order is the contract; the
// loads need not wait for each other).  norm_fixed > 0: the normaliser; 0: max(valid count, 1).
__global__ __launch_bounds__(256) void loss_finalize_kernel(const LossPartial* __restrict__ part, int groups, int norm_fixed,
                                                            LossResult* __restrict__ result) {
  __shared__ float s_sum[kLossMaxGroups];
  __shared__ int s_cnt[kLossMaxGroups], s_st[kLossMaxGroups];
  for (int g = threadIdx.x; g < groups; g += blockDim.x) {           // (groups <= kLossMaxGroups: loss_groups)
    const LossPartial p = part[g];
    s_sum[g] = p.sum; s_cnt[g] = p.count; s_st[g] = p.status;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float s = 0.0f;
  int cnt = 0, st = 0;
  for (int g = 0; g < groups; ++g) {
    s = s + s_sum[g];
    cnt += s_cnt[g];
    st |= s_st[g];
  }
  LossResult r;
  r.normalizer = norm_fixed > 0 ? (float)norm_fixed : (float)(cnt > 1 ? cnt : 1);
  r.loss = __fdiv_rn(s, r.normalizer);
  r.count = cnt;
  r.status = st;
  *result = r;
}

// ---- SoftmaxWithLoss ---------------------------------------------------------------------------------------------------------
// A label: 1 valid (*li its class), 0 ignored, -1 invalid (never used as an index).  (int) of a float outside int's range is
// undefined, so such a label, and a NaN, is invalid before the cast.
__device__ __forceinline__ int loss_label(float l, int C, int has_ignore, int ignore_label, int* li) {
  if (!(l >= -2147483648.0f && l < 2147483648.0f)) return -1;
  const int v = (int)l;
  if (has_ignore && v == ignore_label) return 0;
  if ((float)v != l || v < 0 || v >= C) return -1;
  *li = v;
  return 1;
}

__device__ __forceinline__ float softmax_term(float p_label) { return -logf(fmaxf(p_label, FLT_MIN)); }

// Layout "positions" (inner > 1, the RPN): one lane per position (o, i), class stride `inner`; the loads of a wave are contiguous
// over i.  Three loops over c: the maximum, the ascending sum from +0.0, the outputs.  kGrad: the gradient launch.
template <bool kGrad>
__global__ __launch_bounds__(256) void softmax_loss_pos_kernel(const float* __restrict__ score, const float* __restrict__ label, int C,
                                                               long inner, long npos, int has_ignore, int ignore_label,
                                                               float loss_weight, const LossResult* __restrict__ result,
                                                               float* __restrict__ prob, float* __restrict__ terms,
                                                               float* __restrict__ dscore, LossPartial* __restrict__ part) {
  float acc = 0.0f, scale = 0.0f;
  int cnt = 0, st = 0;
  if (kGrad) scale = __fdiv_rn(loss_weight, result->normalizer);
  for (long base = (long)blockIdx.x * 256; base < npos; base += (long)gridDim.x * 256) {     // (workgroup-uniform trip count: ballots)
    const long pos = base + threadIdx.x;
    int kind = 0, li = 0;
    float term = 0.0f;
    if (pos < npos) {
      const long o = pos / inner, i = pos - o * inner;
      const long x0 = o * C * inner + i;
      const float* x = score + x0;
      kind = loss_label(label[pos], C, has_ignore, ignore_label, &li);
      if (kind == 1 || (!kGrad && prob)) {
        float m = x[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, x[c * inner]);
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s = s + np_exp_f32(x[c * inner] - m);
        if (kGrad) {
          for (int c = 0; c < C; ++c) {
            const float p = __fdiv_rn(np_exp_f32(x[c * inner] - m), s);
            dscore[x0 + c * inner] = (p - (c == li ? 1.0f : 0.0f)) * scale;
          }
        } else {
          if (prob)
            for (int c = 0; c < C; ++c) prob[x0 + c * inner] = __fdiv_rn(np_exp_f32(x[c * inner] - m), s);
          if (kind == 1) term = softmax_term(__fdiv_rn(np_exp_f32(x[li * inner] - m), s));
        }
      } else if (kGrad) {
        for (int c = 0; c < C; ++c) dscore[x0 + c * inner] = 0.0f;
      }
      if (!kGrad && terms) terms[pos] = term;
    }
    if (!kGrad) {
      acc = acc + term;
      cnt += __popcll(__ballot(kind == 1));
      st |= __ballot(kind < 0) != 0ull ? 1 : 0;
    }
  }
  if (!kGrad) loss_write_partial(acc, cnt, st, part);
}

// Layout "rows" (inner == 1, the heads): one wave per position, lane l holds the classes l, l + 64, ...  The maximum by shuffles.
// The sum has to be the ascending one: chunk by chunk of 64 classes, the lanes' exponentials are read lane 0, 1, 2, ... (readlane)
// and added to one running sum that every lane carries -- the sequential carry across the lanes, C dependent adds per row, which
// is what the rule costs.  The exponentials are formed again for the outputs (two exps per class are cheaper than a row in LDS
// at C = 21).  Written for any class stride, so that mnc_softmax_loss_plan can force it on the RPN shape.
template <bool kGrad>
__global__ __launch_bounds__(256) void softmax_loss_row_kernel(const float* __restrict__ score, const float* __restrict__ label, int C,
                                                               long inner, long npos, int has_ignore, int ignore_label,
                                                               float loss_weight, const LossResult* __restrict__ result,
                                                               float* __restrict__ prob, float* __restrict__ terms,
                                                               float* __restrict__ dscore, LossPartial* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const long nwaves = (long)gridDim.x * 4;
  float acc = 0.0f, scale = 0.0f;
  int cnt = 0, st = 0;
  if (kGrad) scale = __fdiv_rn(loss_weight, result->normalizer);
  for (long pos = (long)blockIdx.x * 4 + (threadIdx.x >> 6); pos < npos; pos += nwaves) {     // (wave-uniform)
    const long o = pos / inner, i = pos - o * inner;
    const long x0 = o * C * inner + i;
    const float* x = score + x0;
    int li = 0;
    const int kind = loss_label(label[pos], C, has_ignore, ignore_label, &li);
    float term = 0.0f;
    if (kind == 1 || (!kGrad && prob)) {
      float m = -__builtin_inff();
      for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c * inner]);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
      float s = 0.0f;
      for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const float e = c < C ? np_exp_f32(x[c * inner] - m) : 0.0f;
        const int n = C - c0 < 64 ? C - c0 : 64;
        for (int k = 0; k < n; ++k) s = s + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, e), k));
      }
      if (kGrad) {
        for (int c = lane; c < C; c += 64) {
          const float p = __fdiv_rn(np_exp_f32(x[c * inner] - m), s);
          dscore[x0 + c * inner] = (p - (c == li ? 1.0f : 0.0f)) * scale;
        }
      } else {
        if (prob)
          for (int c = lane; c < C; c += 64) prob[x0 + c * inner] = __fdiv_rn(np_exp_f32(x[c * inner] - m), s);
        if (kind == 1) term = softmax_term(__fdiv_rn(np_exp_f32(x[li * inner] - m), s));
      }
    } else if (kGrad) {
      for (int c = lane; c < C; c += 64) dscore[x0 + c * inner] = 0.0f;
    }
    if (!kGrad) {
      if (terms && lane == 0) terms[pos] = term;
      if (lane == 0) acc = acc + term;                 // (the wave's sum lives in lane 0; the other lanes add +0.0 in the tree)
      cnt += kind == 1;
      st |= kind < 0;
    }
  }
  if (!kGrad) loss_write_partial(acc, cnt, st, part);
}

// ---- SmoothL1Loss: value and gradient in one launch (the normaliser is N, known to the host) -------------------------------
__global__ __launch_bounds__(256) void smooth_l1_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const float* __restrict__ w_in, const float* __restrict__ w_out, long n,
                                                             float s2, float thr, float half_s2, float lin, float scale,
                                                             float* __restrict__ terms, float* __restrict__ dpred,
                                                             LossPartial* __restrict__ part) {
  float acc = 0.0f;
  int cnt = 0;
  for (long base = (long)blockIdx.x * 256; base < n; base += (long)gridDim.x * 256) {
    const long i = base + threadIdx.x;
    float term = 0.0f;
    if (i < n) {
      const float wi = w_in[i], wo = w_out[i];
      const float d = (pred[i] - target[i]) * wi;
      const float a = fabsf(d);
      const bool quad = a < thr;
      term = (quad ? half_s2 * d * d : a - lin) * wo;
      if (terms) terms[i] = term;
      if (dpred) {
        const float g = quad ? s2 * d : (0.0f < d ? 1.0f : 0.0f) - (d < 0.0f ? 1.0f : 0.0f);
        dpred[i] = g * wi * wo * scale;
      }
    }
    acc = acc + term;
    cnt += __popcll(__ballot(i < n));
  }
  loss_write_partial(acc, cnt, 0, part);
}

// ---- SigmoidCrossEntropyLoss with caffe-mnc's weight bottom ------------------------------------------------------------------
__global__ __launch_bounds__(256) void sigmoid_ce_loss_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                              const float* __restrict__ w, long n, float scale,
                                                              float* __restrict__ terms, float* __restrict__ dx,
                                                              LossPartial* __restrict__ part) {
  float acc = 0.0f;
  int cnt = 0;
  for (long base = (long)blockIdx.x * 256; base < n; base += (long)gridDim.x * 256) {
    const long i = base + threadIdx.x;
    float term = 0.0f;
    if (i < n) {
      const float xv = x[i], tv = t[i], wv = w ? w[i] : 1.0f;
      const float pos = xv >= 0.0f ? 1.0f : 0.0f;
      const float lg = logf(1.0f + np_exp_f32(xv - 2.0f * xv * pos));
      term = -(xv * (tv - pos) - lg) * wv;
      if (terms) terms[i] = term;
      if (dx) dx[i] = (__fdiv_rn(1.0f, 1.0f + np_exp_f32(-xv)) - tv) * wv * scale;
    }
    acc = acc + term;
    cnt += __popcll(__ballot(i < n));
  }
  loss_write_partial(acc, cnt, 0, part);
}

// ---- ReLU and Sigmoid backward, from the layer's output ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void eltwise_backward_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                               float* __restrict__ dx, size_t n, int op) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float yv = y[i], g = dy[i];
    dx[i] = op == 1 ? (yv > 0.0f ? g : 0.0f) : (g * yv) * (1.0f - yv);
  }
}

static int loss_groups(long items) {
  long g = (items + 255) / 256;
  if (g > kLossMaxGroups) g = kLossMaxGroups;
  return (int)(g < 1 ? 1 : g);
}

static int loss_zero_result(mnc_ctx* ctx, void* d_result) {
  (void)hipSetDevice(ctx->device);
  MNC_HIP_TRY(hipMemsetAsync(d_result, 0, sizeof(LossResult), ctx->stream));
  clear_error();
  return MNC_OK;
}

static int loss_finalize(mnc_ctx* ctx, const LossPartial* part, int groups, int norm_fixed, void* d_result) {
  LaunchScope ls(ctx, "loss_finalize");
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, part, groups, norm_fixed, (LossResult*)d_result);
  return ls.finish("loss_finalize_kernel");
}

}  // namespace mnc

using namespace mnc;

extern "C" {

int mnc_softmax_loss(mnc_ctx* ctx, const float* d_score, const float* d_label, int outer, int C, int inner, int has_ignore,
                     int ignore_label, int normalize, float loss_weight, float* d_prob, float* d_terms, float* d_dscore,
                     void* d_result) {
  MNC_REQUIRE(ctx && d_result, "mnc_softmax_loss: null ctx or d_result");
  MNC_REQUIRE(C >= 1 && C <= 4096, "mnc_softmax_loss: C=%d is not in [1, 4096]", C);
  MNC_REQUIRE(outer >= 0 && inner >= 0 && (long)outer * inner < (1L << 31), "mnc_softmax_loss: outer=%d, inner=%d: negative, or 2^31 positions or more", outer, inner);
  const long npos = (long)outer * inner;
  if (npos == 0) return loss_zero_result(ctx, d_result);
  MNC_REQUIRE(d_score && d_label, "mnc_softmax_loss: null d_score or d_label");
  const int plan = g_softmax_plan.load();
  const bool rows = plan == 0 ? inner == 1 : plan == 2;
  const int groups = rows ? loss_groups(npos * 64) : loss_groups(npos);
  int rc = ensure_scratch(ctx, kLossMaxGroups * sizeof(LossPartial));
  if (rc) return rc;
  LossPartial* part = (LossPartial*)ctx->scratch.p;
  const LossResult* res = (const LossResult*)d_result;
  {
    LaunchScope ls(ctx, "softmax_loss_fwd", 0.0, 4.0 * npos * (double)C * (d_prob ? 2.0 : 1.0));
    if (rows)
      hipLaunchKernelGGL(softmax_loss_row_kernel<false>, dim3(groups), dim3(256), 0, ctx->stream, d_score, d_label, C, (long)inner, npos,
                         has_ignore, ignore_label, loss_weight, res, d_prob, d_terms, (float*)nullptr, part);
    else
      hipLaunchKernelGGL(softmax_loss_pos_kernel<false>, dim3(groups), dim3(256), 0, ctx->stream, d_score, d_label, C, (long)inner, npos,
                         has_ignore, ignore_label, loss_weight, res, d_prob, d_terms, (float*)nullptr, part);
    rc = ls.finish("softmax_loss_kernel<false>");
    if (rc) return rc;
  }
  rc = loss_finalize(ctx, part, groups, normalize ? 0 : outer, d_result);
  if (rc) return rc;
  if (d_dscore) {
    LaunchScope ls(ctx, "softmax_loss_grad", 0.0, 8.0 * npos * (double)C);
    if (rows)
      hipLaunchKernelGGL(softmax_loss_row_kernel<true>, dim3(groups), dim3(256), 0, ctx->stream, d_score, d_label, C, (long)inner, npos,
                         has_ignore, ignore_label, loss_weight, res, (float*)nullptr, (float*)nullptr, d_dscore, part);
    else
      hipLaunchKernelGGL(softmax_loss_pos_kernel<true>, dim3(groups), dim3(256), 0, ctx->stream, d_score, d_label, C, (long)inner, npos,
                         has_ignore, ignore_label, loss_weight, res, (float*)nullptr, (float*)nullptr, d_dscore, part);
    rc = ls.finish("softmax_loss_kernel<true>");
    if (rc) return rc;
  }
  clear_error();
  return MNC_OK;
}

int mnc_softmax_loss_plan(int plan) {
  MNC_REQUIRE(plan >= 0 && plan <= 2, "mnc_softmax_loss_plan: plan=%d is not 0, 1 or 2", plan);
  g_softmax_plan.store(plan);
  clear_error();
  return MNC_OK;
}

int mnc_smooth_l1_loss(mnc_ctx* ctx, const float* d_pred, const float* d_target, const float* d_w_in, const float* d_w_out, int N,
                       long long count, float sigma, float loss_weight, float* d_terms, float* d_dpred, void* d_result) {
  MNC_REQUIRE(ctx && d_result, "mnc_smooth_l1_loss: null ctx or d_result");
  MNC_REQUIRE(N >= 0 && count >= 0 && count < (1LL << 31), "mnc_smooth_l1_loss: N=%d, count=%lld: negative, or 2^31 elements or more", N, count);
  if (N == 0 || count == 0) return loss_zero_result(ctx, d_result);
  MNC_REQUIRE(d_pred && d_target && d_w_in && d_w_out, "mnc_smooth_l1_loss: null input");
  const float s2 = sigma * sigma;
  const int groups = loss_groups((long)count);
  int rc = ensure_scratch(ctx, kLossMaxGroups * sizeof(LossPartial));
  if (rc) return rc;
  LossPartial* part = (LossPartial*)ctx->scratch.p;
  {
    LaunchScope ls(ctx, "smooth_l1_loss", 0.0, 4.0 * (double)count * (4.0 + (d_terms ? 1.0 : 0.0) + (d_dpred ? 1.0 : 0.0)));
    hipLaunchKernelGGL(smooth_l1_loss_kernel, dim3(groups), dim3(256), 0, ctx->stream, d_pred, d_target, d_w_in, d_w_out, (long)count, s2,
                       1.0f / s2, 0.5f * s2, 0.5f / s2, loss_weight / (float)N, d_terms, d_dpred, part);
    rc = ls.finish("smooth_l1_loss_kernel");
    if (rc) return rc;
  }
  rc = loss_finalize(ctx, part, groups, N, d_result);
  if (rc) return rc;
  clear_error();
  return MNC_OK;
}

int mnc_sigmoid_ce_loss(mnc_ctx* ctx, const float* d_x, const float* d_t, const float* d_w, int N, long long count, float loss_weight,
                        float* d_terms, float* d_dx, void* d_result) {
  MNC_REQUIRE(ctx && d_result, "mnc_sigmoid_ce_loss: null ctx or d_result");
  MNC_REQUIRE(N >= 0 && count >= 0 && count < (1LL << 31), "mnc_sigmoid_ce_loss: N=%d, count=%lld: negative, or 2^31 elements or more", N, count);
  if (N == 0 || count == 0) return loss_zero_result(ctx, d_result);
  MNC_REQUIRE(d_x && d_t, "mnc_sigmoid_ce_loss: null input");
  const int groups = loss_groups((long)count);
  int rc = ensure_scratch(ctx, kLossMaxGroups * sizeof(LossPartial));
  if (rc) return rc;
  LossPartial* part = (LossPartial*)ctx->scratch.p;
  {
    LaunchScope ls(ctx, "sigmoid_ce_loss", 0.0, 4.0 * (double)count * ((d_w ? 3.0 : 2.0) + (d_terms ? 1.0 : 0.0) + (d_dx ? 1.0 : 0.0)));
    hipLaunchKernelGGL(sigmoid_ce_loss_kernel, dim3(groups), dim3(256), 0, ctx->stream, d_x, d_t, d_w, (long)count, loss_weight / (float)N,
                       d_terms, d_dx, part);
    rc = ls.finish("sigmoid_ce_loss_kernel");
    if (rc) return rc;
  }
  rc = loss_finalize(ctx, part, groups, N, d_result);
  if (rc) return rc;
  clear_error();
  return MNC_OK;
}

int mnc_eltwise_backward(mnc_ctx* ctx, const float* d_y, const float* d_dy, float* d_dx, size_t count, int op) {
  MNC_REQUIRE(ctx && (count == 0 || (d_y && d_dy && d_dx)) && (op == 1 || op == 2), "mnc_eltwise_backward: bad argument");
  if (count == 0) {
    clear_error();
    return MNC_OK;
  }
  LaunchScope ls(ctx, "eltwise_bw", 0.0, 12.0 * (double)count);
  size_t g = (count + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(eltwise_backward_kernel, dim3((int)g), dim3(256), 0, ctx->stream, d_y, d_dy, d_dx, count, op);
  return ls.finish("eltwise_backward_kernel");
}

}  // extern "C"
