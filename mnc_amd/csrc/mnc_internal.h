// Internal header of libmnc_hip.so (gfx950 only).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mnc_hip.h"
#include "tune.h"
#include "ws_layout.h"

namespace mnc {

// A device buffer that only grows (arena_ensure, ctx.hip).
struct DevArena {
  void* p = nullptr;
  size_t cap = 0;
};

void set_error(const char* fmt, ...);
void clear_error();

struct ProfRecord {
  const char* name;
  hipEvent_t start, stop;
  double flops, bytes;
};

}  // namespace mnc

namespace mnc {
constexpr int kTickets = 4096;     // mnc_ctx::tickets
}  // namespace mnc

struct mnc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int profiling = 0;   // 0 off, 1 every launch, 2 only launches with >= 1 GFLOP of algorithmic work (the MFMA kernels)
  std::vector<mnc::ProfRecord> prof;
  std::vector<hipEvent_t> event_pool;
  mnc::DevArena scratch;      // split-K scratch for mnc_fc and friends; grown on demand, never shrunk
  void* proposal = nullptr;   // mnc_proposal_state (proposal.hip), created on first use
  mnc::DevArena vote_ws;      // gpu_mask_voting scratch (mv.hip), grown on demand
  mnc::DevArena render_ws;    // instance descriptors of mnc_render_records (render.hip), grown on demand; in no captured graph
  mnc::DevArena mask_ws;      // head, instance table and bits of mnc_mask_records (inst_masks.hip), grown on demand; in no captured graph
  mnc::DevArena rle_ws;       // result and scan buffers of mnc_mask_rle_dev (mask_rle.hip), grown on demand; in no captured graph
  mnc::DevArena overlap_ws;   // uploaded B set, matrices and NMS buffers of mnc_mask_overlaps_dev / mnc_mask_nms_dev (mask_overlaps.hip); in no captured graph
  mnc::DevArena match_ws;     // uploaded ground truth, lists, IoU tables and result tables of mnc_mask_match_dev (mask_match.hip); in no captured graph
  void* comm = nullptr;       // RCCL communicator state (comm.hip), set by mnc_comm_init
  // Arrival tickets of the K-range reductions that finish INSIDE the launch (gemm.hip, conv_wino4.hip): kTickets counters, zero
  // between launches -- allocated and zeroed with the context, every launch's last arriver of a tile puts its counter back to
  // zero.  Launches of one context are stream-ordered, so all of them share the array.
  unsigned* tickets = nullptr;
  // mnc_fc with defer_reduce set leaves the K ranges' partial sums in `scratch` ([splits][M][N]) instead of launching
  // fc_reduce_kernel and reports them here: the caller's next kernel sums them in range order itself (pipeline.hip: the sibling
  // classifiers' reduction, softmax, stage bridge and im_detect tail as one launch).  deferred_splits == 1: `out` is complete.
  bool defer_reduce = false;
  const float* deferred_part = nullptr;
  int deferred_splits = 0;
  // Bumped whenever one of the context-owned arenas above (scratch, proposal state, voting scratch) is re-allocated: a captured
  // HIP graph holds their raw addresses, so a graph owner (pipeline.hip) records the value at capture and drops its graph when
  // the value has moved on.  Written by arena_ensure (ctx.hip) and by nothing else.
  unsigned long arena_gen = 0;
  // conventions of the three Caffe layers whose source is unavailable (all zero = oracle/SPEC.md); read by roi.hip's launchers
  mnc_layer_conventions conv = {0, 0, 0, 0, 0, 0, 0.4f, 0};
  bool capturing = false;     // between mnc_ctx_capture_begin / _end
  unsigned long capture_gen = 0;
  int tune[mnc::T_COUNT];     // kTuneUnset = the launcher decides (filled by mnc_ctx_create; mnc_ctx_set_tuning)
};

struct mnc_graph {
  hipGraphExec_t exec = nullptr;
  mnc_ctx* ctx = nullptr;
  unsigned long arena_gen = 0;
};

namespace mnc {
inline bool tune_set(const mnc_ctx* ctx, TuneKey k) { return tune_set(ctx->tune, k); }
inline int tune(const mnc_ctx* ctx, TuneKey k, int dflt) { return tune(ctx->tune, k, dflt); }
inline bool plan_latency(const mnc_ctx* ctx) { return plan_latency(ctx->tune); }
#ifdef MNC_TUNING
constexpr bool kTuningBuild = true;       // the ablation and superseded kernels are compiled in; plans may have to make room for them
#else
constexpr bool kTuningBuild = false;
#endif
}  // namespace mnc

namespace mnc {

// Makes `a` hold at least `bytes`, growing it to bytes + slack: waits for `stream` (work in flight may use the old buffer), frees,
// allocates.  With a context: refuses while a launch sequence is captured, selects the context's device and, when graph_visible,
// moves ctx->arena_gen -- once per re-allocation, also when the allocation then fails.  Without one (the host-array entry points'
// workspace) the caller has selected the device.  `who` names the arena in the error message.
int arena_ensure(DevArena* a, size_t bytes, size_t slack, const char* who, hipStream_t stream, mnc_ctx* ctx = nullptr,
                 bool graph_visible = false);
void arena_free(DevArena* a);
int ensure_scratch(mnc_ctx* ctx, size_t bytes);
void prof_begin(mnc_ctx* ctx, const char* name, double flops, double bytes);
void prof_end(mnc_ctx* ctx);

#define MNC_HIP_TRY(expr)                                                                    \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      mnc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
      return MNC_ERR_HIP;                                                                    \
    }                                                                                        \
  } while (0)

// Entry points that synchronise the stream or re-allocate an arena refuse to run while a launch sequence is being captured on the
// context (mnc_ctx_capture_begin): the call fails BEFORE it touches the stream, so the capture itself stays valid and can be ended
// and discarded cleanly (a hipStreamSynchronize inside a capture leaves the stream unusable on this runtime).
#define MNC_NO_CAPTURE(ctx, what)                                                                        \
  do {                                                                                                   \
    if ((ctx)->capturing) {                                                                              \
      mnc::set_error("%s: synchronises or re-allocates; not allowed while a launch sequence is captured", what); \
      return MNC_ERR_STATE;                                                                              \
    }                                                                                                    \
  } while (0)

#define MNC_REQUIRE(cond, ...)       \
  do {                               \
    if (!(cond)) {                   \
      mnc::set_error(__VA_ARGS__);   \
      return MNC_ERR_INVALID;        \
    }                                \
  } while (0)

// Raises a kernel's dynamic-LDS limit the first time the kernel is launched on a device (function attributes are per device): one
// bitmask per kernel instantiation, one bit per device.
template <auto kKernel>
inline hipError_t lds_limit_once(int device, int bytes) {
  static std::atomic<unsigned long long> done{0};
  const unsigned long long bit = 1ull << (device & 63);
  if (done.load(std::memory_order_relaxed) & bit) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
  return e;
}

// RAII bracket: records a HIP event pair around the kernels launched inside its scope when profiling is on, and
// turns a failed launch into MNC_ERR_HIP.
struct LaunchScope {
  mnc_ctx* ctx;
  bool on;
  LaunchScope(mnc_ctx* c, const char* name, double flops = 0.0, double bytes = 0.0) : ctx(c) {
    (void)hipSetDevice(ctx->device);    // several contexts on different GPUs may live in one process
    on = ctx->profiling == 1 || (ctx->profiling == 2 && flops >= 1.0e9);
    if (on) prof_begin(ctx, name, flops, bytes);
  }
  int finish(const char* name) {
    if (on) prof_end(ctx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      set_error("kernel launch %s failed: %s", name, hipGetErrorString(e));
      return MNC_ERR_HIP;
    }
    return MNC_OK;
  }
};

// XCD-aware block order for the GEMMs.  The dispatcher places block b on XCD b % 8 (observed, used for speed only:
// a different placement changes nothing but L2 hit rates).  Blocks are re-numbered so that each XCD receives a
// CONTIGUOUS range of the logical order (column tile fastest, then K split, then row block): the workgroups that share
// one K split's activation panel then sit on one XCD and the panel stays in that XCD's 4 MB L2 instead of being
// re-fetched from Infinity Cache by every column tile.  Bijective for any block count (cdna_hip_programming.md, T1).
__device__ __forceinline__ void xcd_decode(int bid, int tn, int splits, int tm, int& bn, int& split, int& bm) {
  const int total = tn * splits * tm;
  const int q = total >> 3, r = total & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  bn = logical % tn;
  const int rest = logical / tn;
  split = rest % splits;
  bm = rest / splits;
}

// ---- K ranges finished inside the launch (cdna_hip_programming.md section 5, "In-launch split-K reduction"; Guideline 16) ----
// Every workgroup of an output tile stores its partial sums as a SLAB in its own register layout (16-byte pieces, lane-contiguous,
// write-through `sc1` stores: no release fence), drains them, and draws an arrival ticket; the workgroup that draws the last one
// reads all slabs of the tile (sc1 loads behind one agent-scope acquire), adds them IN RANGE ORDER -- the order of the separate
// reduction kernels, so the results are the same bits whichever workgroup arrives last -- and writes the finished tile.  Nobody
// waits for anybody: a launch whose workgroups are not co-resident (several streams share the GPU) cannot deadlock.
// Memory-model assumption (MI355X_MICROARCH.md, "Valid forms"): sc1 stores are write-through to the memory side, the asm
// `s_waitcnt vmcnt(0)` in front of the barrier retires them before the ticket's relaxed agent-scope atomic can issue, and the last
// arriver reads them behind ONE agent-scope acquire -- there is no formal release fence; the ordering is the drained write-through.
// A launch that is aborted midway leaves tickets non-zero: mnc_ctx_sync zeroes the array when the stream reports an error.
typedef unsigned mnc_u32x4 __attribute__((ext_vector_type(4)));
typedef float mnc_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slab_rsrc(float* base) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7FFFFFF0, 0x00020000);
}
__device__ __forceinline__ void slab_store(__amdgpu_buffer_rsrc_t rs, int voff, int soff, mnc_f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(mnc_u32x4, v), rs, voff, soff, /*sc1*/ 16);
}
__device__ __forceinline__ mnc_f32x4 slab_load(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(mnc_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, /*sc1*/ 16));
}
// All threads of the workgroup call it after their slab stores; `flag` is a free LDS word of the kernel's ONE shared array (a
// second __shared__ object de-pipelines LDS-DMA loops).  True in every thread of the tile's last arriver, which also puts the
// ticket back to zero for the next launch and has acquired the other workgroups' slabs.
__device__ __forceinline__ bool slab_last_arriver(unsigned* ticket, int arrivals, volatile unsigned* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's write-through slab stores have left
  __syncthreads();
  if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const bool last = __builtin_amdgcn_readfirstlane(*flag) == (unsigned)(arrivals - 1);
  if (last) {
    if (threadIdx.x == 0) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
  }
  return last;
}

// A device buffer of one call, freed on every way out: for entry points whose need grows with a whole dataset (~0.5 KB per
// prediction in mnc_sds_best_overlap), too much to keep in an arena.
struct CallBuf {
  void* p = nullptr;
  ~CallBuf() { if (p) (void)hipFree(p); }
  int alloc(const char* who, size_t bytes);   // ctx.hip
};

// Scope of a host-array entry point (_nms, _mv, mnc_mask_voting*, mnc_sds_best_overlap, mnc_mcg_maskdb, mnc_render_instances,
// mnc_instance_masks, mnc_mask_overlaps, mnc_mask_nms, mnc_mask_rle, mnc_mask_from_rle, mnc_mask_match, mnc_mask_match_boundary,
// mnc_mask_boundary, mnc_mask_from_polygons, mnc_coco_accumulate, mnc_mask_components / _select / _fill_holes / _split, mnc_mask_contours, mnc_contours_simplify, mnc_mask_distance / _inscribed / _morph, mnc_mask_moments / _hull / _oriented, mnc_mask_combine / _merge / _layer, mnc_mask_isometry, mnc_mask_warp, mnc_label_table / _masks, mnc_mask_to_labels, mnc_mask_pixel_stats, mnc_mask_histogram, mnc_mask_surface / _surface_stats / _surface_dist, mnc_mask_targets, mnc_mask_pred_overlaps): the device's stream and growable workspace (the reference cudaMalloc/cudaFree's its scratch on every call: nms_kernel.cu:99-143,
// mv_kernel.cu:250-347) with the workspace's mutex HELD until the scope ends -- taken before the buffer may be re-allocated:
// ctypes releases the GIL, so two host threads may be inside such entry points on one device.
struct HostScope {
  std::unique_lock<std::mutex> lock;
  hipStream_t stream = nullptr;
  void* buf = nullptr;                        // at least the `bytes` of open(); null when it asked for none
  int open(int device_id, size_t bytes);      // nms.hip: device check, lock, stream, workspace
  // asynchronous copies on `stream`; nothing is enqueued for zero bytes
  hipError_t up(void* d_dst, const void* src, size_t bytes) const {
    return bytes ? hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess;
  }
  hipError_t down(void* dst, const void* d_src, size_t bytes) const {
    return bytes ? hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, stream) : hipSuccess;
  }
  hipError_t sync() const { return hipStreamSynchronize(stream); }
};

// The switch and the kept figure behind one mnc_*_timing entry (boundary, polygons, accumulate, components, contours, simplify, distance, shape, algebra, warp, labels, pixels, surface, targets): off and -1.0 until
// the entry is called.
struct CallTimer {
  std::atomic<int> on{0};
  std::atomic<double> last_ms{-1.0};
  int set(int enable, double* out_last_ms);   // ctx.hip: the whole of an mnc_*_timing entry
};

// A HIP event pair around one group of launches of a call, for its timer.  The events exist only while the timer is on; with it off
// begin() is one relaxed load and end() / keep() one bool test.  A span that was never begun, or one of whose event calls failed,
// keeps nothing.
struct TimedSpan {
  CallTimer& timer;
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false;
  explicit TimedSpan(CallTimer& t) : timer(t) {}
  TimedSpan(const TimedSpan&) = delete;
  ~TimedSpan() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void begin(hipStream_t s) {
    if (!timer.on.load(std::memory_order_relaxed)) return;
    on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, s) == hipSuccess;
  }
  void end(hipStream_t s) { if (on) on = hipEventRecord(b, s) == hipSuccess; }
  // All three after the stream was synchronised.  ms() is not const: a failed hipEventElapsedTime switches the span off.
  double ms() {
    float t = 0.f;
    if (on) on = hipEventElapsedTime(&t, a, b) == hipSuccess;
    return on ? (double)t : 0.0;
  }
  void keep() {
    const double t = ms();
    if (on) timer.last_ms.store(t);
  }
  // the sum of an earlier span of the same call and this one; nothing when either is off or failed
  void keep_sum(TimedSpan& earlier) {
    const double t = earlier.ms() + ms();
    if (on && earlier.on) timer.last_ms.store(t);
  }
};

// launchers shared between translation units (all asynchronous on `stream`, pointers are device pointers)
int nms_mask_launch(hipStream_t stream, const float* d_boxes, const int* d_order, int n, int dim, float thr,
                    unsigned long long* d_mask, int batch);
int nms_scan_launch(hipStream_t stream, const unsigned long long* d_mask, int n, int max_keep, int* d_keep, int* d_num,
                    int batch);
// same, with the box count read from device memory (*d_n <= n_cap); buffers are sized for n_cap
int nms_mask_launch_indirect(hipStream_t stream, const float* d_boxes, const int* d_order, const int* d_n, int n_cap,
                             int dim, float thr, unsigned long long* d_mask);
int nms_scan_launch_indirect(hipStream_t stream, const unsigned long long* d_mask, const int* d_n, int n_cap, int max_keep,
                             int* d_keep, int* d_num, const float* d_gather_boxes = nullptr, const int* d_gather_order = nullptr,
                             float* d_rois = nullptr, int rois_cap = 0);   // d_rois: the ProposalLayer's RoI rows written by the same launch
void proposal_state_free(void* state);  // proposal.hip
void comm_free(mnc_ctx* ctx);           // comm.hip
void fc_reduce_launch(hipStream_t stream, const float* part, const float* bias, float* out, int M, int N, int ldc, int splits,
                      int act);   // gemm.hip: out = act(sum of the K splits' partial sums + bias), shared by the three FC kernels
bool fc_reduce_launch_sm(hipStream_t stream, const float* part, const float* bias, float* out, int M, int N, int ldc, int splits,
                         int act, void* sm, int sm_fmt, long sm_rows, long sm_row0);   // + the rows in the next InnerProduct's form
// gemm.hip: B InnerProducts of one shape at constant strides (floats) in one launch of the eight-wave LDS-DMA kernel; launch only
int fc_batch_launch(mnc_ctx* ctx, const float* d_a, long stride_a, const float* d_w, long stride_w, float* d_out, long stride_o, int B,
                    int M, int N, int K, int ldc);
// conv_wino4_split.hip: can the split form run this layer at all / does this context's WINO_SPLIT value move it there?
bool wino4_split_supported(int H, int W, int Cin, int Cout);
bool wino4_split_selected(const mnc_ctx* ctx, int H, int W, int Cin, int Cout);
bool fc_reduce_pair_launch_sm(hipStream_t stream, const float* part0, const float* part1, const float* bias0, const float* bias1,
                              float* out0, float* out1, int M, int N, int ldc, int splits, int act, void* sm0, void* sm1, int sm_fmt,
                              long sm_rows, bool* sm_done);   // two products' reductions in one launch (gemm.hip)
// conv.hip: out = act(sum of the ksplit partial c8 tensors + bias)
void conv_splitk_reduce_launch(hipStream_t stream, const float* d_part, const float* d_bias, float* d_out, int H, int W,
                               int Cout, int ksplit, int relu);
// proposal.hip: finishes the sibling classifiers of a head stage in one launch -- the K ranges of [cls_score | seg_cls_score |
// bbox_pred] summed in range order + bias (fc_reduce_kernel's arithmetic), the softmax of the seg_cls_score columns
// (softmax_rows_wave_kernel's), then StageBridgeLayer.forward_test (rois_ext != nullptr) or im_detect's tail (boxes != nullptr).
int heads_finish_launch(mnc_ctx* ctx, const float* part, int splits, const float* bias, float* heads, int ld, int M, int K,
                        float* scores, const float* rois, float im_h, float im_w, float* rois_ext, const float* rois1,
                        const float* rois2, float scale, int image_height, int image_width, float* boxes, const int* copy_src,
                        int* copy_dst);
// roi.hip: the pixel-major copy of a c8 feature map the warp kernels gather from, and the warp on a copy the caller already holds
int c8_to_hwc_launch(mnc_ctx* ctx, const float* d_feat, float* d_hwc, int C, int H, int W);
int roi_warp_from_hwc(mnc_ctx* ctx, const float* d_hwc, int C, int H, int W, const float* d_rois, int R, int PH, int PW, float scale,
                      int pool2, float* d_out, void* d_sm, int sm_fmt);
bool roi_warp_sm_only_ok(const mnc_ctx* ctx, int C, int pool2);      // may d_out be null (with a stage-major output)?
int detect_tail_launch(mnc_ctx* ctx, const float* d_rois1, int R1, const float* d_rois2, int R2, float scale, int image_height,
                       int image_width, float* d_boxes, const int* d_copy_src, int* d_copy_dst);   // mv.hip: mnc_detect_tail + one int moved
int mv_launch(hipStream_t stream, const float* d_boxes, int box_dim, const float* d_masks, int S, const int* d_inds,
              const int* d_begins, const int* d_ends, const float* d_wts, int H, int W, int R, int* d_bounds,
              float* d_out_mask, int* d_out_box);
// mv_image.hip: the image-space voting kernels (cpu_mask_voting's rule) of rows [0, *d_rcount), records written as mv's
int mv_image_launch(hipStream_t stream, const float* d_boxes, const float* d_masks, int S, const int* d_inds, const int* d_begins,
                    const int* d_ends, const float* d_wts, int H, int W, double thresh, int R, const int* d_rcount, int grid_rows,
                    int* d_bounds, float* d_records, const float* d_rscore, const int* d_rows, int record_cap);

}  // namespace mnc
