// Context, device memory, error reporting and HIP-event profiling for libmnc_hip.so.
#include <atomic>
#include <climits>
#include <cstdlib>

#include "mnc_internal.h"

namespace mnc {

static thread_local char g_err[512] = "";

static const char* const kTuneNames[T_COUNT] = {
#define MNC_TUNE_NAME(n) #n,
    MNC_TUNE_KEYS(MNC_TUNE_NAME)
#undef MNC_TUNE_NAME
};

// "5" -> 5; "2,4" (a tile pair) -> 2 * 1000 + 4
static int parse_tune(const char* v) {
  const char* comma = strchr(v, ',');
  return comma ? atoi(v) * 1000 + atoi(comma + 1) : atoi(v);
}

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
void clear_error() { g_err[0] = 0; }

int arena_ensure(DevArena* a, size_t bytes, size_t slack, const char* who, hipStream_t stream, mnc_ctx* ctx, bool graph_visible) {
  if (bytes <= a->cap) return MNC_OK;
  if (ctx) {
    MNC_NO_CAPTURE(ctx, who);
    MNC_HIP_TRY(hipSetDevice(ctx->device));
  }
  if (a->p) {
    MNC_HIP_TRY(hipStreamSynchronize(stream));
    MNC_HIP_TRY(hipFree(a->p));
  }
  a->p = nullptr;
  a->cap = 0;
  if (ctx && graph_visible) ++ctx->arena_gen;     // a captured graph that holds the old address must not be replayed (pipeline.hip)
  const size_t want = bytes + slack;
  const hipError_t e = hipMalloc(&a->p, want);
  if (e != hipSuccess) {
    (void)hipGetLastError();                      // (the error is sticky: the next MNC_HIP_TRY would report it again)
    a->p = nullptr;
    set_error("%s: hipMalloc(%zu) failed: %s", who, want, hipGetErrorString(e));
    return MNC_ERR_NOMEM;
  }
  a->cap = want;
  return MNC_OK;
}

void arena_free(DevArena* a) {
  if (a->p) (void)hipFree(a->p);
  *a = DevArena();
}

int ensure_scratch(mnc_ctx* ctx, size_t bytes) {
  return arena_ensure(&ctx->scratch, bytes, bytes >> 2, "scratch arena", ctx->stream, ctx, true);
}

int CallBuf::alloc(const char* who, size_t bytes) {
  if (hipMalloc(&p, bytes) == hipSuccess) return MNC_OK;
  (void)hipGetLastError();
  p = nullptr;
  set_error("%s: hipMalloc(%zu) failed", who, bytes);
  return MNC_ERR_NOMEM;
}

int CallTimer::set(int enable, double* out_last_ms) {
  if (out_last_ms) *out_last_ms = last_ms.load();
  on.store(enable ? 1 : 0);
  if (enable) last_ms.store(-1.0);
  clear_error();
  return MNC_OK;
}

static hipEvent_t take_event(mnc_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void prof_begin(mnc_ctx* ctx, const char* name, double flops, double bytes) {
  ProfRecord r{name, take_event(ctx), take_event(ctx), flops, bytes};
  (void)hipEventRecord(r.start, ctx->stream);
  ctx->prof.push_back(r);
}
void prof_end(mnc_ctx* ctx) {
  if (!ctx->prof.empty()) (void)hipEventRecord(ctx->prof.back().stop, ctx->stream);
}

}  // namespace mnc

using namespace mnc;

extern "C" {

const char* mnc_last_error(void) { return g_err; }
#ifdef MNC_TUNING
const char* mnc_version(void) { return "mnc_hip 0.3 (gfx950, tuning build: ablation and superseded kernels included)"; }
#else
const char* mnc_version(void) { return "mnc_hip 0.3 (gfx950)"; }
#endif

int mnc_device_mem_info(int device_id, size_t* free_bytes, size_t* total_bytes) {
  MNC_REQUIRE(free_bytes && total_bytes, "mnc_device_mem_info: null pointer");
  MNC_HIP_TRY(hipSetDevice(device_id));
  MNC_HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
  clear_error();
  return MNC_OK;
}

int mnc_device_count(int* count) {
  MNC_REQUIRE(count, "mnc_device_count: null pointer");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *count = n;
  clear_error();
  return MNC_OK;
}

// Round 6: the HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); a host that keeps more images in flight
// than that has streams sharing a queue, and a shared queue serialises them (profiles/r06_streams.txt: the dip at the fifth stream).
// With 16 queues twelve images in flight measure 280.6 images/s against 270.0 with four (fp32, one box, two runs each; 8 queues / 8
// images: 278.2; twelve images on four queues: 264.9).  The variable is read when the runtime initialises -- at the process's first
// HIP call -- so the library makes its request when it is loaded, before it makes any.
//
// The request (profiles/hw_queues.txt): MNC_HW_QUEUES unset = 16, "0" = leave the runtime's variable alone, any other integer clamped
// to 4 .. 32 (below 4 the runtime can crash replaying a captured graph with parallel branches; 32 is the most a shared machine
// grants); text that is no integer counts as unset.  An exported GPU_MAX_HW_QUEUES that is absent, no positive integer, or LOWER
// than the request is raised to the request; one that is equal or higher is kept -- the library never lowers it.  (Until this
// change an exported value always won: a machine that exports the runtime's own default of 4 in front of every command ran twelve
// streams on four queues without a word.)  MNC_HW_QUEUES is the one way to opt out or to choose.
static int parse_int(const char* s, long* out) {      // the whole string is one integer (blanks around it allowed)
  if (!s) return 0;
  char* end = nullptr;
  const long v = strtol(s, &end, 10);                 // (an integer too large for a long comes back as LONG_MAX / LONG_MIN: clamped like any other)
  if (end == s) return 0;
  while (*end == ' ' || *end == '\t' || *end == '\n') ++end;
  if (*end) return 0;
  *out = v;
  return 1;
}

// MNC_HW_QUEUES -> the request: 0 = leave the variable alone, else 4 .. 32
static int hw_queue_want(const char* setting) {
  long want = 16;
  if (!parse_int(setting, &want)) return 16;
  return want == 0 ? 0 : want < 4 ? 4 : want > 32 ? 32 : (int)want;
}

// GPU_MAX_HW_QUEUES as exported -> its value, 0 when absent or no positive integer
static int hw_queue_exported(const char* exported) {
  long have = 0;
  if (!parse_int(exported, &have) || have <= 0) return 0;
  return have > INT_MAX ? INT_MAX : (int)have;
}

static int hw_queue_decide(int have, int want, int* value) {
  *value = want != 0 && have < want ? want : have;
  return want == 0 ? MNC_HWQ_UNTOUCHED : have >= want ? MNC_HWQ_KEPT : MNC_HWQ_RAISED;
}

static int g_hwq_requested = 0, g_hwq_exported_before = -1, g_hwq_action = MNC_HWQ_UNTOUCHED;

int mnc_hw_queue_policy(const char* exported, const char* setting, int* value, int* action) {
  MNC_REQUIRE(value && action, "mnc_hw_queue_policy: null pointer");
  *action = hw_queue_decide(hw_queue_exported(exported), hw_queue_want(setting), value);
  clear_error();
  return MNC_OK;
}

// The hook.  A constructor, because the request only counts before the process's first HIP call and the library cannot know which of
// its entries that will be.  getenv / setenv are not safe against other threads using the environment at the same moment: a host that
// dlopen()s the library late, while other threads may call getenv, exports GPU_MAX_HW_QUEUES itself before it starts them (and sets
// MNC_HW_QUEUES=0).  No other variable of the runtime is touched.  Overriding a value the host exported prints one line on stderr.  mnc_hw_queue_request reports what happened here;
// mnc_stream_concurrency (queue_probe.hip) measures what the runtime really gave -- the request is void when something else
// initialised HIP before the library was loaded.
__attribute__((constructor)) static void mnc_request_hw_queues() {
  const int have = hw_queue_exported(getenv("GPU_MAX_HW_QUEUES"));
  int value = 0;
  g_hwq_requested = hw_queue_want(getenv("MNC_HW_QUEUES"));
  g_hwq_exported_before = have > 0 ? have : -1;
  g_hwq_action = hw_queue_decide(have, g_hwq_requested, &value);
  if (g_hwq_action == MNC_HWQ_RAISED) {
    char buf[16];
    snprintf(buf, sizeof(buf), "%d", value);
    setenv("GPU_MAX_HW_QUEUES", buf, /*overwrite=*/1);
    // a value the host exported itself is overridden: say so, once per process, where an operator looks
    if (have > 0)
      fprintf(stderr, "libmnc_hip: GPU_MAX_HW_QUEUES raised from %d to %d for this process (MNC_HW_QUEUES=0 keeps the exported value)\n",
              have, value);
  }
}

int mnc_hw_queue_request(int* requested, int* exported_before, int* action) {
  MNC_REQUIRE(requested && exported_before && action, "mnc_hw_queue_request: null pointer");
  *requested = g_hwq_requested;
  *exported_before = g_hwq_exported_before;
  *action = g_hwq_action;
  clear_error();
  return MNC_OK;
}

int mnc_ctx_create(mnc_ctx** out, int device_id) {
  MNC_REQUIRE(out, "mnc_ctx_create: null out pointer");
  *out = nullptr;
  int n = 0;
  MNC_HIP_TRY(hipGetDeviceCount(&n));
  MNC_REQUIRE(device_id >= 0 && device_id < n, "mnc_ctx_create: device %d out of range (have %d)", device_id, n);
  MNC_HIP_TRY(hipSetDevice(device_id));
  mnc_ctx* ctx = new (std::nothrow) mnc_ctx();
  if (!ctx) {
    set_error("mnc_ctx_create: out of host memory");
    return MNC_ERR_NOMEM;
  }
  ctx->device = device_id;
  for (int k = 0; k < T_COUNT; ++k) {                 // the environment is read here, once per context, never on a launch path
    char name[64];
    snprintf(name, sizeof(name), "MNC_%s", kTuneNames[k]);
    const char* v = getenv(name);
    ctx->tune[k] = v && *v ? parse_tune(v) : kTuneUnset;
  }
  hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete ctx;
    set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
    return MNC_ERR_HIP;
  }
  e = hipMalloc((void**)&ctx->tickets, kTickets * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemsetAsync(ctx->tickets, 0, kTickets * sizeof(unsigned), ctx->stream);   // (ordered before the stream's launches)
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    if (ctx->tickets) (void)hipFree(ctx->tickets);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    set_error("mnc_ctx_create: arrival tickets: %s", hipGetErrorString(e));
    return MNC_ERR_HIP;
  }
  *out = ctx;
  clear_error();
  return MNC_OK;
}

int mnc_ctx_destroy(mnc_ctx* ctx) {
  if (!ctx) return MNC_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& r : ctx->prof) {
    (void)hipEventDestroy(r.start);
    (void)hipEventDestroy(r.stop);
  }
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  arena_free(&ctx->scratch);
  if (ctx->proposal) mnc::proposal_state_free(ctx->proposal);
  arena_free(&ctx->vote_ws);
  arena_free(&ctx->render_ws);
  arena_free(&ctx->mask_ws);
  arena_free(&ctx->overlap_ws);
  arena_free(&ctx->rle_ws);
  arena_free(&ctx->match_ws);
  if (ctx->tickets) (void)hipFree(ctx->tickets);
  if (ctx->comm) mnc::comm_free(ctx);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  clear_error();
  return MNC_OK;
}

int mnc_ctx_sync(mnc_ctx* ctx) {
  MNC_REQUIRE(ctx, "mnc_ctx_sync: null context");
  MNC_NO_CAPTURE(ctx, "mnc_ctx_sync");
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    // A launch that failed or faulted midway may have left arrival tickets of the in-launch K-range reductions non-zero
    // (mnc_internal.h: slab_last_arriver resets a tile's ticket only when its last workgroup arrives); every later launch would
    // then never see "arrivals - 1" and leave its tiles unfinished.  Put the counters back before reporting the error.
    if (ctx->tickets) (void)hipMemsetAsync(ctx->tickets, 0, mnc::kTickets * sizeof(unsigned), ctx->stream);
    mnc::set_error("hipStreamSynchronize failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    return MNC_ERR_HIP;
  }
  clear_error();
  return MNC_OK;
}

int mnc_ctx_device(const mnc_ctx* ctx, int* device_id) {
  MNC_REQUIRE(ctx && device_id, "mnc_ctx_device: null pointer");
  *device_id = ctx->device;
  return MNC_OK;
}

int mnc_ctx_arena_generation(const mnc_ctx* ctx, unsigned long* generation) {
  MNC_REQUIRE(ctx && generation, "mnc_ctx_arena_generation: null pointer");
  *generation = ctx->arena_gen;
  return MNC_OK;
}

int mnc_ctx_capture_begin(mnc_ctx* ctx) {
  MNC_REQUIRE(ctx, "mnc_ctx_capture_begin: null context");
  MNC_REQUIRE(!ctx->capturing, "mnc_ctx_capture_begin: a capture is already open on this context");
  if (ctx->profiling != 0) {       // LaunchScope would record event pairs into the captured stream: they never execute
    set_error("mnc_ctx_capture_begin: per-launch profiling is on (mnc_prof_enable); event pairs cannot be captured");
    return MNC_ERR_STATE;
  }
  MNC_HIP_TRY(hipSetDevice(ctx->device));
  MNC_HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
  ctx->capturing = true;
  ctx->capture_gen = ctx->arena_gen;
  clear_error();
  return MNC_OK;
}

int mnc_ctx_capture_end(mnc_ctx* ctx, mnc_graph** out) {
  MNC_REQUIRE(ctx && out, "mnc_ctx_capture_end: null pointer");
  *out = nullptr;
  MNC_REQUIRE(ctx->capturing, "mnc_ctx_capture_end: no capture is open on this context");
  ctx->capturing = false;
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(ctx->stream, &g);
  if (e != hipSuccess || !g) {
    (void)hipGetLastError();
    if (g) (void)hipGraphDestroy(g);
    set_error("mnc_ctx_capture_end: the capture was invalidated (%s): something synchronised or allocated inside it",
              hipGetErrorString(e));
    return MNC_ERR_HIP;
  }
  if (ctx->capture_gen != ctx->arena_gen) {          // an internal arena moved while capturing: earlier nodes hold the old address
    (void)hipGraphDestroy(g);
    set_error("mnc_ctx_capture_end: an internal arena was re-allocated during the capture (run the sequence eagerly once first)");
    return MNC_ERR_STATE;
  }
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess || !exec) {
    (void)hipGetLastError();
    set_error("mnc_ctx_capture_end: hipGraphInstantiate failed: %s", hipGetErrorString(e));
    return MNC_ERR_HIP;
  }
  mnc_graph* gr = new (std::nothrow) mnc_graph();
  if (!gr) { (void)hipGraphExecDestroy(exec); set_error("mnc_ctx_capture_end: out of host memory"); return MNC_ERR_NOMEM; }
  gr->exec = exec;
  gr->ctx = ctx;
  gr->arena_gen = ctx->arena_gen;
  *out = gr;
  clear_error();
  return MNC_OK;
}

int mnc_graph_launch(mnc_ctx* ctx, mnc_graph* graph) {
  MNC_REQUIRE(ctx && graph && graph->ctx == ctx, "mnc_graph_launch: null pointer, or a graph of another context");
  if (graph->arena_gen != ctx->arena_gen) {
    set_error("mnc_graph_launch: an internal arena of the context was re-allocated since the capture; capture again");
    return MNC_ERR_STATE;
  }
  MNC_HIP_TRY(hipSetDevice(ctx->device));
  MNC_HIP_TRY(hipGraphLaunch(graph->exec, ctx->stream));
  return MNC_OK;
}

int mnc_graph_destroy(mnc_graph* graph) {
  if (!graph) return MNC_OK;
  if (graph->exec) (void)hipGraphExecDestroy(graph->exec);
  delete graph;
  return MNC_OK;
}

int mnc_ctx_set_tuning(mnc_ctx* ctx, const char* name, const char* value) {
  MNC_REQUIRE(ctx && name, "mnc_ctx_set_tuning: null pointer");
  if (!strncmp(name, "MNC_", 4)) name += 4;
  for (int k = 0; k < T_COUNT; ++k)
    if (!strcmp(name, kTuneNames[k])) {
      ctx->tune[k] = value && *value ? parse_tune(value) : kTuneUnset;
      clear_error();
      return MNC_OK;
    }
  set_error("mnc_ctx_set_tuning: unknown key %s", name);
  return MNC_ERR_INVALID;
}

int mnc_ctx_set_layer_conventions(mnc_ctx* ctx, const mnc_layer_conventions* conv) {
  MNC_REQUIRE(ctx, "mnc_ctx_set_layer_conventions: null context");
  const mnc_layer_conventions spec = {0, 0, 0, 0, 0, 0, 0.4f, 0};
  const mnc_layer_conventions c = conv ? *conv : spec;
  MNC_REQUIRE(c.warp_sample >= 0 && c.warp_sample <= 2, "layer conventions: warp_sample %d not in {0,1,2}", c.warp_sample);
  MNC_REQUIRE(c.resize_mode >= 0 && c.resize_mode <= 2, "layer conventions: resize_mode %d not in {0,1,2}", c.resize_mode);
  MNC_REQUIRE((c.warp_round_edges | 1) == 1 && (c.warp_no_plus_one | 1) == 1 && (c.warp_oob | 1) == 1 && (c.maskpool_binary | 1) == 1,
              "layer conventions: warp_round_edges / warp_no_plus_one / warp_oob / maskpool_binary are 0 or 1");
  MNC_REQUIRE(c.maskpool_thresh == c.maskpool_thresh, "layer conventions: maskpool_thresh is NaN");
  ctx->conv = c;
  ctx->conv.inherit = 0;
  clear_error();
  return MNC_OK;
}

int mnc_ctx_get_layer_conventions(const mnc_ctx* ctx, mnc_layer_conventions* conv) {
  MNC_REQUIRE(ctx && conv, "mnc_ctx_get_layer_conventions: null pointer");
  *conv = ctx->conv;
  return MNC_OK;
}

int mnc_dev_alloc(mnc_ctx* ctx, size_t bytes, void** d_ptr) {
  MNC_REQUIRE(ctx && d_ptr, "mnc_dev_alloc: null pointer");
  *d_ptr = nullptr;
  MNC_NO_CAPTURE(ctx, "mnc_dev_alloc");
  MNC_HIP_TRY(hipSetDevice(ctx->device));
  hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 16);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("mnc_dev_alloc: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return MNC_ERR_NOMEM;
  }
  clear_error();
  return MNC_OK;
}

int mnc_dev_free(mnc_ctx* ctx, void* d_ptr) {
  MNC_REQUIRE(ctx, "mnc_dev_free: null context");
  if (!d_ptr) return MNC_OK;
  MNC_NO_CAPTURE(ctx, "mnc_dev_free");
  MNC_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MNC_HIP_TRY(hipFree(d_ptr));
  return MNC_OK;
}

int mnc_host_alloc(mnc_ctx* ctx, size_t bytes, void** host_ptr) {
  MNC_REQUIRE(ctx && host_ptr, "mnc_host_alloc: null pointer");
  *host_ptr = nullptr;
  MNC_HIP_TRY(hipSetDevice(ctx->device));
  hipError_t e = hipHostMalloc(host_ptr, bytes ? bytes : 16, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("mnc_host_alloc: hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return MNC_ERR_NOMEM;
  }
  clear_error();
  return MNC_OK;
}

int mnc_host_free(mnc_ctx* ctx, void* host_ptr) {
  MNC_REQUIRE(ctx, "mnc_host_free: null context");
  if (!host_ptr) return MNC_OK;
  MNC_NO_CAPTURE(ctx, "mnc_host_free");
  MNC_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MNC_HIP_TRY(hipHostFree(host_ptr));
  return MNC_OK;
}

int mnc_h2d_async(mnc_ctx* ctx, void* d_dst, const void* src_host, size_t bytes) {
  MNC_REQUIRE(ctx && (bytes == 0 || (d_dst && src_host)), "mnc_h2d_async: null pointer");
  if (bytes == 0) return MNC_OK;
  MNC_HIP_TRY(hipMemcpyAsync(d_dst, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return MNC_OK;
}

int mnc_d2h_async(mnc_ctx* ctx, void* dst_host, const void* d_src, size_t bytes) {
  MNC_REQUIRE(ctx && (bytes == 0 || (dst_host && d_src)), "mnc_d2h_async: null pointer");
  if (bytes == 0) return MNC_OK;
  MNC_HIP_TRY(hipMemcpyAsync(dst_host, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return MNC_OK;
}

int mnc_h2d(mnc_ctx* ctx, void* d_dst, const void* src_host, size_t bytes) {
  MNC_REQUIRE(ctx && (bytes == 0 || (d_dst && src_host)), "mnc_h2d: null pointer");
  if (bytes == 0) return MNC_OK;
  MNC_NO_CAPTURE(ctx, "mnc_h2d");
  MNC_HIP_TRY(hipMemcpyAsync(d_dst, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  MNC_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MNC_OK;
}

int mnc_d2h(mnc_ctx* ctx, void* dst_host, const void* d_src, size_t bytes) {
  MNC_REQUIRE(ctx && (bytes == 0 || (dst_host && d_src)), "mnc_d2h: null pointer");
  if (bytes == 0) return MNC_OK;
  MNC_NO_CAPTURE(ctx, "mnc_d2h");
  MNC_HIP_TRY(hipMemcpyAsync(dst_host, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  MNC_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MNC_OK;
}

int mnc_d2d(mnc_ctx* ctx, void* d_dst, const void* d_src, size_t bytes) {
  MNC_REQUIRE(ctx && (bytes == 0 || (d_dst && d_src)), "mnc_d2d: null pointer");
  if (bytes == 0) return MNC_OK;
  MNC_HIP_TRY(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return MNC_OK;
}

int mnc_dev_zero(mnc_ctx* ctx, void* d_ptr, size_t bytes) {
  MNC_REQUIRE(ctx && (bytes == 0 || d_ptr), "mnc_dev_zero: null pointer");
  if (bytes == 0) return MNC_OK;
  MNC_HIP_TRY(hipMemsetAsync(d_ptr, 0, bytes, ctx->stream));
  return MNC_OK;
}

int mnc_prof_enable(mnc_ctx* ctx, int enable) {
  MNC_REQUIRE(ctx, "mnc_prof_enable: null context");
  ctx->profiling = enable < 0 ? 0 : (enable > 2 ? 1 : enable);
  return MNC_OK;
}

int mnc_prof_reset(mnc_ctx* ctx) {
  MNC_REQUIRE(ctx, "mnc_prof_reset: null context");
  MNC_NO_CAPTURE(ctx, "mnc_prof_reset");
  MNC_HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (auto& r : ctx->prof) {
    ctx->event_pool.push_back(r.start);
    ctx->event_pool.push_back(r.stop);
  }
  ctx->prof.clear();
  return MNC_OK;
}

int mnc_prof_count(mnc_ctx* ctx, int* n_records) {
  MNC_REQUIRE(ctx && n_records, "mnc_prof_count: null pointer");
  MNC_NO_CAPTURE(ctx, "mnc_prof_count");
  MNC_HIP_TRY(hipStreamSynchronize(ctx->stream));
  *n_records = (int)ctx->prof.size();
  return MNC_OK;
}

int mnc_prof_get(mnc_ctx* ctx, int index, char* name_buf, int name_cap, float* ms, double* flops, double* bytes) {
  MNC_REQUIRE(ctx && index >= 0 && index < (int)ctx->prof.size(), "mnc_prof_get: index %d out of range", index);
  const ProfRecord& r = ctx->prof[index];
  if (name_buf && name_cap > 0) {
    strncpy(name_buf, r.name, name_cap - 1);
    name_buf[name_cap - 1] = 0;
  }
  if (ms) {
    float t = 0.f;
    MNC_HIP_TRY(hipEventElapsedTime(&t, r.start, r.stop));
    *ms = t;
  }
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  return MNC_OK;
}

}  // extern "C"
