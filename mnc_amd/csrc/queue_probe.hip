// How many hardware queues do this process's streams really get?  (mnc_stream_concurrency, include/mnc_hip.h)
//
// The library's request for hardware queues (ctx.hip) is an environment variable the runtime reads once, at the process's first HIP
// call: it is void when something else initialised HIP first.  Only a measurement can tell.  Kernels of streams that share a hardware
// queue run one after the other, kernels of streams with queues of their own run side by side when there is room for them -- and a
// single 64-thread workgroup that does nothing but read the clock always finds room.
#include "mnc_internal.h"

namespace mnc {

constexpr int kProbeMaxStreams = 32;
constexpr int kProbeSpinCap = 1 << 14;       // iterations of ~0.5 us (s_sleep 16 = 1024 cycles + one clock read): 10 ms at the very most

// One workgroup of 64 threads; lane 0 stamps its entry, spins until `ticks` of the wall clock have passed or the cap is reached,
// stamps its exit.  `ticks` = 0: in and out (the warm-up pass).
__global__ __launch_bounds__(64) void queue_probe_kernel(long long* stamps, long long ticks, int cap) {
  if (threadIdx.x != 0) return;
  const long long t0 = (long long)wall_clock64();
  long long now = t0;
  for (int i = 0; i < cap && now - t0 < ticks; ++i) {
    __builtin_amdgcn_s_sleep(16);
    now = (long long)wall_clock64();
  }
  stamps[0] = t0;
  stamps[1] = now;
}

// the largest number of [start, end) intervals that hold one instant
static int max_overlap(const long long* stamps, int n) {
  int best = 0;
  for (int i = 0; i < n; ++i) {              // the maximum is reached at some interval's start
    const long long t = stamps[2 * i];
    int c = 0;
    for (int j = 0; j < n; ++j) c += stamps[2 * j] <= t && t < stamps[2 * j + 1];
    if (c > best) best = c;
  }
  return best;
}

}  // namespace mnc

using namespace mnc;

extern "C" int mnc_stream_concurrency(int device, int n_streams, int* concurrent) {
  MNC_REQUIRE(concurrent, "mnc_stream_concurrency: null pointer");
  *concurrent = 0;
  MNC_REQUIRE(n_streams >= 1 && n_streams <= kProbeMaxStreams, "mnc_stream_concurrency: n_streams %d not in 1 .. %d", n_streams,
              kProbeMaxStreams);
  int ndev = 0;
  MNC_HIP_TRY(hipGetDeviceCount(&ndev));
  MNC_REQUIRE(device >= 0 && device < ndev, "mnc_stream_concurrency: device %d out of range (have %d)", device, ndev);
  MNC_HIP_TRY(hipSetDevice(device));
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) {
    (void)hipGetLastError();
    khz = 100000;                            // the constant 100 MHz counter of the CDNA parts
  }
  const long long ticks = khz;               // 1 ms

  hipStream_t streams[kProbeMaxStreams] = {};
  long long* d_stamps = nullptr;
  long long h_stamps[2 * kProbeMaxStreams] = {};
  hipError_t e = hipSuccess;
  int made = 0;
  for (; made < n_streams && e == hipSuccess; ++made) {
    e = hipStreamCreateWithFlags(&streams[made], hipStreamNonBlocking);
    if (e != hipSuccess) break;
  }
  if (e == hipSuccess) e = hipMalloc((void**)&d_stamps, sizeof(h_stamps));
  // everything on the probe's own streams: the null stream would become a user of a hardware queue (profiles/r06_streams.txt)
  if (e == hipSuccess) e = hipMemsetAsync(d_stamps, 0, sizeof(h_stamps), streams[0]);
  if (e == hipSuccess) e = hipStreamSynchronize(streams[0]);
  // pass 0 brings every stream's queue up and loads the kernel; pass 1 is the measurement
  for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {
    for (int s = 0; s < n_streams && e == hipSuccess; ++s) {
      hipLaunchKernelGGL(queue_probe_kernel, dim3(1), dim3(64), 0, streams[s], d_stamps + 2 * s, pass ? ticks : 0LL, kProbeSpinCap);
      e = hipGetLastError();
    }
    for (int s = 0; s < n_streams; ++s) {    // (every stream is waited for, also after an error)
      const hipError_t es = hipStreamSynchronize(streams[s]);
      if (e == hipSuccess) e = es;
    }
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_stamps, d_stamps, sizeof(long long) * 2 * n_streams, hipMemcpyDeviceToHost, streams[0]);
  if (e == hipSuccess) e = hipStreamSynchronize(streams[0]);
  if (d_stamps) (void)hipFree(d_stamps);
  for (int s = 0; s < made; ++s)
    if (streams[s]) (void)hipStreamDestroy(streams[s]);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("mnc_stream_concurrency: %s", hipGetErrorString(e));
    return MNC_ERR_HIP;
  }
  *concurrent = max_overlap(h_stamps, n_streams);
  clear_error();
  return MNC_OK;
}
