// The tight result of a host entry whose size depends on the data, as mask_algebra.hip and mask_warp.hip share it: a set of packed
// masks (include/mnc_hip.h n5) of which the caller knows, before anything is launched, only a LOOSE FRAME per output instance -- a
// box outside of which the result cannot have a pixel.  Internal to libmnc_hip.so.
//
// The protocol.  A size call (out_bits == nullptr) launches nothing and returns the bytes of the loose frames, a bound.  The
// launching call, with that much room, makes five launches whatever the data and reads nothing back in between:
//   the family's extent pass   computes every word of the loose frames and hands it to tight_join: the word's row and its lowest and
//                              highest set column (ctz / clz), reduced over the wave by shuffles and joined by integer atomicMin /
//                              atomicMax into four extents per instance, relative to the frame.
//   tight_size_kernel          one lane per instance: the tight bounds from the extents ((0, 0, -1, -1) when no word was non-zero) and
//                              the words of its rows; scan_launch (scan.h, two launches) turns the counts into the offsets.
//   the family's fill pass     computes the words again at the TIGHT position (the grid is sized for the loose frame; the units of
//                              work past the tight one leave) and stores each once; tight_count sums the popcounts over the wave
//                              and adds them to the instance's area by one integer atomic.
// The tight bounds and the areas come back first, the host derives the offsets from the bounds exactly as the scan did, and copies
// exactly the bytes of the result.  The only atomics are integer min, max and add: the same input gives the same bytes on every
// run.  A family supplies the function that forms a word (one __device__ function both of its passes call), the two thin kernels
// round it, and a call object (below); the unit of work -- a lane per word, a wave per block of 64 x 64 -- is the family's own.
#pragma once
#include <algorithm>
#include <climits>
#include <vector>

#include "mask_set.h"
#include "scan.h"

namespace mnc {

constexpr int kTightThreads = 256;
constexpr int kTightMaxN = 2048;                  // instances of a set and of a result (mnc_mask_boundary's limit)
constexpr int kTightMaxCoord = 1 << 24;
constexpr long long kTightMaxPixels = 1ll << 27;  // pixels of the loose frames of one call

// The loose frame of one output instance; fw or fh 0: no pixel, skipped by every kernel.
struct TightFrame {
  int fx, fy, fw, fh;
};

// Extents relative to the frame (the extent pass; x2 < 0: no pixel), then the tight bounds in image coordinates (tight_size_kernel).
struct TightBox {
  int x1, y1, x2, y2;
};

// Every lane of a wave comes here with a result word of its instance (0: none), the frame-relative column of the word's bit 0 and
// its frame-relative row: the wave's extents joined into *ext.
__device__ __forceinline__ void tight_join(TightBox* __restrict__ ext, u64 v, int col, int row) {
  int minx = INT_MAX, miny = INT_MAX, maxx = -1, maxy = -1;
  if (v) {
    minx = col + (__ffsll((long long)v) - 1);
    maxx = col + 63 - __clzll((long long)v);
    miny = maxy = row;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    minx = min(minx, __shfl_xor(minx, s));
    miny = min(miny, __shfl_xor(miny, s));
    maxx = max(maxx, __shfl_xor(maxx, s));
    maxy = max(maxy, __shfl_xor(maxy, s));
  }
  if ((threadIdx.x & 63) == 0 && maxx >= 0) {
    atomicMin(&ext->x1, minx);
    atomicMin(&ext->y1, miny);
    atomicMax(&ext->x2, maxx);
    atomicMax(&ext->y2, maxy);
  }
}

// Every lane of a wave comes here with the word it stored (0: none): their set bits added to *area.
__device__ __forceinline__ void tight_count(u64* __restrict__ area, u64 v) {
  int set = __popcll(v);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) set += __shfl_xor(set, s);
  if ((threadIdx.x & 63) == 0 && set) atomicAdd(area, (u64)set);
}

// mask_tight.hip.  The launch of tight_size_kernel over n frames `stride` TightFrames apart (a family's jobs begin with their
// frame): box [n] in place from extents into tight bounds, words [n] the words of their rows.
void tight_size_launch(hipStream_t s, const TightFrame* d_frames, int stride, int n, TightBox* d_box, int* d_words);
// MNC_ERR_INVALID: a window (x1, y1, x2, y2) with a coordinate outside +-2^24, or empty.
int tight_check_window(const char* who, const int* window);

// The host side of one call: the jobs of its output instances -- a Job is a TightFrame or derives from one -- and what the launches
// need to know of the frames.  A family derives its call from this and adds
//   void take(WsLayout&)                        the workspace of its sets and operands
//   hipError_t upload(const HostScope&) const   their copies
//   void extent(hipStream_t, const Job* d_jobs, TightBox* d_ext) const
//   void fill(hipStream_t, const Job* d_jobs, const TightBox* d_box, Scanned first, u64* d_out, u64* d_area) const
// the last two one launch each.
template <class Job>
struct TightCall {
  std::vector<Job> jobs;
  const int* window = nullptr;                    // set: every frame is intersected with it
  long long pixels = 0, bound_words = 0;          // of the frames
  long long most_words = 0, most_blocks = 0;      // of one frame: words, and blocks of 64 rows x 64 columns
  // The job of the next output instance: its frame (x1, y1, x2, y2), inclusive; x2 < x1 or y2 < y1: none.
  void add(int x1, int y1, int x2, int y2, Job j = Job()) {
    if (window) {
      x1 = std::max(x1, window[0]); y1 = std::max(y1, window[1]);
      x2 = std::min(x2, window[2]); y2 = std::min(y2, window[3]);
    }
    TightFrame& f = j;
    f = TightFrame{0, 0, 0, 0};
    if (x2 >= x1 && y2 >= y1) {
      f = TightFrame{x1, y1, x2 - x1 + 1, y2 - y1 + 1};
      const long long w = (long long)f.fh * mask_strips(f.fw);
      pixels += (long long)f.fw * f.fh;
      bound_words += w;
      most_words = std::max(most_words, w);
      most_blocks = std::max(most_blocks, (long long)((f.fh + 63) >> 6) * mask_strips(f.fw));
    }
    jobs.push_back(j);
  }
  void add_empty() { add(0, 0, -1, -1); }
};

// The rest of every entry once its jobs are made: the protocol of the sizes, the answers of the host, the launches, the copies.
template <class Call>
int tight_run(const char* who, Call& c, CallTimer& timer, int* out_bounds, long long* out_offsets, long long* out_areas,
              void* out_bits, size_t bits_cap, size_t* bits_bound, size_t* bits_bytes, int device_id) {
  typedef typename decltype(c.jobs)::value_type Job;
  static_assert(sizeof(Job) % sizeof(TightFrame) == 0, "tight_size_kernel steps over the jobs in whole frames");
  const int n = (int)c.jobs.size();
  MNC_REQUIRE(c.pixels <= kTightMaxPixels, "%s: %lld pixels of loose-frame rows in the call (limit %lld)", who, c.pixels,
              kTightMaxPixels);
  MNC_REQUIRE(!out_bits || bits_bytes, "%s: null bits_bytes", who);
  MNC_REQUIRE(!out_bits || n == 0 || (out_bounds && out_offsets && out_areas), "%s: null output pointer", who);
  const size_t bound = (size_t)c.bound_words * 8;
  *bits_bound = bound;
  if (!out_bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(bits_cap >= bound, "%s: bits_cap %zu is below the %zu bytes of the loose frames", who, bits_cap, bound);
  for (int o = 0; o < n; ++o) {
    int* q = out_bounds + 4 * (size_t)o;
    q[0] = 0; q[1] = 0; q[2] = -1; q[3] = -1;
    out_offsets[o] = 0;
    out_areas[o] = 0;
  }
  *bits_bytes = 0;
  if (bound == 0) { clear_error(); return MNC_OK; }        // no frame has a row
  Job* d_jobs; int *d_words, *d_tile; TightBox* d_box; u64 *d_out, *d_area;
  auto layout = [&](WsLayout l) {
    c.take(l);
    d_jobs = l.take<Job>(n);
    d_box = l.take<TightBox>(n);
    d_words = l.take<int>(n);
    d_tile = l.take<int>((size_t)scan_tiles(n) + 1);
    d_out = l.take<u64>((size_t)c.bound_words);
    d_area = l.take<u64>(n);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  std::vector<TightBox> box((size_t)n, TightBox{INT_MAX, INT_MAX, -1, -1});
  std::vector<u64> area((size_t)n, 0ull);
  MNC_HIP_TRY(c.upload(hs));
  MNC_HIP_TRY(hs.up(d_jobs, c.jobs.data(), (size_t)n * sizeof(Job)));
  MNC_HIP_TRY(hs.up(d_box, box.data(), (size_t)n * sizeof(TightBox)));
  MNC_HIP_TRY(hs.up(d_area, area.data(), (size_t)n * sizeof(u64)));
  TimedSpan span(timer);
  span.begin(hs.stream);
  c.extent(hs.stream, d_jobs, d_box);
  tight_size_launch(hs.stream, d_jobs, (int)(sizeof(Job) / sizeof(TightFrame)), n, d_box, d_words);
  const Scanned first = scan_launch(hs.stream, d_words, n, d_tile);
  c.fill(hs.stream, d_jobs, d_box, first, d_out, d_area);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(box.data(), d_box, (size_t)n * sizeof(TightBox)));
  MNC_HIP_TRY(hs.down(area.data(), d_area, (size_t)n * sizeof(u64)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  long long at = 0;                                        // the offsets as the scan placed them: the bytes of the tight rows
  for (int o = 0; o < n; ++o) at += mask_bytes(box[o].x2 - box[o].x1 + 1, box[o].y2 - box[o].y1 + 1);
  if (at < 0 || (size_t)at > bound) {                      // (cannot be: a tight frame lies inside its loose one)
    set_error("%s: the result's %lld bytes exceed the bound %zu", who, at, bound);
    return MNC_ERR_HIP;
  }
  MNC_HIP_TRY(hs.down(out_bits, d_out, (size_t)at));
  MNC_HIP_TRY(hs.sync());
  at = 0;
  for (int o = 0; o < n; ++o) {
    int* q = out_bounds + 4 * (size_t)o;
    q[0] = box[o].x1; q[1] = box[o].y1; q[2] = box[o].x2; q[3] = box[o].y2;
    out_offsets[o] = at;
    out_areas[o] = (long long)area[o];
    at += mask_bytes(box[o].x2 - box[o].x1 + 1, box[o].y2 - box[o].y1 + 1);
  }
  *bits_bytes = (size_t)at;
  clear_error();
  return MNC_OK;
}

}  // namespace mnc
