// The squared Euclidean distance transform of packed instance masks and the morphology by a disc that follows from it
// (include/mnc_hip.h n15), for gfx950, on the PackedMasks layout of inst_masks.hip (n5), without unpacking a mask.  The statements
// of the rules are mnc_amd/distance.py:distance_numpy, inscribed_numpy and morph_numpy; this file computes the same numbers and
// words bit for bit.  All arithmetic is integer.
//
// Everything is one transform, run in two passes over a FRAME of fw x fh pixels in which a source mask of sw x sh pixels stands
// at (px, py).  T is the set whose inside distance is wanted:
//   erode kind    T = the source.  Pixels beyond the frame are not in T (bit -1, bit fw, row -1 and row fh count as unset).
//   dilate kind   T = the complement of the source.  Pixels beyond the frame are in T: nothing of the source lies there.
// D(p) = min over the pixels q not in T of |p - q|^2; erode keeps p iff D(p) > R2, dilate sets p iff D(p) <= R2.
//
//   md_gap_kernel     one lane per pixel of the frame, a wave per 64-bit word of a row (the word is one broadcast read): g, the
//                     distance along the row to the nearest pixel not in T, from the zeros of the lane's own word below and above
//                     its bit (__clzll / __ffsll) and, while none is found, of the neighbouring words one after the other (source
//                     words are funnel-shifted to the frame by mask_word_at, padding bits masked before use), cut off at `cap`.
//                     Stored as uint16, row stride fw: the second pass reads it coalesced.
//   md_final_kernel   one lane per pixel of the OUTPUT WINDOW of the frame (ow x oh at (wx, wy)), 64 lanes along x, a wave taking
//                     md_span(kOut) consecutive words of the window one after the other.  best =
//                     min(g^2, and for the erode kind (y + 1)^2, (fh - y)^2), then the rows y - dy and y + dy while dy^2 < best.
//                     <kBits>: dy stops at rho = isqrt(R2) and as soon as best <= R2 -- a candidate further away is > R2 and the
//                     decision is made; the wave's 64 decisions are one ballot, stored as one word (lanes beyond ow vote 0:
//                     padding bits are 0), the popcounts of the wave's words added to the instance's area by one integer
//                     atomic.  <kDist>: D as uint32.  <kKey>: the 64-bit maximum of (D << 32) | (0xffffffff - linear index) over
//                     the wave's words and lanes (shuffles), then one atomic max per wave: the largest D, at the lowest (y, x).
// `cap` makes a capped g harmless to every reader.  Morphology: cap = rho + 1, whose square is > R2.  Distance maps: cap =
// (min(w, h) + 1) / 2 + 1, above the root of any D of the instance -- NOT the row's own min(y + 1, fh - y), which other rows read
// and which can undercut their true distance.
//
//   erode    one erode stage on the bounds.
//   dilate   one dilate stage on the frame grown by rho on every side; the window is the grown frame or its part in the image.
//   open     erode on the bounds into a temporary set, then dilate of that on the bounds (an opening never leaves the mask).
//   close    dilate into the grown frame (temporary), then erode of that in the grown frame -- unclipped, so that an object at
//            the image's edge is not eaten -- with the bounds as window (a closing by a disc never leaves a rectangle).
// Two launches per stage, so 2 or 4 per call whatever the data; the stages of open and close follow each other on the stream
// without a host round trip.  Every output word and every distance is written exactly once by vector stores; the only atomics are
// integer adds and maxima: the same bytes from run to run.  The instance tables of the stages are made on the host (MdStage).
//
// Bound: latency and L2.  The g plane is two bytes a pixel, written once and read 2 rho + 1 times at most per window pixel by
// coalesced 128-byte wave reads from L2 (a frame of an image's instance is a few tens of KB); the deep search of a distance map
// costs a pixel as many row pairs as its distance.  Measured at 100 instances of a 600 x 1000 image (1.05 x 10^6 pixels of rows),
// kernels alone: the maps 37 us of a 0.38 ms call that is mostly the 4 MB of distances coming back; inscribed 45 us of 0.11 ms;
// open + close at R = 2 125 us (8 launches) of 0.39 ms; dilate at R = 23 106 us of 0.24 ms (profiles/mask_distance_bench.txt).
#include <vector>

#include "mask_set.h"

namespace mnc {

constexpr int kMdThreads = 256;
constexpr int kMdWaves = kMdThreads / 64;
constexpr int kMdMaxN = 2048;                  // instances of one call (mnc_mask_boundary's limit)
constexpr int kMdMaxSide = 32768;              // H, W limit
constexpr int kMdMaxR2 = 1024 * 1024;
constexpr int kMdMaxCoord = 1 << 24;
constexpr long long kMdMaxArea = 1ll << 26;    // pixels of one (grown) instance
constexpr long long kMdMaxPixels = 1ll << 27;  // pixels of the frames of one call

enum MdKind { kMdErode = 0, kMdDilate = 1 };
enum MdOut { kBits = 0, kDist = 1, kKey = 2 };
// Consecutive words of a window that one wave of the second pass takes, one after the other, before its one atomic: the atomics of
// an instance all meet at one address, where 16 000 of them (an image's 100 instances, a word each) cost more than the shallow
// search of a morphology at R = 2 does.  The maps have no atomic and a deep search, whose latency only more waves hide: a word a
// wave.  (Measured on the 100 instances of a 600 x 1000 image, kernels alone: open + close 285 us a word a wave, 126 us at 8;
// the maps 37 us a word a wave, 58 us at 8.)
__host__ __device__ constexpr int md_span(int out) { return out == kBits ? 8 : out == kKey ? 4 : 1; }

// One instance of one stage.  A frame or a window without pixels (fh == 0 resp. oh == 0) is skipped by both kernels.
struct MdInst {
  long long src_words;        // first word of the source rows
  long long g_off;            // first entry of the frame in the g plane
  long long out_off;          // first word of the window in the output bits / first entry in the distances
  int sw, sh;                 // source
  int fw, fh;                 // frame
  int px, py;                 // the source's place in the frame
  int wx, wy, ow, oh;         // window of the frame that is written
  int cap;
  int pad_;
};

// Word j (any int) of row y of T in the frame: the columns 64 j .. 64 j + 63.
__device__ __forceinline__ u64 md_t_word(const u64* __restrict__ src, const MdInst& a, int sstrips, int y, int j, int dilate) {
  const int sy = y - a.py;
  u64 s = 0ull;
  if (sy >= 0 && sy < a.sh) s = mask_word_at(src + a.src_words + (long long)sy * sstrips, j * 64 - a.px, sstrips, a.sw);
  return dilate ? ~s : s;
}

// grid (ceil(most frame words / 4), n), block 256: a wave per word of the frame.
__global__ __launch_bounds__(kMdThreads) void md_gap_kernel(const MdInst* __restrict__ insts, const u64* __restrict__ src, int dilate,
                                                            unsigned short* __restrict__ g) {
  const MdInst a = insts[blockIdx.y];
  if (a.fh < 1 || a.fw < 1) return;
  const int strips = mask_strips(a.fw), sstrips = mask_strips(a.sw);
  const long long word = (long long)blockIdx.x * kMdWaves + (threadIdx.x >> 6);
  if (word >= (long long)a.fh * strips) return;
  const int y = (int)(word / strips), j = (int)(word - (long long)y * strips), b = threadIdx.x & 63;
  const int cap = a.cap;
  int dist = cap;
  // the pixels not in T as ones
  const u64 z0 = ~md_t_word(src, a, sstrips, y, j, dilate);
  // at or below this bit: the highest one of word j - k stands 64 k + b - hi columns before
  u64 z = z0 & ((2ull << b) - 1ull);
  for (int k = 0;;) {
    if (z) {
      dist = min(dist, 64 * k + b - (63 - __clzll((long long)z)));
      break;
    }
    ++k;
    if (64 * k + b - 63 >= cap) break;
    z = ~md_t_word(src, a, sstrips, y, j - k, dilate);
  }
  // at or above it: the lowest one of word j + k stands 64 k + lo - b columns after
  z = z0 & (~0ull << b);
  for (int k = 0;;) {
    if (z) {
      dist = min(dist, 64 * k + (__ffsll((long long)z) - 1) - b);
      break;
    }
    ++k;
    if (64 * k - b >= cap) break;
    z = ~md_t_word(src, a, sstrips, y, j + k, dilate);
  }
  const int x = j * 64 + b;
  if (x < a.fw) g[a.g_off + (long long)y * a.fw + x] = (unsigned short)dist;
}

// grid (ceil(most window words / (4 md_span)), n), block 256: a wave per md_span(kOut) consecutive words of the window.
template <int kOut>
__global__ __launch_bounds__(kMdThreads) void md_final_kernel(const MdInst* __restrict__ insts, const unsigned short* __restrict__ g,
                                                              int dilate, unsigned r2, int rho, u64* __restrict__ bits,
                                                              u64* __restrict__ area, unsigned* __restrict__ dist, u64* __restrict__ key) {
  const int i = blockIdx.y;
  const MdInst a = insts[i];
  if (a.oh < 1 || a.ow < 1) return;
  const int ostrips = mask_strips(a.ow);
  const long long words = (long long)a.oh * ostrips;
  constexpr int kSpan = md_span(kOut);
  const long long first = ((long long)blockIdx.x * kMdWaves + (threadIdx.x >> 6)) * kSpan;
  if (first >= words) return;                          // (the whole wave)
  const long long end = first + kSpan < words ? first + kSpan : words;
  const int reach = kOut == kBits ? rho : 65535;
  u64 set = 0ull, top = 0ull;                          // the bits this wave set (every lane alike) / this lane's largest key
  for (long long word = first; word < end; ++word) {
    const int yo = (int)(word / ostrips), xo = (int)(word - (long long)yo * ostrips) * 64 + (threadIdx.x & 63);
    const bool live = xo < a.ow;
    unsigned best = 0u;
    if (live) {
      const int y = a.wy + yo;
      const unsigned short* col = g + a.g_off + a.wx + xo;
      const unsigned v = col[(long long)y * a.fw];
      best = v * v;
      if (!dilate) {
        const unsigned edge = (unsigned)min(min(y + 1, a.fh - y), 65535);
        best = min(best, edge * edge);
      }
      // (g <= cap <= 4098, as an instance has at most 2^26 pixels and rho <= 1024: g^2 + dy^2 with dy^2 < best stays far below 2^32)
      for (int dy = 1; dy <= reach && (unsigned)dy * (unsigned)dy < best && (kOut != kBits || best > r2); ++dy) {
        const unsigned dd = (unsigned)dy * (unsigned)dy;
        if (y - dy >= 0) {
          const unsigned u = col[(long long)(y - dy) * a.fw];
          best = min(best, u * u + dd);
        }
        if (y + dy < a.fh) {
          const unsigned u = col[(long long)(y + dy) * a.fw];
          best = min(best, u * u + dd);
        }
      }
    }
    if (kOut == kBits) {
      const u64 w = __ballot(live && (dilate ? best <= r2 : best > r2));
      if ((threadIdx.x & 63) == 0) bits[a.out_off + word] = w;
      set += (u64)__popcll(w);
    } else if (kOut == kDist) {
      if (live) dist[a.out_off + (long long)yo * a.ow + xo] = best;
    } else if (live) {
      const u64 k = ((u64)best << 32) | (u64)(0xffffffffu - (unsigned)(yo * a.ow + xo));
      top = k > top ? k : top;
    }
  }
  if (kOut == kBits) {
    if ((threadIdx.x & 63) == 0 && set) atomicAdd(&area[i], set);
  } else if (kOut == kKey) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const u64 o = __shfl_xor(top, s);
      top = o > top ? o : top;
    }
    if ((threadIdx.x & 63) == 0 && (top >> 32)) atomicMax(&key[i], top);
  }
}

namespace {

// The instance table of one stage and what its two launches need.
struct MdStage {
  std::vector<MdInst> inst;
  int kind = kMdErode;
  long long g_entries = 0;      // of the frames
  long long most_frame = 0;     // words of the largest frame
  long long most_window = 0;    // words of the largest window
  void add(const MdInst& in) {
    MdInst a = in;
    if (a.fw < 1 || a.fh < 1 || a.ow < 1 || a.oh < 1) a.fw = a.fh = a.ow = a.oh = 0;
    a.g_off = g_entries;
    g_entries += (long long)a.fw * a.fh;
    const long long f = (long long)a.fh * mask_strips(a.fw), w = (long long)a.oh * mask_strips(a.ow);
    if (f > most_frame) most_frame = f;
    if (w > most_window) most_window = w;
    inst.push_back(a);
  }
};

int md_isqrt(int v) {
  int r = 0;
  while ((long long)(r + 1) * (r + 1) <= v) ++r;
  return r;
}


// A whole frame as window: the erode stage of a mask on its bounds, for the maps (cap as the head says) or at a disc.
MdInst md_on_bounds(const mnc_mask_info& a, long long src_words, int cap, long long out_off) {
  MdInst m = MdInst();
  if (!mask_has_rows(a)) return m;
  m.src_words = src_words;
  m.sw = m.fw = m.ow = a.x2 - a.x1 + 1;
  m.sh = m.fh = m.oh = a.y2 - a.y1 + 1;
  m.cap = cap;
  m.out_off = out_off;
  return m;
}

inline int md_map_cap(const mnc_mask_info& a) {
  const int w = a.x2 - a.x1 + 1, h = a.y2 - a.y1 + 1;
  return ((w < h ? w : h) + 1) / 2 + 1;
}

void md_launch_gap(hipStream_t s, const MdStage& st, const MdInst* d_inst, const u64* d_src, unsigned short* d_g) {
  if (st.most_frame < 1) return;
  hipLaunchKernelGGL(md_gap_kernel, dim3((unsigned)((st.most_frame + kMdWaves - 1) / kMdWaves), (unsigned)st.inst.size()),
                     dim3(kMdThreads), 0, s, d_inst, d_src, st.kind, d_g);
}

template <int kOut>
void md_launch_final(hipStream_t s, const MdStage& st, const MdInst* d_inst, const unsigned short* d_g, int r2, int rho, u64* d_bits,
                     u64* d_area, unsigned* d_dist, u64* d_key) {
  if (st.most_window < 1) return;
  const long long per_block = kMdWaves * md_span(kOut);
  hipLaunchKernelGGL(md_final_kernel<kOut>, dim3((unsigned)((st.most_window + per_block - 1) / per_block), (unsigned)st.inst.size()),
                     dim3(kMdThreads), 0, s, d_inst, d_g, st.kind, (unsigned)r2, rho, d_bits, d_area, d_dist, d_key);
}

// What every entry refuses about its set beyond HostMaskSet::check, and the pixels of the rows.
int md_check_set(const char* who, HostMaskSet* set, const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n,
                 long long* pixels) {
  MNC_REQUIRE(n >= 0 && n <= kMdMaxN, "%s: n=%d not in [0, %d]", who, n, kMdMaxN);
  const int rc = set->check(who, "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
  if (rc) return rc;
  *pixels = 0;
  for (const mnc_mask_info& a : set->info)
    if (mask_has_rows(a)) *pixels += (long long)(a.x2 - a.x1 + 1) * (a.y2 - a.y1 + 1);
  MNC_REQUIRE(*pixels <= kMdMaxPixels, "%s: %lld pixels of rows in the call (limit %lld)", who, *pixels, kMdMaxPixels);
  return MNC_OK;
}

CallTimer g_md_timer;

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_distance(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, long long* dist_ptr,
                      unsigned* dist, size_t dist_cap, size_t* dist_total, int device_id) {
  const char* who = "mnc_mask_distance";
  MNC_REQUIRE(dist_ptr && dist_total, "%s: null dist_ptr or dist_total", who);
  HostMaskSet set;
  long long pixels = 0;
  int rc = md_check_set(who, &set, bounds, offsets, bits, bytes, n, &pixels);
  if (rc) return rc;
  MdStage st;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = set.info[i];
    dist_ptr[i] = st.g_entries;                            // (a frame is the bounds: the maps are numbered as the g plane is)
    st.add(md_on_bounds(a, a.offset / 8, mask_has_rows(a) ? md_map_cap(a) : 0, st.g_entries));
  }
  dist_ptr[n] = st.g_entries;
  *dist_total = (size_t)pixels;
  if (!dist || pixels == 0) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(dist_cap >= (size_t)pixels, "%s: dist_cap %zu is below the %lld distances of the maps", who, dist_cap, pixels);
  MdInst* d_inst; unsigned short* d_g; unsigned* d_dist;
  auto layout = [&](WsLayout l) {
    set.take(l);
    d_inst = l.take<MdInst>(n);
    d_g = l.take<unsigned short>((size_t)pixels);
    d_dist = l.take<unsigned>((size_t)pixels);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(set.upload(hs));
  MNC_HIP_TRY(hs.up(d_inst, st.inst.data(), (size_t)n * sizeof(MdInst)));
  TimedSpan span(g_md_timer);
  span.begin(hs.stream);
  md_launch_gap(hs.stream, st, d_inst, set.d_bits, d_g);
  md_launch_final<kDist>(hs.stream, st, d_inst, d_g, 0, 0, nullptr, nullptr, d_dist, nullptr);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(dist, d_dist, (size_t)pixels * sizeof(unsigned)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_inscribed(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int* xy, int* r2,
                       int device_id) {
  const char* who = "mnc_mask_inscribed";
  MNC_REQUIRE(n <= 0 || (xy && r2), "%s: null output pointer", who);
  HostMaskSet set;
  long long pixels = 0;
  int rc = md_check_set(who, &set, bounds, offsets, bits, bytes, n, &pixels);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) { xy[2 * (size_t)i] = -1; xy[2 * (size_t)i + 1] = -1; r2[i] = 0; }
  if (pixels == 0) { clear_error(); return MNC_OK; }
  MdStage st;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = set.info[i];
    st.add(md_on_bounds(a, a.offset / 8, mask_has_rows(a) ? md_map_cap(a) : 0, 0));
  }
  MdInst* d_inst; unsigned short* d_g; u64* d_key;
  auto layout = [&](WsLayout l) {
    set.take(l);
    d_inst = l.take<MdInst>(n);
    d_g = l.take<unsigned short>((size_t)pixels);
    d_key = l.take<u64>(n);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  std::vector<u64> key((size_t)n, 0ull);
  MNC_HIP_TRY(set.upload(hs));
  MNC_HIP_TRY(hs.up(d_inst, st.inst.data(), (size_t)n * sizeof(MdInst)));
  MNC_HIP_TRY(hs.up(d_key, key.data(), (size_t)n * sizeof(u64)));
  TimedSpan span(g_md_timer);
  span.begin(hs.stream);
  md_launch_gap(hs.stream, st, d_inst, set.d_bits, d_g);
  md_launch_final<kKey>(hs.stream, st, d_inst, d_g, 0, 0, nullptr, nullptr, nullptr, d_key);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(key.data(), d_key, (size_t)n * sizeof(u64)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  for (int i = 0; i < n; ++i) {
    if (!(key[i] >> 32)) continue;                         // no set pixel: the largest D is 0
    const mnc_mask_info& a = set.info[i];
    const unsigned at = 0xffffffffu - (unsigned)(key[i] & 0xffffffffull);
    const int w = a.x2 - a.x1 + 1;
    xy[2 * (size_t)i] = a.x1 + (int)(at % (unsigned)w);
    xy[2 * (size_t)i + 1] = a.y1 + (int)(at / (unsigned)w);
    r2[i] = (int)(key[i] >> 32);
  }
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_morph(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int op, int r2, int H, int W,
                   int* out_bounds, long long* out_offsets, long long* out_areas, void* out_bits, size_t bits_cap, size_t* bits_bytes,
                   int device_id) {
  const char* who = "mnc_mask_morph";
  MNC_REQUIRE(op >= 0 && op <= 3, "%s: op=%d is not 0 (erode), 1 (dilate), 2 (open) or 3 (close)", who, op);
  MNC_REQUIRE(r2 >= 0 && r2 <= kMdMaxR2, "%s: r2=%d not in [0, %d]", who, r2, kMdMaxR2);
  MNC_REQUIRE((H == 0 && W == 0) || (H >= 1 && W >= 1 && H <= kMdMaxSide && W <= kMdMaxSide),
              "%s: image %d x %d is neither 0 x 0 (no clip) nor in [1, %d]", who, H, W, kMdMaxSide);
  MNC_REQUIRE(bits_bytes, "%s: null bits_bytes", who);
  MNC_REQUIRE(n <= 0 || (out_bounds && out_offsets), "%s: null output pointer", who);
  MNC_REQUIRE(n <= 0 || !out_bits || out_areas, "%s: null out_areas", who);
  HostMaskSet set;
  long long pixels = 0;
  int rc = md_check_set(who, &set, bounds, offsets, bits, bytes, n, &pixels);
  if (rc) return rc;
  const int rho = md_isqrt(r2), cap = rho + 1;
  const bool grown = op == 1 || op == 3, clip = op == 1 && H > 0;
  if (grown) {                                             // the frames are the bounds grown by rho
    pixels = 0;
    for (int i = 0; i < n; ++i) {
      const mnc_mask_info& a = set.info[i];
      if (!mask_has_rows(a)) continue;
      MNC_REQUIRE(a.x1 - rho > -kMdMaxCoord && a.y1 - rho > -kMdMaxCoord && a.x2 + rho < kMdMaxCoord && a.y2 + rho < kMdMaxCoord,
                  "%s: masks[%d] grown by %d leaves the coordinate range", who, i, rho);
      const long long p = (long long)(a.x2 - a.x1 + 1 + 2 * rho) * (a.y2 - a.y1 + 1 + 2 * rho);
      MNC_REQUIRE(p <= kMdMaxArea, "%s: masks[%d] grown by %d covers %lld pixels (limit %lld)", who, i, rho, p, kMdMaxArea);
      pixels += p;
    }
    MNC_REQUIRE(pixels <= kMdMaxPixels, "%s: %lld pixels of grown rows in the call (limit %lld)", who, pixels, kMdMaxPixels);
  }
  // the result's table, and the stages: first reads the set, second (open, close) reads the temporary set the first wrote
  MdStage first, second;
  std::vector<int> ob((size_t)n * 4);
  std::vector<long long> oo((size_t)n);
  long long out_words = 0, tmp_words = 0;
  first.kind = op == 0 || op == 2 ? kMdErode : kMdDilate;
  second.kind = op == 2 ? kMdDilate : kMdErode;
  for (int i = 0; i < n; ++i) {
    const mnc_mask_info& a = set.info[i];
    int* q = &ob[4 * (size_t)i];
    q[0] = a.x1; q[1] = a.y1; q[2] = a.x2; q[3] = a.y2;
    oo[i] = out_words * 8;
    if (!mask_has_rows(a)) {
      if (clip) { q[0] = 0; q[1] = 0; q[2] = -1; q[3] = -1; }
      first.add(MdInst());
      if (op >= 2) second.add(MdInst());
      continue;
    }
    const int w = a.x2 - a.x1 + 1, h = a.y2 - a.y1 + 1;
    MdInst on = md_on_bounds(a, a.offset / 8, cap, out_words), g = on;    // g: the grown frame with the set's rows at (rho, rho)
    g.fw = g.ow = w + 2 * rho;
    g.fh = g.oh = h + 2 * rho;
    g.px = g.py = rho;
    if (op == 0) {
      first.add(on);
      out_words += (long long)h * mask_strips(w);
    } else if (op == 1) {
      int x1 = a.x1 - rho, y1 = a.y1 - rho, x2 = a.x2 + rho, y2 = a.y2 + rho;
      if (clip) {
        x1 = x1 > 0 ? x1 : 0; y1 = y1 > 0 ? y1 : 0;
        x2 = x2 < W - 1 ? x2 : W - 1; y2 = y2 < H - 1 ? y2 : H - 1;
      }
      if (x2 < x1 || y2 < y1) {                            // wholly outside the image
        q[0] = 0; q[1] = 0; q[2] = -1; q[3] = -1;
        first.add(MdInst());
        continue;
      }
      q[0] = x1; q[1] = y1; q[2] = x2; q[3] = y2;
      g.wx = x1 - (a.x1 - rho); g.wy = y1 - (a.y1 - rho);
      g.ow = x2 - x1 + 1; g.oh = y2 - y1 + 1;
      first.add(g);
      out_words += (long long)g.oh * mask_strips(g.ow);
    } else if (op == 2) {
      on.out_off = tmp_words;
      first.add(on);
      MdInst d = md_on_bounds(a, tmp_words, cap, out_words);
      second.add(d);
      tmp_words += (long long)h * mask_strips(w);
      out_words += (long long)h * mask_strips(w);
    } else {
      g.out_off = tmp_words;
      first.add(g);
      MdInst e = MdInst();
      e.src_words = tmp_words;
      e.sw = e.fw = g.fw; e.sh = e.fh = g.fh;
      e.wx = e.wy = rho; e.ow = w; e.oh = h;
      e.cap = cap;
      e.out_off = out_words;
      second.add(e);
      tmp_words += (long long)g.fh * mask_strips(g.fw);
      out_words += (long long)h * mask_strips(w);
    }
  }
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 4; ++k) out_bounds[4 * (size_t)i + k] = ob[4 * (size_t)i + k];
    out_offsets[i] = oo[i];
  }
  const size_t need = (size_t)out_words * 8;
  *bits_bytes = need;
  if (!out_bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(bits_cap >= need, "%s: bits_cap %zu is below the %zu bytes of the result", who, bits_cap, need);
  for (int i = 0; i < n; ++i) out_areas[i] = 0;
  if (need == 0) { clear_error(); return MNC_OK; }         // no instance has a row (in the image)
  const bool two = op >= 2;
  const long long g_entries = first.g_entries > second.g_entries ? first.g_entries : second.g_entries;
  MdInst *d_first, *d_second; unsigned short* d_g; u64 *d_tmp, *d_obits, *d_area;
  auto layout = [&](WsLayout l) {
    set.take(l);
    d_first = l.take<MdInst>(n);
    d_second = l.take<MdInst>(two ? n : 0);
    d_g = l.take<unsigned short>((size_t)g_entries);
    d_tmp = l.take<u64>((size_t)tmp_words);
    d_obits = l.take<u64>((size_t)out_words);
    d_area = l.take<u64>(2 * (size_t)n);                   // of the result, then (open, close) of the temporary set: not read
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  std::vector<u64> area(2 * (size_t)n, 0ull);
  MNC_HIP_TRY(set.upload(hs));
  MNC_HIP_TRY(hs.up(d_first, first.inst.data(), (size_t)n * sizeof(MdInst)));
  if (two) MNC_HIP_TRY(hs.up(d_second, second.inst.data(), (size_t)n * sizeof(MdInst)));
  MNC_HIP_TRY(hs.up(d_area, area.data(), area.size() * sizeof(u64)));
  TimedSpan span(g_md_timer);
  span.begin(hs.stream);
  md_launch_gap(hs.stream, first, d_first, set.d_bits, d_g);
  md_launch_final<kBits>(hs.stream, first, d_first, d_g, r2, rho, two ? d_tmp : d_obits, two ? d_area + n : d_area, nullptr, nullptr);
  if (two) {
    md_launch_gap(hs.stream, second, d_second, d_tmp, d_g);
    md_launch_final<kBits>(hs.stream, second, d_second, d_g, r2, rho, d_obits, d_area, nullptr, nullptr);
  }
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(area.data(), d_area, (size_t)n * sizeof(u64)));
  MNC_HIP_TRY(hs.down(out_bits, d_obits, need));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  for (int i = 0; i < n; ++i) out_areas[i] = (long long)area[i];
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_distance_timing(int on, double* last_ms) { return g_md_timer.set(on, last_ms); }
