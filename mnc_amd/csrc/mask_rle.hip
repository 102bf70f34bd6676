// COCO run-length encoding of packed instance masks, and the way back, for gfx950 (include/mnc_hip.h n7) -- the rule of the
// published maskApi.c (rleEncode / rleDecode / rleToBbox) on the PackedMasks layout of inst_masks.hip (n5), without unpacking a mask.
// An H x W image is read column by column, pixel (x, y) stands at position p = x * H + y; counts = the lengths of the runs of 0 and
// of 1 in turn, beginning with a run of 0.  With t_0 < t_1 < ... the positions whose pixel differs from the one before (the pixel
// before position 0 is 0): counts = diff([0, t_0, ..., t_{T-1}, H * W]).  Integer counts only: nothing depends on order, every
// output slot comes from a scan.
//
// Encode (the input is row-major words, the output is ordered by column):
//   rle_columns_kernel<0>   one wave per (instance, 64-column strip) walks 64-row tiles down the strip.  Lane r holds the 64 bits of
//                           row r under the strip (funnel-shifted from two words, as mask_overlaps_kernel does; the padding and
//                           the columns outside the image cleared); 64 __ballots of bit k give column k's 64 rows as one uniform
//                           word c -- a 64 x 64 bit transpose without LDS.  Column k's transitions are T = c ^ ((c << 1) | carry),
//                           carry = the pixel above the tile: the last row of the tile before (lane 63's word), for the image's
//                           row 0 the pixel at the bottom of the column before.  An instance that ends above the image's bottom
//                           gets the row below its last one, and every instance the column right of its last one, so that the
//                           closing transition of a run of 1 is seen.  A mask that touches the bottom but not the top closes
//                           its run at row 0 of the next column, above its first row: that one transition is taken from the bottom
//                           pixel directly.  Lane k sums __popcll(T) of its column.
//   rle_scan_columns_kernel one wave per instance: the exclusive prefix of the column sums, in place, and the instance's sum.
//   rle_scan_runs_kernel    one wave: run_ptr = the exclusive prefix of (transitions + 1) over the instances, the head.
//   rle_columns_kernel<1>   the same walk once more: lane r stores transition r of column k at run_ptr[i] + prefix[k] + the
//                           transitions of T below bit r -- positions in order, guarded by the capacity.
//   rle_diff_kernel         one thread per run: the difference of two neighbouring positions (0 before the first, H * W after the
//                           last), as uint32.
// Decode:
//   rle_bounds_kernel       one workgroup per instance over its runs of 1 (the host made the start position of every run): min /
//                           max column and row (a run that crosses a column boundary spans rows 0 .. H-1) and the pixel sum --
//                           rleToBbox and the area.
//   rle_fill_kernel         the encoder's mirror: one wave per (instance, 64-column strip, 64-row tile), lane = column.  A lane
//                           bisects the start positions for the run that holds its column's first row, walks the runs down the
//                           64 rows into one column word, 64 __ballots turn the columns into row words and lane r stores row r's
//                           whole: every word of every row is written by exactly one lane, padding (0) included.
// Bound: the encoder reads every word of a mask twice per pass (16 bytes per 64 pixels and pass, from L2) and issues 64 ballots per
// 64 x 64 pixels.  Not measured yet (tools/mask_rle_bench.py, profiles/mask_rle_bench.txt).
#include <exception>
#include <vector>

#include "mask_set.h"
#include "scan.h"

namespace mnc {

constexpr int kRleThreads = 256;
constexpr int kRleWaves = kRleThreads / 64;
constexpr int kRleMaxN = 2048;                 // instances of one call
constexpr int kRleMaxSide = 32768;             // H, W limit: H * W <= 2^30, a position fits an unsigned

// An instance in an H x W image.
struct RleGeom {
  int x1, y1, w, sw;       // the bounds' corner, width, words per row
  int ax, ay, bx, by;      // the bounds clipped to the image
  int ncols, nrows;        // columns ax .. min(bx + 1, W - 1) and rows ay .. min(by + 1, H - 1): where a transition can stand
  const u64* rows;         // the first row's words
};

__host__ __device__ inline void rle_extent(int x1, int y1, int x2, int y2, int H, int W, int* ncols, int* nrows) {
  const int ax = max(x1, 0), ay = max(y1, 0), bx = min(x2, W - 1), by = min(y2, H - 1);
  const bool any = ax <= bx && ay <= by;
  *ncols = any ? min(bx + 1, W - 1) - ax + 1 : 0;
  *nrows = any ? min(by + 1, H - 1) - ay + 1 : 0;
}

__device__ __forceinline__ RleGeom rle_geom(const mnc_mask_info& m, const u64* bits, int H, int W) {
  RleGeom g;
  g.x1 = m.x1; g.y1 = m.y1;
  g.w = m.x2 - m.x1 + 1;
  g.sw = mask_strips(g.w);
  g.ax = max(m.x1, 0); g.ay = max(m.y1, 0); g.bx = min(m.x2, W - 1); g.by = min(m.y2, H - 1);
  rle_extent(m.x1, m.y1, m.x2, m.y2, H, W, &g.ncols, &g.nrows);
  g.rows = bits + m.offset / 8;
  return g;
}

// The 64 pixels (X0 .. X0 + 63, y) of the instance, ay <= y <= by and ax <= X0 <= bx + 1: bit k is column X0 + k; columns past bx read 0.
__device__ __forceinline__ u64 rle_row_bits(const RleGeom& g, int y, int X0) {
  u64 v = mask_word_at(g.rows + (long long)(y - g.y1) * g.sw, X0 - g.x1, g.sw, g.w);
  const int inside = g.bx - X0 + 1;
  if (inside < 64) v &= inside > 0 ? (1ull << inside) - 1ull : 0ull;
  return v;
}

__device__ __forceinline__ bool rle_pixel(const RleGeom& g, int x, int y) {
  if (x < g.ax || x > g.bx || y < g.ay || y > g.by) return false;
  const int dx = x - g.x1;
  return (g.rows[(long long)(y - g.y1) * g.sw + (dx >> 6)] >> (dx & 63)) & 1ull;
}

// grid (ceil(strips / 4), cap), block 256: wave = one (instance blockIdx.y, strip).  cols [cap][stride]: kEmit = 0 stores the
// transitions of every column of the strip there; kEmit = 1 reads their exclusive prefix from it and stores the positions of the
// transitions at pos[run_ptr[i] + ...], slots >= runs_cap dropped.
template <bool kEmit>
__global__ __launch_bounds__(kRleThreads) void rle_columns_kernel(MaskSet A, int cap, int H, int W, int stride, int* __restrict__ cols,
                                                                  const long long* __restrict__ run_ptr, unsigned* __restrict__ pos,
                                                                  long long runs_cap) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.y, strip = blockIdx.x * kRleWaves + wave;
  if (i >= mask_count(A, cap)) return;
  const RleGeom g = rle_geom(A.info[i], A.bits, H, W);
  if (strip * 64 >= g.ncols) return;                     // (uniform over the wave; an instance outside the image has no columns)
  const int X0 = g.ax + strip * 64;
  const int ncol = min(64, g.ncols - strip * 64);
  int* mine_at = cols + (long long)i * stride + strip * 64 + lane;
  // bit k: the pixel at the bottom of the column before column X0 + k
  const u64 bottom = __ballot(lane < ncol && g.by == H - 1 && rle_pixel(g, X0 + lane - 1, H - 1));
  // a mask that starts at row 0 joins it to its own first row; one that starts lower has a 0 there: a transition of its own
  u64 carry = g.ay == 0 ? bottom : 0ull;
  const u64 closing = g.ay == 0 ? 0ull : bottom;
  const long long first = kEmit ? run_ptr[i] : 0;
  int mine = kEmit && lane < ncol ? *mine_at : 0;        // count: the transitions of column `lane`; emit: its next slot
  if ((closing >> lane) & 1ull) {
    if (kEmit && first + mine < runs_cap) pos[first + mine] = (unsigned)(X0 + lane) * (unsigned)H;
    ++mine;
  }
  for (int r0 = 0; r0 < g.nrows; r0 += 64) {
    const int y = g.ay + r0 + lane;
    const u64 word = r0 + lane < g.nrows && y <= g.by ? rle_row_bits(g, y, X0) : 0ull;
    const int rows = min(64, g.nrows - r0);
    const u64 live = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const u64 c = __ballot((word >> k) & 1ull);
      const u64 t = (c ^ ((c << 1) | ((carry >> k) & 1ull))) & live;
      if (t == 0ull) continue;                           // (uniform)
      if (kEmit) {
        const long long slot = first + __shfl(mine, k) + __popcll(t & ((1ull << lane) - 1ull));
        if (((t >> lane) & 1ull) && slot < runs_cap) pos[slot] = (unsigned)(X0 + k) * (unsigned)H + (unsigned)y;
      }
      if (lane == k) mine += __popcll(t);
    }
    carry = __shfl(word, 63);                            // the tile's last row (a partial tile is the last one)
  }
  if (!kEmit && lane < ncol) *mine_at = mine;
}

// grid cap, block 64.  cols [cap][stride] -> the exclusive prefix over each instance's columns; sums [cap].
__global__ __launch_bounds__(64) void rle_scan_columns_kernel(MaskSet A, int cap, int H, int W, int stride, int* __restrict__ cols,
                                                              int* __restrict__ sums) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= mask_count(A, cap)) return;
  const mnc_mask_info m = A.info[i];
  int ncols, nrows;
  rle_extent(m.x1, m.y1, m.x2, m.y2, H, W, &ncols, &nrows);
  int* c = cols + (long long)i * stride;
  int base = 0;
  for (int k0 = 0; k0 < ncols; k0 += 64) {
    const int k = k0 + lane;
    const int v = k < ncols ? c[k] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (k < ncols) c[k] = base + incl - v;
    base += __shfl(incl, 63);
  }
  if (lane == 0) sums[i] = base;
}

// One mnc_mask_rle_dev result's first 256 bytes.
struct RleHead {
  int kept;
  int reserved0;
  long long total_runs;
  long long reserved1[30];
};
static_assert(sizeof(RleHead) == 256, "the layout include/mnc_hip.h documents");

// grid 1, block 64.  run_ptr [cap + 1]: instance i has sums[i] + 1 runs; the entries past the count repeat the total.
__global__ __launch_bounds__(64) void rle_scan_runs_kernel(MaskSet A, int cap, const int* __restrict__ sums, RleHead* __restrict__ head,
                                                           long long* __restrict__ run_ptr) {
  const int lane = threadIdx.x;
  const int n = mask_count(A, cap);
  long long base = 0;
  for (int i0 = 0; i0 <= cap; i0 += 64) {
    const int i = i0 + lane;
    const long long v = i < n ? (long long)sums[i] + 1 : 0, incl = wave_incl_scan(v, lane);
    if (i <= cap) run_ptr[i] = base + incl - v;
    base += __shfl(incl, 63);
  }
  if (lane == 0) {
    RleHead h = {};
    h.kept = n;
    h.total_runs = base;
    *head = h;
  }
}

// grid ceil(runs_cap / 256), block 256.  runs[j] = the length of run j: the difference of the positions on its two sides.
__global__ __launch_bounds__(kRleThreads) void rle_diff_kernel(const RleHead* __restrict__ head, const long long* __restrict__ run_ptr,
                                                               const unsigned* __restrict__ pos, long long runs_cap, unsigned HW,
                                                               unsigned* __restrict__ runs) {
  const long long j = (long long)blockIdx.x * kRleThreads + threadIdx.x;
  if (j >= runs_cap || j >= head->total_runs) return;
  int lo = 0, hi = head->kept - 1;                       // the last instance whose first run is <= j (every instance has a run)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (run_ptr[mid] <= j) lo = mid; else hi = mid - 1;
  }
  const unsigned before = j > run_ptr[lo] ? pos[j - 1] : 0u;
  const unsigned behind = j + 1 < run_ptr[lo + 1] ? pos[j] : HW;
  runs[j] = behind - before;
}

// What rle_bounds_kernel makes of one instance.
struct RleBox {
  int x1, y1, x2, y2;
  long long area;
  long long reserved;
};

// grid n, block 256.  starts[j] = the position at which run j begins (run_ptr's numbering); the runs of odd index are the 1s.
__global__ __launch_bounds__(kRleThreads) void rle_bounds_kernel(const long long* __restrict__ run_ptr, const unsigned* __restrict__ starts,
                                                                 int H, unsigned HW, RleBox* __restrict__ boxes) {
  __shared__ int s_box[kRleWaves][4];
  __shared__ long long s_area[kRleWaves];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long lo = run_ptr[i], count = run_ptr[i + 1] - lo;
  int x1 = 0x7fffffff, y1 = 0x7fffffff, x2 = -1, y2 = -1;
  long long area = 0;
  for (long long m = 1 + 2 * (long long)threadIdx.x; m < count; m += 2 * kRleThreads) {
    const unsigned s = starts[lo + m], e = m + 1 < count ? starts[lo + m + 1] : HW;
    if (e <= s) continue;                                // a run of length 0 covers nothing
    const int xs = (int)(s / (unsigned)H), xe = (int)((e - 1) / (unsigned)H);
    const int ys = (int)(s - (unsigned)xs * H), ye = (int)(e - 1 - (unsigned)xe * H);
    x1 = min(x1, xs); x2 = max(x2, xe);
    y1 = min(y1, xs == xe ? ys : 0); y2 = max(y2, xs == xe ? ye : H - 1);
    area += e - s;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x1 = min(x1, __shfl_xor(x1, o)); y1 = min(y1, __shfl_xor(y1, o));
    x2 = max(x2, __shfl_xor(x2, o)); y2 = max(y2, __shfl_xor(y2, o));
    area += __shfl_xor(area, o);
  }
  if (lane == 0) { s_box[wave][0] = x1; s_box[wave][1] = y1; s_box[wave][2] = x2; s_box[wave][3] = y2; s_area[wave] = area; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kRleWaves; ++k) {
      x1 = min(x1, s_box[k][0]); y1 = min(y1, s_box[k][1]); x2 = max(x2, s_box[k][2]); y2 = max(y2, s_box[k][3]);
      area += s_area[k];
    }
    RleBox b = {};
    if (area > 0) { b.x1 = x1; b.y1 = y1; b.x2 = x2; b.y2 = y2; } else { b.x2 = -1; b.y2 = -1; }
    b.area = area;
    boxes[i] = b;
  }
}

// grid (ceil(items / 4), n), block 256: wave = one (instance blockIdx.y, strip, tile) of the instance's own bounds, strips fastest.
// info: bounds inside the image and offsets; every word of every row is stored once.
__global__ __launch_bounds__(kRleThreads) void rle_fill_kernel(const mnc_mask_info* __restrict__ info, const long long* __restrict__ run_ptr,
                                                               const unsigned* __restrict__ starts, int H, unsigned HW,
                                                               u64* __restrict__ bits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.y, item = blockIdx.x * kRleWaves + wave;
  const mnc_mask_info m = info[i];
  const int w = m.x2 - m.x1 + 1, h = m.y2 - m.y1 + 1;
  if (w < 1 || h < 1) return;
  const int strips = mask_strips(w), tiles = (h + 63) >> 6;
  const int strip = item % strips, tile = item / strips;
  if (tile >= tiles) return;                             // (uniform over the wave)
  const int rows = min(64, h - tile * 64);
  const int x = m.x1 + strip * 64 + lane;
  u64 col = 0ull;
  if (x <= m.x2) {
    const unsigned* st = starts + run_ptr[i];
    const long long count = run_ptr[i + 1] - run_ptr[i];
    const unsigned p0 = (unsigned)x * (unsigned)H + (unsigned)(m.y1 + tile * 64), end = p0 + (unsigned)rows;
    long long lo = 0, hi = count - 1;                    // the last run that begins at or before p0 (run 0 begins at 0)
    while (lo < hi) {
      const long long mid = (lo + hi + 1) >> 1;
      if (st[mid] <= p0) lo = mid; else hi = mid - 1;
    }
    unsigned cur = p0;
    for (long long r = lo; r < count && cur < end; ++r) {
      const unsigned stop = min(r + 1 < count ? st[r + 1] : HW, end);
      if (stop <= cur) continue;                         // a run of length 0
      if (r & 1) {
        const int a = (int)(cur - p0), len = (int)(stop - cur);
        col |= (len == 64 ? ~0ull : (1ull << len) - 1ull) << a;
      }
      cur = stop;
    }
  }
  u64 mine = 0ull;
#pragma unroll
  for (int r = 0; r < 64; ++r) {
    const u64 b = __ballot((col >> r) & 1ull);
    if (lane == r) mine = b;
  }
  if (lane < rows) bits[m.offset / 8 + (long long)(tile * 64 + lane) * strips + strip] = mine;
}

namespace {

// Buffers of one encoding of a set of capacity `cap` in an image W wide, and its launch sequence.
struct RleWs {
  int *cols, *sums;
  unsigned* pos;
  int stride;
  void layout(WsLayout& l, int cap, int W, size_t runs_cap) {
    stride = cdiv(W, 64) * 64;
    cols = l.take<int>((size_t)cap * stride);
    sums = l.take<int>(cap);
    pos = l.take<unsigned>(runs_cap);
  }
};

// out: [RleHead | run_ptr [cap + 1] | runs [runs_cap]].  The bytes of it in front of the runs:
inline size_t rle_front(int cap) { return sizeof(RleHead) + ((size_t)cap + 1) * 8; }

void rle_launch(hipStream_t s, const MaskSet& A, int cap, int H, int W, const RleWs& w, void* out, size_t runs_cap) {
  RleHead* head = (RleHead*)out;
  long long* run_ptr = (long long*)((char*)out + sizeof(RleHead));
  unsigned* runs = (unsigned*)((char*)out + rle_front(cap));
  const dim3 grid(cdiv(w.stride / 64, kRleWaves), cap);
  hipLaunchKernelGGL(rle_columns_kernel<false>, grid, dim3(kRleThreads), 0, s, A, cap, H, W, w.stride, w.cols, nullptr, nullptr, 0LL);
  hipLaunchKernelGGL(rle_scan_columns_kernel, dim3(cap), dim3(64), 0, s, A, cap, H, W, w.stride, w.cols, w.sums);
  hipLaunchKernelGGL(rle_scan_runs_kernel, dim3(1), dim3(64), 0, s, A, cap, w.sums, head, run_ptr);
  if (runs_cap == 0) return;
  hipLaunchKernelGGL(rle_columns_kernel<true>, grid, dim3(kRleThreads), 0, s, A, cap, H, W, w.stride, w.cols, run_ptr, w.pos,
                     (long long)runs_cap);
  hipLaunchKernelGGL(rle_diff_kernel, dim3((unsigned)((runs_cap + kRleThreads - 1) / kRleThreads)), dim3(kRleThreads), 0, s, head,
                     run_ptr, w.pos, (long long)runs_cap, (unsigned)H * (unsigned)W, runs);
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_rle(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, int H, int W, long long* run_ptr,
                 unsigned* runs, size_t runs_cap, size_t* runs_total, int device_id) {
  MNC_REQUIRE(n >= 0 && n <= kRleMaxN, "mnc_mask_rle: n=%d not in [0, %d]", n, kRleMaxN);
  MNC_REQUIRE(H >= 1 && W >= 1 && H <= kRleMaxSide && W <= kRleMaxSide, "mnc_mask_rle: image %d x %d not in [1, %d]", H, W, kRleMaxSide);
  MNC_REQUIRE(run_ptr && runs_total, "mnc_mask_rle: null output pointer");
  HostMaskSet set;
  int rc = set.check("mnc_mask_rle", "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
  if (rc) return rc;
  *runs_total = 0;
  run_ptr[0] = 0;
  if (n == 0) { clear_error(); return MNC_OK; }
  // a column holds at most one transition per row of the extent and the one at row 0 that closes the run of the column before; an
  // instance has one run more than transitions: room beyond that is never used
  size_t most = 0;
  int widest = 1;
  for (int i = 0; i < n; ++i) {
    int ncols, nrows;
    const mnc_mask_info& m = set.info[i];
    rle_extent(m.x1, m.y1, m.x2, m.y2, H, W, &ncols, &nrows);
    most += (size_t)ncols * ((size_t)nrows + 1) + 1;
    if (ncols > widest) widest = ncols;
  }
  const size_t cap = !runs ? 0 : runs_cap < most ? runs_cap : most;
  RleWs w; char* d_out;
  auto layout = [&](WsLayout l) {
    set.take(l);
    w.layout(l, n, widest, cap);
    d_out = l.take<char>(rle_front(n) + cap * 4);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(set.upload(hs));
  rle_launch(hs.stream, set.view(), n, H, W, w, d_out, cap);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(run_ptr, d_out + sizeof(RleHead), ((size_t)n + 1) * 8));
  MNC_HIP_TRY(hs.sync());
  const size_t total = (size_t)run_ptr[n];
  *runs_total = total;
  if (!runs) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(runs_cap >= total, "mnc_mask_rle: runs_cap %zu is below the %zu runs of the masks", runs_cap, total);
  MNC_HIP_TRY(hs.down(runs, d_out + rle_front(n), total * 4));
  MNC_HIP_TRY(hs.sync());
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_rle_dev(mnc_ctx* ctx, const void* d_info, const void* d_bits, int rows_cap, int H, int W, size_t runs_cap, void** d_rle) {
  MNC_REQUIRE(ctx && d_rle, "mnc_mask_rle_dev: null pointer");
  MNC_REQUIRE(rows_cap >= 0 && rows_cap <= kRleMaxN, "mnc_mask_rle_dev: rows_cap=%d not in [0, %d]", rows_cap, kRleMaxN);
  MNC_REQUIRE(H >= 1 && W >= 1 && H <= kRleMaxSide && W <= kRleMaxSide, "mnc_mask_rle_dev: image %d x %d not in [1, %d]", H, W,
              kRleMaxSide);
  MNC_REQUIRE(runs_cap <= (size_t)1 << 32, "mnc_mask_rle_dev: runs_cap %zu above 2^32", runs_cap);
  MNC_REQUIRE(d_info && (d_bits || rows_cap == 0), "mnc_mask_rle_dev: null device pointer");
  MNC_NO_CAPTURE(ctx, "mnc_mask_rle_dev");
  RleWs w; char* out;
  auto layout = [&](WsLayout l) {
    out = l.take<char>(rle_front(rows_cap) + runs_cap * 4);
    w.layout(l, rows_cap, W, runs_cap);
    return l.bytes();
  };
  // an arena of its own: mask_ws holds the masks this call reads.  In no captured graph.
  int rc = arena_ensure(&ctx->rle_ws, layout(WsLayout()), 0, "mask-rle buffers", ctx->stream, ctx);
  if (rc) return rc;
  layout(WsLayout(ctx->rle_ws.p));
  LaunchScope ls(ctx, "mask_rle");
  hipStream_t s = ctx->stream;
  if (rows_cap == 0) {
    MNC_HIP_TRY(hipMemsetAsync(out, 0, rle_front(0), s));
  } else {
    rle_launch(s, MaskSet::of_records(d_info, d_bits, rows_cap), rows_cap, H, W, w, out, runs_cap);
  }
  rc = ls.finish("mask_rle");
  if (rc) return rc;
  *d_rle = out;
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_from_rle(const long long* run_ptr, const unsigned* runs, int n, int H, int W, int* bounds, long long* offsets,
                      long long* areas, void* bits, size_t bits_cap, size_t* bits_bytes, int device_id) {
  MNC_REQUIRE(n >= 0 && n <= kRleMaxN, "mnc_mask_from_rle: n=%d not in [0, %d]", n, kRleMaxN);
  MNC_REQUIRE(H >= 1 && W >= 1 && H <= kRleMaxSide && W <= kRleMaxSide, "mnc_mask_from_rle: image %d x %d not in [1, %d]", H, W,
              kRleMaxSide);
  MNC_REQUIRE(bits_bytes, "mnc_mask_from_rle: null bits_bytes");
  *bits_bytes = 0;
  if (n == 0) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(run_ptr && bounds && offsets && areas, "mnc_mask_from_rle: null pointer");
  MNC_REQUIRE(run_ptr[0] >= 0, "mnc_mask_from_rle: run_ptr[0]=%lld is negative", run_ptr[0]);
  for (int i = 0; i < n; ++i)
    MNC_REQUIRE(run_ptr[i + 1] >= run_ptr[i], "mnc_mask_from_rle: run_ptr decreases at %d", i + 1);
  MNC_REQUIRE(runs || run_ptr[n] == run_ptr[0], "mnc_mask_from_rle: null runs");
  // the position at which every run begins; the counts of one mask sum to H * W exactly
  const unsigned HW = (unsigned)H * (unsigned)W;
  const long long first = run_ptr[0], total = run_ptr[n] - first;
  std::vector<unsigned> starts;
  std::vector<long long> ptr((size_t)n + 1);
  try {
    starts.resize((size_t)total);
  } catch (const std::exception&) {
    set_error("mnc_mask_from_rle: no host memory for the start positions of %lld runs", total);
    return MNC_ERR_NOMEM;
  }
  for (int i = 0; i <= n; ++i) ptr[i] = run_ptr[i] - first;
  for (int i = 0; i < n; ++i) {
    unsigned long long at = 0;
    for (long long j = run_ptr[i]; j < run_ptr[i + 1]; ++j) {
      starts[(size_t)(j - first)] = (unsigned)at;
      at += runs[j];
      MNC_REQUIRE(at <= HW, "mnc_mask_from_rle: the counts of mask %d sum past %d x %d", i, H, W);
    }
    MNC_REQUIRE(at == HW, "mnc_mask_from_rle: the counts of mask %d sum to %llu, not %d x %d", i, at, H, W);
  }
  // no tight box is larger than the image: room beyond that is never used
  const size_t image = (size_t)H * mask_strips(W) * 8, most = image * n;
  const size_t room = !bits ? 0 : (bits_cap < most ? bits_cap : most) & ~(size_t)7;
  long long* d_ptr; unsigned* d_starts; RleBox* d_boxes; mnc_mask_info* d_info; u64* d_bits;
  auto layout = [&](WsLayout l) {
    d_ptr = l.take<long long>((size_t)n + 1);
    d_starts = l.take<unsigned>((size_t)total);
    d_boxes = l.take<RleBox>(n);
    d_info = l.take<mnc_mask_info>(n);
    d_bits = l.take<u64>(room / 8);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(hs.up(d_ptr, ptr.data(), ((size_t)n + 1) * 8));
  MNC_HIP_TRY(hs.up(d_starts, starts.data(), (size_t)total * 4));
  hipLaunchKernelGGL(rle_bounds_kernel, dim3(n), dim3(kRleThreads), 0, hs.stream, d_ptr, d_starts, H, HW, d_boxes);
  MNC_HIP_TRY(hipGetLastError());
  std::vector<RleBox> boxes((size_t)n);
  MNC_HIP_TRY(hs.down(boxes.data(), d_boxes, (size_t)n * sizeof(RleBox)));
  MNC_HIP_TRY(hs.sync());
  std::vector<mnc_mask_info> info((size_t)n);
  size_t need = 0;
  int items = 0;
  for (int i = 0; i < n; ++i) {
    const RleBox& b = boxes[i];
    const int w = b.x2 - b.x1 + 1, h = b.y2 - b.y1 + 1;
    mnc_mask_info& d = info[i];
    d = mnc_mask_info();
    d.x1 = b.x1; d.y1 = b.y1; d.x2 = b.x2; d.y2 = b.y2;
    d.row = i;
    d.offset = (long long)need;
    d.area = b.area;
    bounds[4 * (size_t)i] = b.x1; bounds[4 * (size_t)i + 1] = b.y1; bounds[4 * (size_t)i + 2] = b.x2; bounds[4 * (size_t)i + 3] = b.y2;
    offsets[i] = d.offset;
    areas[i] = b.area;
    if (w < 1 || h < 1) continue;
    need += (size_t)h * mask_strips(w) * 8;
    if (cdiv(w, 64) * cdiv(h, 64) > items) items = cdiv(w, 64) * cdiv(h, 64);
  }
  *bits_bytes = need;
  if (!bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(bits_cap >= need, "mnc_mask_from_rle: bits_cap %zu is below the %zu bytes of the masks", bits_cap, need);
  if (need) {
    MNC_HIP_TRY(hs.up(d_info, info.data(), (size_t)n * sizeof(mnc_mask_info)));
    hipLaunchKernelGGL(rle_fill_kernel, dim3(cdiv(items, kRleWaves), n), dim3(kRleThreads), 0, hs.stream, d_info, d_ptr, d_starts, H, HW,
                       d_bits);
    MNC_HIP_TRY(hipGetLastError());
    MNC_HIP_TRY(hs.down(bits, d_bits, need));
    MNC_HIP_TRY(hs.sync());
  }
  clear_error();
  return MNC_OK;
}
