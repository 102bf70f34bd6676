// COCO polygon segmentations rasterised into packed instance masks for gfx950 (include/mnc_hip.h n9) -- the rule of the published
// maskApi.c (rleFrPoly per polygon, the OR of an annotation's polygons) landing in the PackedMasks layout of inst_masks.hip (n5).
// The rule walks every edge of the polygon at five times the image's resolution, takes the points at which the walk's u passes
// from one image column into the next as crossings, and sets pixel p of the column-major order (p = x * H + y) when the number
// of crossings at positions <= p is odd.  No pixel is tested against the polygon.
//
// Host: the vertices rounded (X = (int)(5 x + .5)), one PolyEdge per edge with the prefix of the walk lengths, and per polygon
// the rectangle of the image its crossings can fall into, from the rounded vertices alone (a margin of one pixel on every side:
// nothing is reduced on the device for it).  A polygon whose rectangle misses the image's columns has no crossing and is left out.
//   poly_toggle_kernel  one thread per walk point: bisects the edge table, forms its point and the one before it in closed form
//                       (the point before an edge's first is the last of the edge before), decides whether it is a crossing
//                       and XORs bit (x, y) into the polygon's toggle plane -- rows ry0 .. ry0 + nr - 1 of the image and one
//                       more row for the crossings clamped to y == H, 64 columns to a word, the words those of the image's
//                       columns (word = x >> 6), so that polygons of one annotation line up.  XOR commutes: atomic order does
//                       not show.  A crossing outside the host's rectangle would be a bug: it is not stored and raises a flag.
//   poly_fill_kernel    one workgroup of 16 waves per annotation, polygon after polygon, 64 words (4096 columns) at a time:
//                       lane = word, wave = a segment of the polygon's rows.  Every wave XORs its segment's toggle rows; the
//                       segments' sums go through LDS; their total (with the clamped row) is the parity every column hands on,
//                       so the parity carried INTO a column is the XOR of the totals to its left -- a bit-prefix XOR inside the
//                       word, a wave scan of the words' parities, and the carry of the 64 words before.  Then every wave
//                       walks its segment once more with the running XOR (carry ^ the segments above ^ its own rows so far)
//                       and ORs it into the annotation's plane; within a polygon a word of that plane belongs to one lane,
//                       between polygons stands a barrier.  (A walk ends in the column it began in, so it passes every column
//                       boundary an even number of times: with the clamped row counted, what a column hands on is even, and a
//                       column's carry could only be odd through a fault of the walk.  The scan carries it all the same
//                       inside the polygon's rows; rows above them, which an odd carry would also set, are not looked at.)
//                       The workgroup then reduces the tight box and the area of the plane (rleToBbox).
//   poly_write_kernel   one thread per output word: the row funnel-shifted from the plane into the tight box, the padding
//                       cleared; every word of every row is written once.
// The planes are zeroed by one memset.  Bound: a walk point costs one bisection and two divisions; the fill reads every toggle
// word twice and the plane's once per polygon.  Not measured yet (tools/mask_poly_bench.py, profiles/mask_poly_bench.txt).
#include <atomic>
#include <cmath>
#include <exception>
#include <vector>

#include "mask_set.h"

namespace mnc {


constexpr int kPolyThreads = 256;
constexpr int kPolyMaxN = 2048;                  // annotations of one call
constexpr int kPolyMaxSide = 32768;              // H, W limit
constexpr long long kPolyMaxPixels = 1ll << 30;  // H * W limit: a position fits an unsigned
constexpr long long kPolyMaxPoints = 1ll << 30;  // the walks of one call
constexpr double kPolyMaxCoord = 1048576.0;      // |x|, |y| <= 2^20: five times it fits an int with room
constexpr int kFillWaves = 16;
constexpr int kFillThreads = kFillWaves * 64;

// One edge's walk: the ends after the flip, in the rounded coordinates.
struct PolyEdge {
  long long start;         // the index of its first point among the call's walk points
  int xs, ys, xe, ye;
  int dx, dy;
  int flags;               // 1: flipped (walked from the far end), 2: the polygon's first edge (its first point has none before it)
  int plane;               // index into the planes
};

// The toggle plane of one polygon, or the pixel plane of one annotation: rows ry0 .. ry0 + nr - 1 (a toggle plane has one more
// row behind them, for y == H), image words wx0 .. wx0 + nw - 1, row-major from `words` on.
struct PolyPlane {
  long long words;
  int ry0, nr, wx0, nw;
};

struct PolyAnn {
  int first, count;        // its toggle planes
  PolyPlane px;
};

// What poly_fill_kernel makes of one annotation.
struct PolyBox {
  int x1, y1, x2, y2;
  long long area;
  long long reserved;
};

// Point d of an edge's walk.
__device__ __forceinline__ void poly_point(const PolyEdge& e, int d, int* u, int* v) {
  if (e.dx >= e.dy) {
    const int t = (e.flags & 1) ? e.dx - d : d;
    *u = t + e.xs;
    if (e.dx == 0) { *v = e.ys; return; }
    const double s = (double)(e.ye - e.ys) / e.dx;
    *v = (int)(e.ys + s * t + .5);
  } else {
    const int t = (e.flags & 1) ? e.dy - d : d;
    *v = t + e.ys;
    const double s = (double)(e.xe - e.xs) / e.dy;
    *u = (int)(e.xs + s * t + .5);
  }
}

// grid ceil(points / 256), block 256.
__global__ __launch_bounds__(kPolyThreads) void poly_toggle_kernel(const PolyEdge* __restrict__ edges, int n_edges, long long points,
                                                                   const PolyPlane* __restrict__ planes, int H, int W,
                                                                   u64* __restrict__ ws, int* __restrict__ flag) {
  const long long g = (long long)blockIdx.x * kPolyThreads + threadIdx.x;
  if (g >= points) return;
  int lo = 0, hi = n_edges - 1;                          // the last edge that starts at or before g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (edges[mid].start <= g) lo = mid; else hi = mid - 1;
  }
  const PolyEdge e = edges[lo];
  const int d = (int)(g - e.start);
  int u, v, up, vp;
  poly_point(e, d, &u, &v);
  if (d > 0) {
    poly_point(e, d - 1, &up, &vp);
  } else {
    if (e.flags & 2) return;                             // the polygon's first point
    const PolyEdge b = edges[lo - 1];
    poly_point(b, max(b.dx, b.dy), &up, &vp);
  }
  if (u == up) return;
  double xd = (double)(u < up ? u : u - 1);
  xd = (xd + .5) / 5 - .5;
  if (floor(xd) != xd || xd < 0 || xd > W - 1) return;
  double yd = (double)(v < vp ? v : vp);
  yd = (yd + .5) / 5 - .5;
  if (yd < 0) yd = 0; else if (yd > H) yd = H;
  yd = ceil(yd);
  const int x = (int)xd, y = (int)yd;
  const PolyPlane p = planes[e.plane];
  const int w = (x >> 6) - p.wx0, r = y == H ? p.nr : y - p.ry0;
  if (w < 0 || w >= p.nw || r < 0 || r > p.nr || (y < H && r == p.nr)) { *flag = 1; return; }
  atomicXor(ws + p.words + (long long)r * p.nw + w, 1ull << (x & 63));
}

// bit k of the result = the XOR of bits 0 .. k of v
__device__ __forceinline__ u64 poly_prefix_xor(u64 v) {
  v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16; v ^= v << 32;
  return v;
}

// grid n, block 1024: one annotation.
__global__ __launch_bounds__(kFillThreads) void poly_fill_kernel(const PolyAnn* __restrict__ anns, const PolyPlane* __restrict__ planes,
                                                                 u64* __restrict__ ws, PolyBox* __restrict__ boxes) {
  __shared__ u64 s_seg[kFillWaves][64];
  __shared__ int s_box[kFillWaves][4];
  __shared__ long long s_area[kFillWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PolyAnn a = anns[blockIdx.x];
  u64* px = ws + a.px.words;
  for (int q = a.first; q < a.first + a.count; ++q) {
    const PolyPlane p = planes[q];
    const u64* tg = ws + p.words;
    const int per = (p.nr + kFillWaves - 1) / kFillWaves;           // rows of a segment
    const int r0 = min(wave * per, p.nr), r1 = min(r0 + per, p.nr);
    int before = 0;                                                   // the parity of the polygon's words before this chunk
    for (int c0 = 0; c0 < p.nw; c0 += 64) {                           // (uniform over the workgroup)
      const int w = c0 + lane;
      const bool live = w < p.nw;
      u64 seg = 0ull;
      if (live)
        for (int r = r0; r < r1; ++r) seg ^= tg[(long long)r * p.nw + w];
      __syncthreads();                                                // (the chunk before has been read)
      s_seg[wave][lane] = seg;
      __syncthreads();
      u64 above = 0ull, total = live ? tg[(long long)p.nr * p.nw + w] : 0ull;   // the clamped row counts for its column's total
#pragma unroll
      for (int k = 0; k < kFillWaves; ++k) {
        const u64 t = s_seg[k][lane];
        if (k < wave) above ^= t;
        total ^= t;
      }
      // the parity carried into column b of this word: the totals of the columns before it
      int odd = __popcll(total) & 1, incl = odd;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl ^= t;
      }
      const int words_before = before ^ incl ^ odd;
      before ^= __shfl(incl, 63);
      u64 run = (poly_prefix_xor(total) << 1) ^ (words_before ? ~0ull : 0ull) ^ above;
      if (live) {
        u64* out = px + (long long)(p.ry0 - a.px.ry0) * a.px.nw + (p.wx0 - a.px.wx0) + w;
        for (int r = r0; r < r1; ++r) {
          run ^= tg[(long long)r * p.nw + w];
          if (run) out[(long long)r * a.px.nw] |= run;
        }
      }
    }
    __syncthreads();                                                  // the next polygon's lanes are other lanes of these words
  }
  // the tight box and the area of what stands in the plane now
  int x1 = 0x7fffffff, y1 = 0x7fffffff, x2 = -1, y2 = -1;
  long long area = 0;
  const long long count = (long long)a.px.nr * a.px.nw;
  for (long long k = threadIdx.x; k < count; k += kFillThreads) {
    const u64 v = px[k];
    if (v == 0ull) continue;
    const int r = (int)(k / a.px.nw), w = (int)(k - (long long)r * a.px.nw);
    const int x = (a.px.wx0 + w) << 6, y = a.px.ry0 + r;
    x1 = min(x1, x + __ffsll(v) - 1); x2 = max(x2, x + 63 - __clzll(v));
    y1 = min(y1, y); y2 = max(y2, y);
    area += __popcll(v);
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
    for (int k = 1; k < kFillWaves; ++k) {
      x1 = min(x1, s_box[k][0]); y1 = min(y1, s_box[k][1]); x2 = max(x2, s_box[k][2]); y2 = max(y2, s_box[k][3]);
      area += s_area[k];
    }
    PolyBox b = {};
    if (area > 0) { b.x1 = x1; b.y1 = y1; b.x2 = x2; b.y2 = y2; } else { b.x2 = -1; b.y2 = -1; }
    b.area = area;
    boxes[blockIdx.x] = b;
  }
}

// grid (ceil(most words / 256), n), block 256.  info: the tight bounds inside the image and the offsets.
__global__ __launch_bounds__(kPolyThreads) void poly_write_kernel(const mnc_mask_info* __restrict__ info, const PolyAnn* __restrict__ anns,
                                                                  const u64* __restrict__ ws, u64* __restrict__ bits) {
  const mnc_mask_info m = info[blockIdx.y];
  const int w = m.x2 - m.x1 + 1, h = m.y2 - m.y1 + 1;
  if (w < 1 || h < 1) return;
  const int strips = mask_strips(w);
  const long long k = (long long)blockIdx.x * kPolyThreads + threadIdx.x;
  if (k >= (long long)h * strips) return;
  const int r = (int)(k / strips), s = (int)(k - (long long)r * strips);
  const PolyPlane p = anns[blockIdx.y].px;                // the box lies inside the plane: its pixels are the plane's
  const u64* row = ws + p.words + (long long)(m.y1 + r - p.ry0) * p.nw;
  const int off = m.x1 + (s << 6) - (p.wx0 << 6), j = off >> 6, sh = off & 63;
  u64 v = row[j] >> sh;
  if (sh && j + 1 < p.nw) v |= row[j + 1] << (64 - sh);
  const int valid = w - (s << 6);
  if (valid < 64) v &= (1ull << valid) - 1ull;
  bits[m.offset / 8 + k] = v;
}

namespace {

// mnc_mask_poly_timing: a HIP event pair around each group of launches of the next calls, their sum kept (tools/mask_poly_bench.py)
CallTimer g_poly_timer;

inline int floordiv5(int a) { return a >= 0 ? a / 5 : -((4 - a) / 5); }
inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_from_polygons(const double* xy, const long long* vert_ptr, const long long* poly_ptr, int n, int H, int W, int* bounds,
                           long long* offsets, long long* areas, void* bits, size_t bits_cap, size_t* bits_bytes, int device_id) {
  MNC_REQUIRE(n >= 0 && n <= kPolyMaxN, "mnc_mask_from_polygons: n=%d not in [0, %d]", n, kPolyMaxN);
  MNC_REQUIRE(H >= 1 && W >= 1 && H <= kPolyMaxSide && W <= kPolyMaxSide, "mnc_mask_from_polygons: image %d x %d not in [1, %d]", H, W,
              kPolyMaxSide);
  MNC_REQUIRE((long long)H * W <= kPolyMaxPixels, "mnc_mask_from_polygons: image %d x %d has more than 2^30 pixels", H, W);
  MNC_REQUIRE(bits_bytes, "mnc_mask_from_polygons: null bits_bytes");
  *bits_bytes = 0;
  if (n == 0) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(poly_ptr && bounds && offsets && areas, "mnc_mask_from_polygons: null pointer");
  MNC_REQUIRE(poly_ptr[0] >= 0, "mnc_mask_from_polygons: poly_ptr[0]=%lld is negative", poly_ptr[0]);
  for (int i = 0; i < n; ++i)
    MNC_REQUIRE(poly_ptr[i + 1] >= poly_ptr[i], "mnc_mask_from_polygons: poly_ptr decreases at %d", i + 1);
  const long long q0 = poly_ptr[0], q1 = poly_ptr[n];
  MNC_REQUIRE(q1 == q0 || (vert_ptr && xy), "mnc_mask_from_polygons: null vert_ptr or xy");
  MNC_REQUIRE(q1 == q0 || vert_ptr[q0] >= 0, "mnc_mask_from_polygons: vert_ptr[%lld]=%lld is negative", q0, q1 == q0 ? 0 : vert_ptr[q0]);
  long long points = 0;
  for (long long q = q0; q < q1; ++q) {
    MNC_REQUIRE(vert_ptr[q + 1] >= vert_ptr[q], "mnc_mask_from_polygons: vert_ptr decreases at %lld", q + 1);
    MNC_REQUIRE(vert_ptr[q + 1] > vert_ptr[q], "mnc_mask_from_polygons: polygon %lld has no vertices", q);
  }
  if (q1 > q0)
    for (long long j = 2 * vert_ptr[q0]; j < 2 * vert_ptr[q1]; ++j)
      MNC_REQUIRE(std::isfinite(xy[j]) && std::fabs(xy[j]) <= kPolyMaxCoord,
                  "mnc_mask_from_polygons: coordinate %lld (%g) is not finite or of magnitude above 2^20", j, xy[j]);
  // the edges, and per polygon the rectangle its crossings can fall into
  std::vector<PolyEdge> edges;
  std::vector<PolyPlane> planes;
  std::vector<PolyAnn> anns((size_t)n);
  std::vector<int> X, Y;
  long long words = 0, launched = 0;
  try {
    for (int i = 0; i < n; ++i) {
      PolyAnn& a = anns[i];
      a.first = (int)planes.size();
      int ay0 = H, ay1 = -1, aw0 = 0x7fffffff, aw1 = -1;
      for (long long q = poly_ptr[i]; q < poly_ptr[i + 1]; ++q) {
        const long long k = vert_ptr[q + 1] - vert_ptr[q];
        const double* p = xy + 2 * vert_ptr[q];
        X.resize((size_t)k + 1); Y.resize((size_t)k + 1);
        int lox = 0x7fffffff, hix = -0x7fffffff, loy = 0x7fffffff, hiy = -0x7fffffff;
        for (long long j = 0; j < k; ++j) {
          X[j] = (int)(5 * p[2 * j] + .5); Y[j] = (int)(5 * p[2 * j + 1] + .5);
          lox = X[j] < lox ? X[j] : lox; hix = X[j] > hix ? X[j] : hix;
          loy = Y[j] < loy ? Y[j] : loy; hiy = Y[j] > hiy ? Y[j] : hiy;
        }
        X[k] = X[0]; Y[k] = Y[0];
        long long walk = 0;
        for (long long j = 0; j < k; ++j) {
          const long long dx = std::llabs((long long)X[j + 1] - X[j]), dy = std::llabs((long long)Y[j] - Y[j + 1]);
          walk += (dx >= dy ? dx : dy) + 1;
        }
        points += walk;
        MNC_REQUIRE(points <= kPolyMaxPoints, "mnc_mask_from_polygons: the walks have more than 2^30 points");
        // u lies within one unit of [lox, hix], a crossing's column is (u - 2) / 5 or (u - 3) / 5; v and the rows alike
        const int cx0 = clampi(floordiv5(lox - 5), 0, W), cx1 = clampi(floordiv5(hix + 5), -1, W - 1);
        if (cx0 > cx1) continue;                         // no crossing inside the image's columns: an empty polygon
        // (the rule clamps a crossing's row to [0, H]: a polygon above the image toggles row 0, one below it the row for y == H)
        const int ry0 = clampi(floordiv5(loy - 5), 0, H), ry1 = clampi(floordiv5(hiy + 5) + 1, 0, H - 1);
        PolyPlane t;
        t.words = words;
        t.ry0 = ry0; t.nr = ry1 >= ry0 ? ry1 - ry0 + 1 : 0;
        t.wx0 = cx0 >> 6; t.nw = (cx1 >> 6) - t.wx0 + 1;
        words += ((long long)t.nr + 1) * t.nw;
        if (t.nr) {
          ay0 = ry0 < ay0 ? ry0 : ay0; ay1 = ry1 > ay1 ? ry1 : ay1;
          aw0 = t.wx0 < aw0 ? t.wx0 : aw0; aw1 = t.wx0 + t.nw - 1 > aw1 ? t.wx0 + t.nw - 1 : aw1;
        }
        for (long long j = 0; j < k; ++j) {
          PolyEdge e;
          e.start = launched;
          e.xs = X[j]; e.xe = X[j + 1]; e.ys = Y[j]; e.ye = Y[j + 1];
          e.dx = std::abs(e.xe - e.xs); e.dy = std::abs(e.ys - e.ye);
          const bool flip = (e.dx >= e.dy && e.xs > e.xe) || (e.dx < e.dy && e.ys > e.ye);
          if (flip) { int s = e.xs; e.xs = e.xe; e.xe = s; s = e.ys; e.ys = e.ye; e.ye = s; }
          e.flags = (flip ? 1 : 0) | (j == 0 ? 2 : 0);
          e.plane = (int)planes.size();
          launched += (e.dx >= e.dy ? e.dx : e.dy) + 1;
          edges.push_back(e);
        }
        planes.push_back(t);
      }
      a.count = (int)planes.size() - a.first;
      a.px.words = 0;
      a.px.ry0 = ay1 >= ay0 ? ay0 : 0; a.px.nr = ay1 >= ay0 ? ay1 - ay0 + 1 : 0;
      a.px.wx0 = ay1 >= ay0 ? aw0 : 0; a.px.nw = ay1 >= ay0 ? aw1 - aw0 + 1 : 0;
    }
  } catch (const std::exception&) {
    set_error("mnc_mask_from_polygons: no host memory for the edge table");
    return MNC_ERR_NOMEM;
  }
  for (int i = 0; i < n; ++i) {
    anns[i].px.words = words;
    words += (long long)anns[i].px.nr * anns[i].px.nw;
  }
  // no tight box is larger than the image: room beyond that is never used
  const size_t image = (size_t)H * mask_strips(W) * 8, most = image * n;
  const size_t room = !bits ? 0 : (bits_cap < most ? bits_cap : most) & ~(size_t)7;
  PolyEdge* d_edges; PolyPlane* d_planes; PolyAnn* d_anns; PolyBox* d_boxes; mnc_mask_info* d_info; int* d_flag; u64* d_ws; u64* d_bits;
  auto layout = [&](WsLayout l) {
    d_edges = l.take<PolyEdge>(edges.size());
    d_planes = l.take<PolyPlane>(planes.size());
    d_anns = l.take<PolyAnn>(n);
    d_boxes = l.take<PolyBox>(n);
    d_info = l.take<mnc_mask_info>(n);
    d_flag = l.take<int>(1);
    d_ws = l.take<u64>((size_t)words);
    d_bits = l.take<u64>(room / 8);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(hs.up(d_edges, edges.data(), edges.size() * sizeof(PolyEdge)));
  MNC_HIP_TRY(hs.up(d_planes, planes.data(), planes.size() * sizeof(PolyPlane)));
  MNC_HIP_TRY(hs.up(d_anns, anns.data(), (size_t)n * sizeof(PolyAnn)));
  TimedSpan rasterise(g_poly_timer), write(g_poly_timer);
  rasterise.begin(hs.stream);
  MNC_HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), hs.stream));
  if (words) MNC_HIP_TRY(hipMemsetAsync(d_ws, 0, (size_t)words * 8, hs.stream));
  if (launched)
    hipLaunchKernelGGL(poly_toggle_kernel, dim3((unsigned)((launched + kPolyThreads - 1) / kPolyThreads)), dim3(kPolyThreads), 0,
                       hs.stream, d_edges, (int)edges.size(), launched, d_planes, H, W, d_ws, d_flag);
  hipLaunchKernelGGL(poly_fill_kernel, dim3(n), dim3(kFillThreads), 0, hs.stream, d_anns, d_planes, d_ws, d_boxes);
  rasterise.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  std::vector<PolyBox> boxes((size_t)n);
  int flag = 0;
  MNC_HIP_TRY(hs.down(boxes.data(), d_boxes, (size_t)n * sizeof(PolyBox)));
  MNC_HIP_TRY(hs.down(&flag, d_flag, sizeof(int)));
  MNC_HIP_TRY(hs.sync());
  rasterise.keep();                    // what a sizes-only call leaves
  if (flag) {
    set_error("mnc_mask_from_polygons: a crossing fell outside the rectangle the host made for its polygon (a bug)");
    return MNC_ERR_STATE;
  }
  std::vector<mnc_mask_info> info((size_t)n);
  size_t need = 0;
  long long most_words = 0;
  for (int i = 0; i < n; ++i) {
    const PolyBox& b = boxes[i];
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
    const long long count = (long long)h * mask_strips(w);
    need += (size_t)count * 8;
    if (count > most_words) most_words = count;
  }
  *bits_bytes = need;
  if (!bits) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(bits_cap >= need, "mnc_mask_from_polygons: bits_cap %zu is below the %zu bytes of the masks", bits_cap, need);
  if (need) {
    MNC_HIP_TRY(hs.up(d_info, info.data(), (size_t)n * sizeof(mnc_mask_info)));
    write.begin(hs.stream);
    hipLaunchKernelGGL(poly_write_kernel, dim3((unsigned)((most_words + kPolyThreads - 1) / kPolyThreads), n), dim3(kPolyThreads), 0,
                       hs.stream, d_info, d_anns, d_ws, d_bits);
    write.end(hs.stream);
    MNC_HIP_TRY(hipGetLastError());
    MNC_HIP_TRY(hs.down(bits, d_bits, need));
    MNC_HIP_TRY(hs.sync());
    write.keep_sum(rasterise);
  }
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_poly_timing(int on, double* last_ms) { return g_poly_timer.set(on, last_ms); }
