// COCO's matching of one image's detections to its ground truths (the published cocoeval.py: computeIoU, evaluateImg; rleIou of
// maskApi.c for the crowd union) on two sets of packed masks (include/mnc_hip.h n5, n8), for gfx950.  The statement of the rule is
// mnc_amd/coco_eval.py:match_numpy; this file computes the same tables bit for bit.
//
//   mask_overlaps_kernel    (mask_overlaps.hip, through overlaps_launch, unchanged) inter[d][g], the count alone.
//   match_lists_kernel      one thread per detection and per ground truth, by counting (as mask_order_kernel orders the NMS):
//                           rank[d] = detections of d's class with a higher score, or the same score and a lower index; dpos[d]
//                           = detections of a lower class + rank[d], so that dsorted[] lists the detections class by class in
//                           rank order; gpos[g] alike by (class, index); per detection the range its class takes in both lists;
//                           per ground truth and area range the ignore flag gig[a][g].
//   match_iou_kernel        one thread per pair: union = crowd ? area_d : area_d + area_g - inter, iou = union < 1 ? 0.0 :
//                           (double)inter / (double)union, stored in the caller's order (the optional output) and once more at
//                           [dpos[d]][gpos[g]]: a class's block of that table is contiguous in both directions.
//   match_iou_min_kernel    (mnc_mask_match_boundary, n11) match_iou_kernel's sibling: the same arithmetic on the masks' counts and
//                           once more on the counts of the two sets' boundary bands (mask_boundary.hip), the smaller of the two
//                           IoUs stored where match_iou_kernel stores its one, the boundary IoU alone in a table of its own.
//   match_cells_kernel      one wave per (class, area range, threshold) cell -- they are independent.  The cell of a class is
//                           run by the wave numbered after the class's best detection (rank 0); every other wave leaves at once.
//                           The wave walks the class's detections in rank order; its 64 lanes hold the class's ground truths in
//                           chunks of 64 (lane l of chunk c: position 64 c + l of the class's list).  Each lane keeps the ignore,
//                           crowd and matched state of its ground truths as one bit per chunk in three 32-bit registers (at most
//                           2048 / 64 = 32 chunks), so nothing is indexed dynamically and nothing goes to scratch.  The choice
//                           of a detection is the closed form of evaluateImg's walk: among the candidates of a chunk (a ballot;
//                           no candidate, no reduction) a wave max-reduction of the IoU, then a ballot of the lanes that equal
//                           the maximum, whose highest set bit is the tie rule; a later chunk wins on >=.  Not-ignored ground
//                           truths are looked at first; ignored ones (a crowd one however often) only while no not-ignored one
//                           was found.  Lane 0 stores the cell's results -- one thread, program order: the last detection
//                           that takes a crowd ground truth is the one gt_match keeps.
// No atomics, no host read-back between the passes, every table written with ordinary vector stores (the result tables are
// first filled with -1 / 0 by hipMemsetAsync on the same stream): the same bits from run to run.
//
// Bound: latency.  A cell is a serial walk over at most max_det detections, one coalesced row read of 512 bytes a chunk each;
// the next detection's first row is requested before the current one is reduced.  The cells of an image (classes x 4 x 10) run
// side by side, one wave each.
//
// Compiled with -ffp-contract=off as mask_overlaps.hip is (the lone division has nothing to contract with).
#include <cmath>
#include <vector>

#include "mask_set.h"

namespace mnc {

constexpr int kMtThreads = 256;
constexpr int kMtWaves = kMtThreads / 64;
constexpr int kMtMaxN = 2048;                  // detections / ground truths of one image: 32 chunks of 64, one bit each
constexpr int kMtMaxT = 16;
constexpr int kMtMaxA = 8;

// The ground truths' side of a call on the device, and the parameters.
struct MtGt {
  const mnc_mask_info* info;                   // cls, area: the instance table uploaded with the set
  const unsigned char* crowd;                  // [G] 0 / 1
  const unsigned char* ignore;                 // [G] 0 / 1
  const double* eval_area;                     // [G]
  const double* thrs;                          // [T]
  const double* rngs;                          // [A][2]
  int G, T, A, max_det;
};

// The lists of match_lists_kernel.  dcap = the capacity the detections' buffers were sized with.
struct MtLists {
  int* rank;                                   // [dcap] the output
  int* dpos;                                   // [dcap] position in dsorted
  int* dsorted;                                // [dcap] detections by (class, rank)
  double* dsarea;                              // [dcap] their areas, in that order
  int* dstart;                                 // [dcap] per detection: where its class begins in dsorted,
  int* dcount;                                 //        how many detections it has,
  int* gstart;                                 //        where its class begins in gsorted,
  int* gcount;                                 //        how many ground truths it has
  int* gpos;                                   // [G] position in gsorted
  int* gsorted;                                // [G] ground truths by (class, index)
  unsigned char* gig;                          // [A][G] the output gt_ignore
};

// grid ceil(max(dcap, G) / 256), block 256.  Thread i: detection i (i < the detections' count) and ground truth i (i < G).
__global__ __launch_bounds__(kMtThreads) void match_lists_kernel(MaskSet D, int dcap, MtGt gt, MtLists L) {
  const int nd = mask_count(D, dcap);
  const int i = blockIdx.x * kMtThreads + threadIdx.x;
  if (i < dcap && i >= nd) L.rank[i] = -1;
  if (i < nd) {
    const int cls = D.info[i].cls;
    const unsigned mine = mask_score_key(D.info[i].score);
    int lower = 0, rank = 0, same = 0;
    for (int j = 0; j < nd; ++j) {
      const int c = D.info[j].cls;
      const unsigned k = mask_score_key(D.info[j].score);
      lower += c < cls ? 1 : 0;
      same += c == cls ? 1 : 0;
      rank += (c == cls && (k > mine || (k == mine && j < i))) ? 1 : 0;
    }
    int glower = 0, gsame = 0;
    for (int j = 0; j < gt.G; ++j) {
      const int c = gt.info[j].cls;
      glower += c < cls ? 1 : 0;
      gsame += c == cls ? 1 : 0;
    }
    const int pos = lower + rank;                        // < nd: a permutation
    L.rank[i] = rank;
    L.dpos[i] = pos;
    L.dsorted[pos] = i;
    L.dsarea[pos] = (double)D.info[i].area;
    L.dstart[i] = lower;
    L.dcount[i] = same;
    L.gstart[i] = glower;
    L.gcount[i] = gsame;
  }
  if (i < gt.G) {
    const int cls = gt.info[i].cls;
    int pos = 0;
    for (int j = 0; j < gt.G; ++j) {
      const int c = gt.info[j].cls;
      pos += (c < cls || (c == cls && j < i)) ? 1 : 0;
    }
    L.gpos[i] = pos;                                     // < G: a permutation
    L.gsorted[pos] = i;
    const bool always = gt.ignore[i] != 0 || gt.crowd[i] != 0;
    const double area = gt.eval_area[i];
    for (int a = 0; a < gt.A; ++a) L.gig[(size_t)a * gt.G + i] = (always || area < gt.rngs[2 * a] || area > gt.rngs[2 * a + 1]) ? 1 : 0;
  }
}

// grid ceil(dcap * G / 256), block 256.  inter [dcap][G] of the overlap kernel -> iou_out [dcap][G] in the caller's order (may be
// null) and siou [dcap][G] at [dpos[d]][gpos[g]]; rows past the detections' count store 0.0 in iou_out and nothing in siou.
__global__ __launch_bounds__(kMtThreads) void match_iou_kernel(MaskSet D, int dcap, MtGt gt, const long long* __restrict__ inter,
                                                               const int* __restrict__ dpos, const int* __restrict__ gpos,
                                                               double* __restrict__ iou_out, double* __restrict__ siou) {
  const long long p = (long long)blockIdx.x * kMtThreads + threadIdx.x;
  if (p >= (long long)dcap * gt.G) return;
  const int d = (int)(p / gt.G), g = (int)(p % gt.G);
  if (d >= mask_count(D, dcap)) {
    if (iou_out) iou_out[p] = 0.0;
    return;
  }
  const long long in = inter[p];
  const long long uni = gt.crowd[g] ? D.info[d].area : D.info[d].area + gt.info[g].area - in;
  const double iou = uni < 1 ? 0.0 : (double)in / (double)uni;
  if (iou_out) iou_out[p] = iou;
  siou[(long long)dpos[d] * gt.G + gpos[g]] = iou;
}

// grid ceil(dcap * G / 256), block 256.  match_iou_kernel with a second pair of sets: Db / gb_info the boundary bands of the
// detections and of the ground truths, binter their counts.  iou_out and siou receive min(iou, biou), biou_out (may be null) biou.
__global__ __launch_bounds__(kMtThreads) void match_iou_min_kernel(MaskSet D, MaskSet Db, int dcap, MtGt gt, const mnc_mask_info* __restrict__ gb_info,
                                                                   const long long* __restrict__ inter, const long long* __restrict__ binter,
                                                                   const int* __restrict__ dpos, const int* __restrict__ gpos,
                                                                   double* __restrict__ iou_out, double* __restrict__ biou_out,
                                                                   double* __restrict__ siou) {
  const long long p = (long long)blockIdx.x * kMtThreads + threadIdx.x;
  if (p >= (long long)dcap * gt.G) return;
  const int d = (int)(p / gt.G), g = (int)(p % gt.G);
  if (d >= mask_count(D, dcap)) {
    if (iou_out) iou_out[p] = 0.0;
    if (biou_out) biou_out[p] = 0.0;
    return;
  }
  const long long in = inter[p];
  const long long uni = gt.crowd[g] ? D.info[d].area : D.info[d].area + gt.info[g].area - in;
  const double iou = uni < 1 ? 0.0 : (double)in / (double)uni;
  const long long bin = binter[p];
  const long long buni = gt.crowd[g] ? Db.info[d].area : Db.info[d].area + gb_info[g].area - bin;
  const double biou = buni < 1 ? 0.0 : (double)bin / (double)buni;
  const double low = biou < iou ? biou : iou;
  if (iou_out) iou_out[p] = low;
  if (biou_out) biou_out[p] = biou;
  siou[(long long)dpos[d] * gt.G + gpos[g]] = low;
}

__device__ __forceinline__ double mt_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// grid ceil(dcap * A * T / 4), block 256.  Wave (d0, a, t) runs the cell of d0's class when rank[d0] == 0.  dt_match / dt_ignore
// [A][T][dcap], gt_match [A][T][G], filled with -1 / 0 / -1 before the launch.
__global__ __launch_bounds__(kMtThreads) void match_cells_kernel(MaskSet D, int dcap, MtGt gt, MtLists L, const double* __restrict__ siou,
                                                                 int* __restrict__ dt_match, unsigned char* __restrict__ dt_ignore,
                                                                 int* __restrict__ gt_match) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long cell = (long long)blockIdx.x * kMtWaves + wave;
  const int cells = gt.A * gt.T;
  if (cell >= (long long)dcap * cells) return;
  const int d0 = (int)(cell / cells), a = (int)(cell % cells) / gt.T, t = (int)(cell % cells) % gt.T;
  if (d0 >= mask_count(D, dcap) || L.rank[d0] != 0) return;
  const int G = gt.G;
  const int dstart = L.dstart[d0], dn = min(L.dcount[d0], gt.max_det);
  const int gstart = L.gstart[d0], gn = L.gcount[d0];
  const int chunks = (gn + 63) >> 6;                     // <= 32
  const double lo = gt.rngs[2 * a], hi = gt.rngs[2 * a + 1];
  const double thr = fmin(gt.thrs[t], 1.0 - 1e-10);
  // bit c of each word: the state of ground truth 64 c + lane of the class's list
  unsigned ign = 0, crowd = 0, matched = 0;
  for (int c = 0; c < chunks; ++c) {
    const int pos = (c << 6) + lane;
    if (pos < gn) {
      const int g = L.gsorted[gstart + pos];
      ign |= (unsigned)(L.gig[(size_t)a * G + g] != 0) << c;
      crowd |= (unsigned)(gt.crowd[g] != 0) << c;
    }
  }
  int* dm = dt_match + (size_t)(a * gt.T + t) * dcap;
  unsigned char* di = dt_ignore + (size_t)(a * gt.T + t) * dcap;
  int* gm = gt_match + (size_t)(a * gt.T + t) * G;
  const double* col = siou + gstart + lane;              // + row * G + 64 c
  double next = (dn > 0 && lane < gn) ? col[(size_t)dstart * G] : 0.0;
  for (int r = 0; r < dn; ++r) {
    const int row = dstart + r;
    const int d = L.dsorted[row];
    const double area = L.dsarea[row];
    double v = next;
    if (r + 1 < dn && lane < gn) next = col[(size_t)(row + 1) * G];       // the next detection's first chunk, on its way
    double best1 = thr, best2 = thr;
    int m1 = -1, m2 = -1;
    for (int c = 0; c < chunks; ++c) {
      const int pos = (c << 6) + lane;
      const bool valid = pos < gn;
      if (c > 0) v = valid ? col[(size_t)row * G + (c << 6)] : 0.0;
      const bool is_ign = (ign >> c) & 1u, is_crowd = (crowd >> c) & 1u, is_matched = (matched >> c) & 1u;
      const bool reach = valid && v >= thr;
      const bool cand1 = reach && !is_ign && !is_matched;
      if (__ballot(cand1)) {
        const double mx = mt_wave_max(cand1 ? v : -1.0);                   // (an IoU is >= 0)
        if (mx >= best1) {
          best1 = mx;
          m1 = (c << 6) + 63 - __clzll((long long)__ballot(cand1 && v == mx));
        }
      } else if (m1 < 0) {
        const bool cand2 = reach && is_ign && (is_crowd || !is_matched);
        if (__ballot(cand2)) {
          const double mx = mt_wave_max(cand2 ? v : -1.0);
          if (mx >= best2) {
            best2 = mx;
            m2 = (c << 6) + 63 - __clzll((long long)__ballot(cand2 && v == mx));
          }
        }
      }
    }
    const int m = m1 >= 0 ? m1 : m2;                     // a not-ignored ground truth wins over an ignored one of larger IoU
    if (m >= 0) {
      if (lane == (m & 63)) matched |= 1u << (m >> 6);
      if (lane == 0) {
        const int g = L.gsorted[gstart + m];
        dm[d] = g;
        di[d] = m1 >= 0 ? 0 : 1;
        gm[g] = d;
      }
    } else if (lane == 0 && (area < lo || area > hi)) {
      di[d] = 1;
    }
  }
}

namespace {

// The parts of a call every form shares: checked parameters, and the host's tables of the ground truths.
struct MtHost {
  HostMaskSet gt;
  std::vector<unsigned char> crowd, ignore;
  std::vector<double> eval_area;
};

int mt_check(const char* who, const int* g_bounds, const long long* g_offsets, const long long* g_areas, const void* g_bits,
             size_t g_bytes, int ng, const int* g_classes, const unsigned char* g_crowd, const unsigned char* g_ignore,
             const double* g_eval_area, const double* iou_thrs, int T, const double* area_rngs, int A, int max_det, MtHost* h) {
  MNC_REQUIRE(ng >= 0 && ng <= kMtMaxN, "%s: %d ground truths not in [0, %d]", who, ng, kMtMaxN);
  MNC_REQUIRE(T >= 1 && T <= kMtMaxT, "%s: T=%d not in [1, %d]", who, T, kMtMaxT);
  MNC_REQUIRE(A >= 1 && A <= kMtMaxA, "%s: A=%d not in [1, %d]", who, A, kMtMaxA);
  MNC_REQUIRE(max_det >= 1 && max_det <= kMtMaxN, "%s: max_det=%d not in [1, %d]", who, max_det, kMtMaxN);
  MNC_REQUIRE(iou_thrs && area_rngs, "%s: null thresholds or area ranges", who);
  for (int t = 0; t < T; ++t) MNC_REQUIRE(!std::isnan(iou_thrs[t]), "%s: threshold %d is NaN", who, t);
  for (int a = 0; a < A; ++a) {
    MNC_REQUIRE(!std::isnan(area_rngs[2 * a]) && !std::isnan(area_rngs[2 * a + 1]), "%s: a bound of area range %d is NaN", who, a);
    MNC_REQUIRE(area_rngs[2 * a] <= area_rngs[2 * a + 1], "%s: area range %d has lo > hi", who, a);
  }
  MNC_REQUIRE(ng == 0 || (g_classes && g_crowd), "%s: null classes or crowd flags of the ground truths", who);
  h->crowd.assign((size_t)ng, 0);
  h->ignore.assign((size_t)ng, 0);
  h->eval_area.assign((size_t)ng, 0.0);
  for (int g = 0; g < ng; ++g) {
    MNC_REQUIRE(g_crowd[g] <= 1, "%s: crowd flag %d of ground truth %d is not 0 / 1", who, (int)g_crowd[g], g);
    MNC_REQUIRE(!g_ignore || g_ignore[g] <= 1, "%s: ignore flag %d of ground truth %d is not 0 / 1", who, (int)g_ignore[g], g);
    h->crowd[g] = g_crowd[g];
    h->ignore[g] = g_ignore ? g_ignore[g] : 0;
  }
  const int rc = h->gt.check(who, "gt", g_bounds, g_offsets, g_areas, g_bits, g_bytes, ng, g_classes, nullptr);
  if (rc) return rc;
  for (int g = 0; g < ng; ++g) h->eval_area[g] = g_eval_area ? g_eval_area[g] : (double)g_areas[g];
  return MNC_OK;
}

// Device buffers of one call over dcap detections and G ground truths (the ground truths' set takes its place first), and its
// launch sequence.
struct MtWs {
  unsigned char *crowd, *ignore;
  double *eval_area, *thrs, *rngs;
  MtLists L;
  long long* inter;
  double *iou, *siou;
  int *dt_match, *gt_match;
  unsigned char* dt_ignore;
  void layout(WsLayout& l, int dcap, MtHost& h, int G, int T, int A, bool want_iou) {
    const size_t pairs = (size_t)dcap * G, cells = (size_t)A * T;
    h.gt.take(l);
    crowd = l.take<unsigned char>(G);
    ignore = l.take<unsigned char>(G);
    eval_area = l.take<double>(G);
    thrs = l.take<double>(T);
    rngs = l.take<double>(2 * (size_t)A);
    L.rank = l.take<int>(dcap);
    L.dpos = l.take<int>(dcap);
    L.dsorted = l.take<int>(dcap);
    L.dsarea = l.take<double>(dcap);
    L.dstart = l.take<int>(dcap);
    L.dcount = l.take<int>(dcap);
    L.gstart = l.take<int>(dcap);
    L.gcount = l.take<int>(dcap);
    L.gpos = l.take<int>(G);
    L.gsorted = l.take<int>(G);
    L.gig = l.take<unsigned char>((size_t)A * G);
    inter = l.take<long long>(pairs);
    iou = l.take<double>(want_iou ? pairs : 0);
    siou = l.take<double>(pairs);
    dt_match = l.take<int>(cells * dcap);
    dt_ignore = l.take<unsigned char>(cells * dcap);
    gt_match = l.take<int>(cells * G);
  }
};

// What mnc_mask_match_boundary adds to a call: the image, the distance and where the boundary IoU goes on the host (null: not
// wanted) -- its arguments; then the plans and the device buffers of the two boundary sets (their instance tables uploaded by the
// caller), the scratch planes both launches use in turn, the second count table and the boundary IoU's table (null: not wanted).
struct MtBd {
  int H, W, d;
  double* biou_out;
  BdPlan dplan, gplan;
  mnc_mask_info *dinfo, *ginfo;
  u64 *dbits, *gbits, *scratch;
  long long* inter;
  double* biou;
};

// Uploads the ground truths and the parameters, then the passes.  D.info / D.bits are device pointers already.  bd != nullptr:
// the matching runs on min(iou, boundary iou).
int mt_launch(hipStream_t s, const MaskSet& D, int dcap, const MtHost& h, int G, const double* iou_thrs, int T, const double* area_rngs,
              int A, int max_det, bool want_iou, const MtWs& w, const MtBd* bd = nullptr) {
  const size_t cells = (size_t)A * T;
  auto up = [s](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  MNC_HIP_TRY(h.gt.upload(s));
  MNC_HIP_TRY(up(w.crowd, h.crowd.data(), (size_t)G));
  MNC_HIP_TRY(up(w.ignore, h.ignore.data(), (size_t)G));
  MNC_HIP_TRY(up(w.eval_area, h.eval_area.data(), (size_t)G * 8));
  MNC_HIP_TRY(up(w.thrs, iou_thrs, (size_t)T * 8));
  MNC_HIP_TRY(up(w.rngs, area_rngs, (size_t)A * 16));
  if (cells * dcap) {
    MNC_HIP_TRY(hipMemsetAsync(w.dt_match, 0xff, cells * dcap * 4, s));
    MNC_HIP_TRY(hipMemsetAsync(w.dt_ignore, 0, cells * dcap, s));
  }
  if (cells * G) MNC_HIP_TRY(hipMemsetAsync(w.gt_match, 0xff, cells * G * 4, s));
  const MtGt gt = {h.gt.d_info, w.crowd, w.ignore, w.eval_area, w.thrs, w.rngs, G, T, A, max_det};
  const int n = dcap > G ? dcap : G;
  if (n < 1) return MNC_OK;
  hipLaunchKernelGGL(match_lists_kernel, dim3(cdiv(n, kMtThreads)), dim3(kMtThreads), 0, s, D, dcap, gt, w.L);
  const long long pairs = (long long)dcap * G;
  if (pairs > 0) {
    const MaskSet B = h.gt.view();
    overlaps_launch(s, D, B, nullptr, 0, dcap, G, w.inter, nullptr);
    if (!bd) {
      hipLaunchKernelGGL(match_iou_kernel, dim3((unsigned)((pairs + kMtThreads - 1) / kMtThreads)), dim3(kMtThreads), 0, s, D, dcap, gt,
                         w.inter, w.L.dpos, w.L.gpos, want_iou ? w.iou : nullptr, w.siou);
    } else {
      // the two boundary sets, one after the other through the same scratch planes, then their counts
      boundary_launch(s, D, bd->H, bd->W, bd->d, bd->dplan, bd->dinfo, bd->dbits, bd->scratch);
      boundary_launch(s, B, bd->H, bd->W, bd->d, bd->gplan, bd->ginfo, bd->gbits, bd->scratch);
      const MaskSet Db = {bd->dinfo, bd->dbits, nullptr, dcap}, Gb = {bd->ginfo, bd->gbits, nullptr, G};
      overlaps_launch(s, Db, Gb, nullptr, 0, dcap, G, bd->inter, nullptr);
      hipLaunchKernelGGL(match_iou_min_kernel, dim3((unsigned)((pairs + kMtThreads - 1) / kMtThreads)), dim3(kMtThreads), 0, s, D, Db,
                         dcap, gt, bd->ginfo, w.inter, bd->inter, w.L.dpos, w.L.gpos, want_iou ? w.iou : nullptr, bd->biou, w.siou);
    }
  }
  if (dcap > 0)
    hipLaunchKernelGGL(match_cells_kernel, dim3((unsigned)(((long long)dcap * cells + kMtWaves - 1) / kMtWaves)), dim3(kMtThreads), 0, s,
                       D, dcap, gt, w.L, w.siou, w.dt_match, w.dt_ignore, w.gt_match);
  return MNC_OK;
}

// nd == 0 or ng == 0: nothing can match -- the ranks, the ground truths' flags and the size rule of the unmatched, on the host.
void mt_nothing(const MtHost& h, int nd, const int* dt_classes, const float* dt_scores, const long long* dt_areas, int ng, int T,
                const double* area_rngs, int A, int max_det, int* rank, int* dt_match, unsigned char* dt_ignore, int* gt_match,
                unsigned char* gt_ignore) {
  for (int d = 0; d < nd; ++d) {
    int r = 0;
    for (int j = 0; j < nd; ++j) {
      const float sj = dt_scores[j], sd = dt_scores[d];
      r += (dt_classes[j] == dt_classes[d] && (sj > sd || (sj == sd && j < d))) ? 1 : 0;
    }
    rank[d] = r;
  }
  for (int a = 0; a < A; ++a) {
    const double lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
    for (int g = 0; g < ng; ++g)
      gt_ignore[(size_t)a * ng + g] = (h.ignore[g] || h.crowd[g] || h.eval_area[g] < lo || h.eval_area[g] > hi) ? 1 : 0;
    for (int t = 0; t < T; ++t) {
      for (int g = 0; g < ng; ++g) gt_match[((size_t)a * T + t) * ng + g] = -1;
      for (int d = 0; d < nd; ++d) {
        const double area = (double)dt_areas[d];
        dt_match[((size_t)a * T + t) * nd + d] = -1;
        dt_ignore[((size_t)a * T + t) * nd + d] = (rank[d] < max_det && (area < lo || area > hi)) ? 1 : 0;
      }
    }
  }
}

// mnc_mask_match (bd == nullptr) and mnc_mask_match_boundary (bd: H, W, d and biou_out filled in), which differ in the boundary
// part alone.
int mt_host(const char* who, const int* dt_bounds, const long long* dt_offsets, const long long* dt_areas, const void* dt_bits,
            size_t dt_bytes, int nd, const int* dt_classes, const float* dt_scores, const int* gt_bounds, const long long* gt_offsets,
            const long long* gt_areas, const void* gt_bits, size_t gt_bytes, int ng, const int* gt_classes,
            const unsigned char* gt_crowd, const unsigned char* gt_ignore_in, const double* gt_eval_area, const double* iou_thrs, int T,
            const double* area_rngs, int A, int max_det, MtBd* bd, int* rank, int* dt_match, unsigned char* dt_ignore, int* gt_match,
            unsigned char* gt_ignore, double* iou, int device_id) {
  MNC_REQUIRE(nd >= 0 && nd <= kMtMaxN, "%s: %d detections not in [0, %d]", who, nd, kMtMaxN);
  MNC_REQUIRE(rank && dt_match && dt_ignore && gt_match && gt_ignore, "%s: null output pointer", who);
  MNC_REQUIRE(nd == 0 || (dt_classes && dt_scores), "%s: null classes or scores of the detections", who);
  for (int k = 0; k < nd; ++k) MNC_REQUIRE(!std::isnan(dt_scores[k]), "%s: score %d is NaN", who, k);
  int rc = bd ? boundary_check_image(who, bd->H, bd->W, bd->d) : MNC_OK;
  if (rc) return rc;
  MtHost h;
  rc = mt_check(who, gt_bounds, gt_offsets, gt_areas, gt_bits, gt_bytes, ng, gt_classes, gt_crowd, gt_ignore_in, gt_eval_area,
                iou_thrs, T, area_rngs, A, max_det, &h);
  if (rc) return rc;
  HostMaskSet dt;
  rc = dt.check(who, "dt", dt_bounds, dt_offsets, dt_areas, dt_bits, dt_bytes, nd, dt_classes, dt_scores);
  if (rc) return rc;
  const size_t cells = (size_t)A * T, pairs = (size_t)nd * ng;
  if (nd == 0 || ng == 0) {                              // (no pair: no IoU table has an entry)
    mt_nothing(h, nd, dt_classes, dt_scores, dt_areas, ng, T, area_rngs, A, max_det, rank, dt_match, dt_ignore, gt_match, gt_ignore);
    clear_error();
    return MNC_OK;
  }
  // the boundary sets' instance tables follow from the bounds alone
  std::vector<mnc_mask_info> dbinfo, gbinfo;
  if (bd) {
    boundary_plan(dt.info, bd->H, bd->W, bd->d, &dbinfo, &bd->dplan);
    boundary_plan(h.gt.info, bd->H, bd->W, bd->d, &gbinfo, &bd->gplan);
  }
  MtWs w;
  auto layout = [&](WsLayout l) {
    dt.take(l);
    w.layout(l, nd, h, ng, T, A, iou != nullptr);
    if (bd) {
      const size_t plane = bd->dplan.bytes > bd->gplan.bytes ? bd->dplan.bytes : bd->gplan.bytes;
      bd->dinfo = l.take<mnc_mask_info>(nd);
      bd->ginfo = l.take<mnc_mask_info>(ng);
      bd->dbits = l.take<u64>(bd->dplan.bytes / 8);
      bd->gbits = l.take<u64>(bd->gplan.bytes / 8);
      bd->scratch = l.take<u64>(plane / 8 * bd->dplan.planes);
      bd->inter = l.take<long long>(pairs);
      bd->biou = l.take<double>(bd->biou_out ? pairs : 0);
    }
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(dt.upload(hs));
  TimedSpan span(g_bd_timer);                            // (never begun without the boundary part)
  if (bd) {
    if (!bd->biou_out) bd->biou = nullptr;
    MNC_HIP_TRY(hs.up(bd->dinfo, dbinfo.data(), (size_t)nd * sizeof(mnc_mask_info)));
    MNC_HIP_TRY(hs.up(bd->ginfo, gbinfo.data(), (size_t)ng * sizeof(mnc_mask_info)));
    span.begin(hs.stream);
  }
  rc = mt_launch(hs.stream, dt.view(), nd, h, ng, iou_thrs, T, area_rngs, A, max_det, iou != nullptr, w, bd);
  if (rc) return rc;
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(rank, w.L.rank, (size_t)nd * 4));
  MNC_HIP_TRY(hs.down(dt_match, w.dt_match, cells * nd * 4));
  MNC_HIP_TRY(hs.down(dt_ignore, w.dt_ignore, cells * nd));
  MNC_HIP_TRY(hs.down(gt_match, w.gt_match, cells * ng * 4));
  MNC_HIP_TRY(hs.down(gt_ignore, w.L.gig, (size_t)A * ng));
  if (iou) MNC_HIP_TRY(hs.down(iou, w.iou, pairs * 8));
  if (bd && bd->biou_out) MNC_HIP_TRY(hs.down(bd->biou_out, bd->biou, pairs * 8));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mask_match(const int* dt_bounds, const long long* dt_offsets, const long long* dt_areas, const void* dt_bits, size_t dt_bytes,
                   int nd, const int* dt_classes, const float* dt_scores, const int* gt_bounds, const long long* gt_offsets,
                   const long long* gt_areas, const void* gt_bits, size_t gt_bytes, int ng, const int* gt_classes,
                   const unsigned char* gt_crowd, const unsigned char* gt_ignore_in, const double* gt_eval_area, const double* iou_thrs,
                   int T, const double* area_rngs, int A, int max_det, int* rank, int* dt_match, unsigned char* dt_ignore,
                   int* gt_match, unsigned char* gt_ignore, double* iou, int device_id) {
  return mt_host("mnc_mask_match", dt_bounds, dt_offsets, dt_areas, dt_bits, dt_bytes, nd, dt_classes, dt_scores, gt_bounds, gt_offsets,
                 gt_areas, gt_bits, gt_bytes, ng, gt_classes, gt_crowd, gt_ignore_in, gt_eval_area, iou_thrs, T, area_rngs, A, max_det,
                 nullptr, rank, dt_match, dt_ignore, gt_match, gt_ignore, iou, device_id);
}

// see include/mnc_hip.h
int mnc_mask_match_boundary(const int* dt_bounds, const long long* dt_offsets, const long long* dt_areas, const void* dt_bits,
                            size_t dt_bytes, int nd, const int* dt_classes, const float* dt_scores, const int* gt_bounds,
                            const long long* gt_offsets, const long long* gt_areas, const void* gt_bits, size_t gt_bytes, int ng,
                            const int* gt_classes, const unsigned char* gt_crowd, const unsigned char* gt_ignore_in,
                            const double* gt_eval_area, const double* iou_thrs, int T, const double* area_rngs, int A, int max_det,
                            int H, int W, int d, int* rank, int* dt_match, unsigned char* dt_ignore, int* gt_match,
                            unsigned char* gt_ignore, double* iou, double* biou, int device_id) {
  MtBd bd;
  bd.H = H; bd.W = W; bd.d = d;
  bd.biou_out = biou;
  return mt_host("mnc_mask_match_boundary", dt_bounds, dt_offsets, dt_areas, dt_bits, dt_bytes, nd, dt_classes, dt_scores, gt_bounds,
                 gt_offsets, gt_areas, gt_bits, gt_bytes, ng, gt_classes, gt_crowd, gt_ignore_in, gt_eval_area, iou_thrs, T, area_rngs, A,
                 max_det, &bd, rank, dt_match, dt_ignore, gt_match, gt_ignore, iou, device_id);
}

// see include/mnc_hip.h
int mnc_mask_match_dev(mnc_ctx* ctx, const void* d_info, const void* d_bits, int rows_cap, const int* gt_bounds,
                       const long long* gt_offsets, const long long* gt_areas, const void* gt_bits, size_t gt_bytes, int ng,
                       const int* gt_classes, const unsigned char* gt_crowd, const unsigned char* gt_ignore_in,
                       const double* gt_eval_area, const double* iou_thrs, int T, const double* area_rngs, int A, int max_det,
                       int want_iou, void** d_rank, void** d_dt_match, void** d_dt_ignore, void** d_gt_match, void** d_gt_ignore,
                       void** d_iou) {
  const char* who = "mnc_mask_match_dev";
  MNC_REQUIRE(ctx, "%s: null context", who);
  MNC_REQUIRE(d_rank && d_dt_match && d_dt_ignore && d_gt_match && d_gt_ignore, "%s: null output pointer", who);
  MNC_REQUIRE(want_iou == 0 || (want_iou == 1 && d_iou), "%s: want_iou=%d is not 0 / 1, or d_iou is null", who, want_iou);
  MNC_REQUIRE(rows_cap >= 0 && rows_cap <= kMtMaxN, "%s: rows_cap=%d not in [0, %d]", who, rows_cap, kMtMaxN);
  MtHost h;
  int rc = mt_check(who, gt_bounds, gt_offsets, gt_areas, gt_bits, gt_bytes, ng, gt_classes, gt_crowd, gt_ignore_in, gt_eval_area,
                    iou_thrs, T, area_rngs, A, max_det, &h);
  if (rc) return rc;
  MNC_REQUIRE(rows_cap == 0 || (d_info && d_bits), "%s: null device pointer", who);
  MNC_NO_CAPTURE(ctx, who);
  MtWs w;
  auto layout = [&](WsLayout l) {
    w.layout(l, rows_cap, h, ng, T, A, want_iou != 0);
    return l.bytes();
  };
  // an arena of its own: mask_ws holds the masks this call reads, overlap_ws somebody's matrices.  In no captured graph.
  rc = arena_ensure(&ctx->match_ws, layout(WsLayout()), 0, "mask-match buffers", ctx->stream, ctx);
  if (rc) return rc;
  layout(WsLayout(ctx->match_ws.p));
  LaunchScope ls(ctx, "mask_match");
  hipStream_t s = ctx->stream;
  rc = mt_launch(s, MaskSet::of_records(d_info, d_bits, rows_cap), rows_cap, h, ng, iou_thrs, T, area_rngs, A, max_det, want_iou != 0, w);
  if (rc) return rc;
  rc = ls.finish("mask_match");
  if (rc) return rc;
  *d_rank = w.L.rank;
  *d_dt_match = w.dt_match;
  *d_dt_ignore = w.dt_ignore;
  *d_gt_match = w.gt_match;
  *d_gt_ignore = w.L.gig;
  if (d_iou) *d_iou = want_iou ? w.iou : nullptr;
  clear_error();
  return MNC_OK;
}
