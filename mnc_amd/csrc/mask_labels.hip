// Label maps in and out of packed instance masks (include/mnc_hip.h n19), for gfx950, on the PackedMasks layout of inst_masks.hip
// (n5): the instance table of an integer label map (mnc_label_table), the bits of its instances (mnc_label_masks), and the label
// map of a set of packed masks (mnc_mask_to_labels).  The statements of the rules are mnc_amd/labels.py:from_labels_numpy and
// to_labels_numpy; this file computes the same tables, words and maps exactly.  All arithmetic is integer.
//
// mnc_label_table, one pass over the map per step and six launches whatever the data (lb_presence_kernel, lb_count_kernel, lb_rank
// and lb_ids_kernel are label_bits.h's, shared with label_pairs.hip):
//   lb_presence_kernel   a lane owns kLbRun consecutive pixels of the flat map (one 16-byte load); a value's bit is ORed into a
//                        presence bitmap of 32-bit words sized to the largest id once per change of value inside the lanes' runs,
//                        by one lane of the wave for all that have the value, and only where a relaxed look does not show the
//                        bit yet (a stale look costs one more atomic, never a bit).
//   lb_count_kernel      a lane per bitmap word: the skip values cleared, the word stored back, its popcount stored.
//   scan_launch          (scan.h, two launches) the exclusive prefix of the popcounts: the rank of an id is the prefix of its word
//                        plus the set bits below it.  At most 2^19 words (ids below 2^24), 512 scan tiles, a total below 2^24.
//   lb_stats_kernel      the map again, the same runs cut at row ends: per run the rank, then integer atomicMin / atomicMax into the
//                        box, atomicAdd into the area, min / max of cls.  The lanes of a wave whose pixels continue one run join it
//                        by shuffles first, so a run costs one set of atomics per wave it crosses; a min / max atomic is issued
//                        only where a relaxed look shows that it would change the word.
//   lb_ids_kernel        a lane per bitmap word writes the ids of its set bits at their ranks.
// mnc_label_masks, one launch over the zeroed output: a wave owns 64 consecutive pixels of a row; while lanes remain it takes the
// first remaining lane's value, ballots the lanes that equal it, finds the value by binary search in the table (at most 11 turns)
// and ORs the ballot, shifted by the instance's x1, into the one or two destination words with a 64-bit atomicOr.  OR commutes:
// the bytes do not depend on the order of arrival.  The map is read once however many boxes cover a pixel (a superpixel map is
// covered many times over).  A value that is not in the table, a row outside the instance's box and a word outside its row are
// skipped, bits past its width are masked: whatever the map and the table hold, nothing is written outside the rows.
// mnc_mask_to_labels, one launch, no atomics: a wave owns one 64-pixel strip of a row, tests the bounds of 64 instances at a time
// in painting order, one per lane, ballots those that meet the strip and walks them in order with mask_read and a `taken` mask --
// lane l keeps the value of the first instance that has its bit -- and leaves when every in-image bit is taken.  Every pixel is
// stored exactly once, background included.
//
// Bound: latency and same-address atomics.  On the map of the 98 best instances of a 600 x 1000 image the table's six launches take
// 189 us, nearly all of it lb_stats_kernel's atomics on the few words of the instances; the masks' launch takes 20 us, the painting
// 12 us.  The calls with their copies take 0.71, 0.11 and 0.15 ms: the host's walk over the 2.4 MB map, its upload (0.053 ms) and
// the read-backs (profiles/mask_labels_bench.txt).  6 to 22 VGPRs, no LDS and no scratch in any kernel.
#include <algorithm>
#include <climits>
#include <vector>

#include "label_bits.h"
#include "mask_tight.h"

namespace mnc {

// One instance of mnc_label_masks: its value, its box, the words of a row and its first word in the output.
struct LbInst {
  int id, x1, y1, x2, y2, strips;
  long long first;
};

// One step of the painting order of mnc_mask_to_labels.
struct LbSeq {
  int idx, value;
};

struct LbStats {
  int* box;      // [cap][4], (INT_MAX, INT_MAX, INT_MIN, INT_MIN) before
  u64* area;     // [cap], 0 before
  int* clo;      // [cap], INT_MAX before
  int* chi;      // [cap], INT_MIN before
};

// One run of value-rank k in row y, columns x1 .. x2: the box by atomics only where a look shows that it grows, the area by one.
__device__ __forceinline__ void lb_join(const LbStats& st, bool with_cls, int k, int x1, int x2, int y, int clo, int chi) {
  int* b = st.box + 4 * k;
  if (lb_peek(b) > x1) atomicMin(b, x1);
  if (lb_peek(b + 1) > y) atomicMin(b + 1, y);
  if (lb_peek(b + 2) < x2) atomicMax(b + 2, x2);
  if (lb_peek(b + 3) < y) atomicMax(b + 3, y);
  atomicAdd(st.area + k, (u64)(x2 - x1 + 1));
  if (with_cls) {
    if (lb_peek(st.clo + k) > clo) atomicMin(st.clo + k, clo);
    if (lb_peek(st.chi + k) < chi) atomicMax(st.chi + k, chi);
  }
}

// grid ceil(total / 1024), block 256.  Ranks at or past cap are dropped: the host refuses such a map from the count alone.
__global__ __launch_bounds__(kLbThreads) void lb_stats_kernel(const int* __restrict__ label, const int* __restrict__ cls, int W,
                                                              long long total, const unsigned* __restrict__ present, int words,
                                                              Scanned pre, int cap, LbStats st) {
  const long long p = ((long long)blockIdx.x * kLbThreads + threadIdx.x) * kLbRun;
  const bool live = p < total;
  int v[kLbRun] = {0, 0, 0, 0}, c[kLbRun] = {0, 0, 0, 0};
  int count = 0;
  if (live) {
    count = lb_load(label, p, total, v[0], v[1], v[2], v[3]);
    if (cls) lb_load(cls, p, total, c[0], c[1], c[2], c[3]);
  }
  const int y0 = live ? (int)(p / W) : 0;
  int x = live ? (int)(p - (long long)y0 * W) : 0, y = y0;
  // The last run of a lane is held back: a lane that is one run joins the last run of the lane before it when value and row are
  // the same (their pixels are consecutive), and the first lane of such a segment -- its head -- issues the atomics for all of it.
  int rv = v[0], rx1 = x, ry = y, rlen = 0, rclo = INT_MAX, rchi = INT_MIN, runs = 0;
#pragma unroll
  for (int e = 0; e < kLbRun; ++e) {
    if (e >= count) continue;
    if (e > 0 && (v[e] != rv || x == 0)) {
      const int k = lb_rank(present, words, pre, rv);
      if (k >= 0 && k < cap) lb_join(st, cls != nullptr, k, rx1, rx1 + rlen - 1, ry, rclo, rchi);
      rv = v[e]; rx1 = x; ry = y; rlen = 0; rclo = INT_MAX; rchi = INT_MIN;
      ++runs;
    }
    ++rlen;
    rclo = min(rclo, c[e]);
    rchi = max(rchi, c[e]);
    if (++x == W) { x = 0; ++y; }
  }
  const int lane = threadIdx.x & 63;
  const int pv = __shfl_up(rv, 1), py = __shfl_up(ry, 1), plive = __shfl_up((int)live, 1);
  const bool joins = live && runs == 0 && lane > 0 && plive && pv == rv && py == ry;
  const u64 alive = __ballot(live), heads = __ballot(live && !joins);
  if (alive == 0ull) return;                               // (the whole wave)
  // the last lane of this lane's segment: the one before the next head, or the last live lane
  const u64 after = heads & ~((2ull << lane) - 1ull);
  const int last = after ? __ffsll((long long)after) - 2 : 63 - __clzll((long long)alive);
  if (cls) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int tlo = __shfl_down(rclo, s), thi = __shfl_down(rchi, s);
      if (lane + s <= last) {
        rclo = min(rclo, tlo);
        rchi = max(rchi, thi);
      }
    }
  }
  const int rx2 = __shfl(rx1 + rlen - 1, min(max(last, 0), 63));
  if (live && !joins) {
    const int k = lb_rank(present, words, pre, rv);
    if (k >= 0 && k < cap) lb_join(st, cls != nullptr, k, rx1, rx2, ry, rclo, rchi);
  }
}

// grid ceil(H * strips / 4), block 256: a wave per 64-pixel strip of a row.  out is zero before.
__global__ __launch_bounds__(kLbThreads) void lb_masks_kernel(const int* __restrict__ label, int H, int W, int strips,
                                                              const LbInst* __restrict__ tab, int n, u64* out) {
  const long long wave = ((long long)blockIdx.x * kLbThreads + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= (long long)H * strips) return;               // (the whole wave)
  const int y = (int)(wave / strips), x0 = (int)(wave - (long long)y * strips) * 64;
  const bool active = x0 + lane < W;
  const int v = active ? label[(long long)y * W + x0 + lane] : -1;
  u64 rest = __ballot(active);
  while (rest) {
    const int lv = __shfl(v, __ffsll((long long)rest) - 1);
    const u64 same = __ballot(active && v == lv);
    rest &= ~same;
    int lo = 0, hi = n - 1;
    for (int turn = 0; turn < 12 && lo < hi; ++turn) {
      const int mid = (lo + hi) >> 1;
      if (tab[mid].id < lv) lo = mid + 1; else hi = mid;
    }
    const LbInst t = tab[lo];
    const int r = x0 - t.x1, s = r & 63, q = (r >> 6) + lane;  // (floor division: r may be negative)
    u64 b = lane == 0 ? same << s : (lane == 1 && s ? same >> (64 - s) : 0ull);
    const bool inside = t.id == lv && y >= t.y1 && y <= t.y2 && q >= 0 && q < t.strips;
    const int valid = t.x2 - t.x1 + 1 - q * 64;
    if (inside && valid < 64) b &= (1ull << valid) - 1ull;
    if (inside && b) atomicOr(out + t.first + (long long)(y - t.y1) * t.strips + q, b);
  }
}

// grid ceil(H * strips / 4), block 256: a wave per 64-pixel strip of a row.
__global__ __launch_bounds__(kLbThreads) void lb_paint_kernel(MaskSet A, const LbSeq* __restrict__ seq, int n, int background, int H,
                                                              int W, int strips, int* __restrict__ out) {
  const long long wave = ((long long)blockIdx.x * kLbThreads + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= (long long)H * strips) return;               // (the whole wave)
  const int y = (int)(wave / strips), x0 = (int)(wave - (long long)y * strips) * 64;
  const u64 inimg = W - x0 >= 64 ? ~0ull : (1ull << (W - x0)) - 1ull;
  u64 taken = 0ull;
  int mine = background;
  for (int base = 0; base < n && taken != inimg; base += 64) {
    bool hit = false;
    if (base + lane < n) {
      const mnc_mask_info& m = A.info[seq[base + lane].idx];
      hit = mask_has_rows(m) && y >= m.y1 && y <= m.y2 && m.x1 <= x0 + 63 && m.x2 >= x0;
    }
    u64 hits = __ballot(hit);
    while (hits && taken != inimg) {
      const LbSeq s = seq[base + __ffsll((long long)hits) - 1];
      hits &= hits - 1ull;
      const u64 word = mask_read(A.info[s.idx], A.bits, x0, y) & inimg & ~taken;
      if ((word >> lane) & 1ull) mine = s.value;
      taken |= word;
    }
  }
  if (x0 + lane < W) out[(long long)y * W + x0 + lane] = mine;
}

namespace {

CallTimer g_lb_timer;

int lb_check_image(const char* who, int H, int W) {
  MNC_REQUIRE(H >= 1 && H <= kLbMaxSide && W >= 1 && W <= kLbMaxSide, "%s: H=%d or W=%d not in [1, %d]", who, H, W, kLbMaxSide);
  MNC_REQUIRE((long long)H * W <= kLbMaxPixels, "%s: %lld pixels (limit %lld)", who, (long long)H * W, kLbMaxPixels);
  return MNC_OK;
}

unsigned lb_blocks(long long units) { return (unsigned)((units + kLbThreads - 1) / kLbThreads); }

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_label_table(const int* label, const int* cls, int H, int W, const int* skip, int n_skip, int cap, int* n, int* ids, int* bounds,
                    long long* areas, int* cls_lo, int* cls_hi, size_t* bits_bytes, int device_id) {
  const char* who = "mnc_label_table";
  MNC_REQUIRE(label && n && bits_bytes, "%s: null pointer", who);
  MNC_REQUIRE(n_skip >= 0 && n_skip <= kLbMaxSkip && (n_skip == 0 || skip), "%s: n_skip=%d not in [0, %d], or null skip", who, n_skip,
              kLbMaxSkip);
  MNC_REQUIRE(cap >= 0 && (cap == 0 || (ids && bounds && areas && cls_lo && cls_hi)), "%s: cap=%d is negative, or a null output", who,
              cap);
  int rc = lb_check_image(who, H, W);
  if (rc) return rc;
  const long long total = (long long)H * W;
  int top = 0;
  for (long long p = 0; p < total; ++p) {
    MNC_REQUIRE(label[p] >= 0 && label[p] < kLbMaxId, "%s: label[%lld][%lld]=%d not in [0, %d)", who, p / W, p % W, label[p], kLbMaxId);
    top = std::max(top, label[p]);
  }
  const int words = (top >> 5) + 1, limit = std::min(cap, kTightMaxN);
  static_assert(kLbMaxId / 32 == kLbMaxWords, "the bitmap of the largest id");
  LbSkip sk;
  sk.n = n_skip;
  for (int k = 0; k < kLbMaxSkip; ++k) sk.v[k] = k < n_skip ? skip[k] : -1;
  int *d_label, *d_cls, *d_cnt, *d_tile, *d_ids;
  unsigned* d_present;
  LbStats st;
  auto layout = [&](WsLayout l) {
    d_label = l.take<int>((size_t)total);
    d_cls = l.take<int>(cls ? (size_t)total : 0);
    d_present = l.take<unsigned>(words);
    d_cnt = l.take<int>(words);
    d_tile = l.take<int>((size_t)scan_tiles(words) + 1);
    d_ids = l.take<int>(kTightMaxN);
    st.box = l.take<int>(4 * (size_t)kTightMaxN);
    st.area = l.take<u64>(kTightMaxN);
    st.clo = l.take<int>(kTightMaxN);
    st.chi = l.take<int>(kTightMaxN);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  std::vector<int> box(4 * (size_t)kTightMaxN), h_ids(kTightMaxN, 0), clo(kTightMaxN, INT_MAX), chi(kTightMaxN, INT_MIN);
  for (int k = 0; k < kTightMaxN; ++k) {
    box[4 * k] = box[4 * k + 1] = INT_MAX;
    box[4 * k + 2] = box[4 * k + 3] = INT_MIN;
  }
  std::vector<u64> area(kTightMaxN, 0ull);
  MNC_HIP_TRY(hs.up(d_label, label, (size_t)total * sizeof(int)));
  if (cls) MNC_HIP_TRY(hs.up(d_cls, cls, (size_t)total * sizeof(int)));
  MNC_HIP_TRY(hs.up(st.box, box.data(), box.size() * sizeof(int)));
  MNC_HIP_TRY(hs.up(st.area, area.data(), area.size() * sizeof(u64)));
  MNC_HIP_TRY(hs.up(st.clo, clo.data(), clo.size() * sizeof(int)));
  MNC_HIP_TRY(hs.up(st.chi, chi.data(), chi.size() * sizeof(int)));
  MNC_HIP_TRY(hipMemsetAsync(d_present, 0, (size_t)words * sizeof(unsigned), hs.stream));
  TimedSpan span(g_lb_timer);
  span.begin(hs.stream);
  const unsigned px_blocks = lb_blocks((total + kLbRun - 1) / kLbRun);
  hipLaunchKernelGGL(lb_presence_kernel, dim3(px_blocks), dim3(kLbThreads), 0, hs.stream, d_label, total, words, d_present, nullptr);
  hipLaunchKernelGGL(lb_count_kernel, dim3(lb_blocks(words)), dim3(kLbThreads), 0, hs.stream, d_present, words, sk, d_cnt);
  const Scanned pre = scan_launch(hs.stream, d_cnt, words, d_tile);
  hipLaunchKernelGGL(lb_stats_kernel, dim3(px_blocks), dim3(kLbThreads), 0, hs.stream, d_label, cls ? d_cls : nullptr, W, total,
                     d_present, words, pre, kTightMaxN, st);
  hipLaunchKernelGGL(lb_ids_kernel, dim3(lb_blocks(words)), dim3(kLbThreads), 0, hs.stream, d_present, words, pre, kTightMaxN, d_ids);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  int found = 0;
  MNC_HIP_TRY(hs.down(&found, d_tile + pre.tiles, sizeof(int)));
  MNC_HIP_TRY(hs.down(h_ids.data(), d_ids, h_ids.size() * sizeof(int)));
  MNC_HIP_TRY(hs.down(box.data(), st.box, box.size() * sizeof(int)));
  MNC_HIP_TRY(hs.down(area.data(), st.area, area.size() * sizeof(u64)));
  if (cls) {
    MNC_HIP_TRY(hs.down(clo.data(), st.clo, clo.size() * sizeof(int)));
    MNC_HIP_TRY(hs.down(chi.data(), st.chi, chi.size() * sizeof(int)));
  }
  MNC_HIP_TRY(hs.sync());
  span.keep();
  *n = found;
  MNC_REQUIRE(found <= limit, "%s: the map has %d instances (cap %d, limit %d)", who, found, cap, kTightMaxN);
  long long at = 0;
  for (int k = 0; k < found; ++k) {
    ids[k] = h_ids[k];
    for (int e = 0; e < 4; ++e) bounds[4 * (size_t)k + e] = box[4 * (size_t)k + e];
    areas[k] = (long long)area[k];
    cls_lo[k] = cls ? clo[k] : 0;
    cls_hi[k] = cls ? chi[k] : 0;
    at += mask_bytes(box[4 * k + 2] - box[4 * k] + 1, box[4 * k + 3] - box[4 * k + 1] + 1);
  }
  *bits_bytes = (size_t)at;
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_label_masks(const int* label, int H, int W, const int* ids, const int* bounds, int n, void* out_bits, size_t bits_cap,
                    size_t* bits_bytes, int device_id) {
  const char* who = "mnc_label_masks";
  MNC_REQUIRE(label && bits_bytes, "%s: null pointer", who);
  MNC_REQUIRE(n >= 0 && n <= kTightMaxN, "%s: n=%d not in [0, %d]", who, n, kTightMaxN);
  MNC_REQUIRE(n == 0 || (ids && bounds), "%s: null table", who);
  int rc = lb_check_image(who, H, W);
  if (rc) return rc;
  std::vector<LbInst> tab((size_t)n);
  long long at = 0;
  for (int i = 0; i < n; ++i) {
    const int* q = bounds + 4 * (size_t)i;
    MNC_REQUIRE(ids[i] >= 0 && ids[i] < kLbMaxId && (i == 0 || ids[i] > ids[i - 1]), "%s: ids[%d]=%d is out of range or not ascending",
                who, i, ids[i]);
    MNC_REQUIRE(q[0] >= 0 && q[0] <= q[2] && q[2] < W && q[1] >= 0 && q[1] <= q[3] && q[3] < H,
                "%s: bounds[%d] = (%d, %d, %d, %d) is empty or leaves the %d x %d image", who, i, q[0], q[1], q[2], q[3], H, W);
    tab[i] = LbInst{ids[i], q[0], q[1], q[2], q[3], mask_strips(q[2] - q[0] + 1), at / 8};
    at += mask_bytes(q[2] - q[0] + 1, q[3] - q[1] + 1);
  }
  MNC_REQUIRE(n == 0 || out_bits, "%s: null out_bits", who);
  MNC_REQUIRE(bits_cap >= (size_t)at, "%s: bits_cap %zu is below the %lld bytes of the boxes", who, bits_cap, at);
  *bits_bytes = (size_t)at;
  if (n == 0) { clear_error(); return MNC_OK; }
  const long long total = (long long)H * W;
  const int strips = mask_strips(W);
  int* d_label; LbInst* d_tab; u64* d_out;
  auto layout = [&](WsLayout l) {
    d_label = l.take<int>((size_t)total);
    d_tab = l.take<LbInst>(n);
    d_out = l.take<u64>((size_t)(at / 8));
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(hs.up(d_label, label, (size_t)total * sizeof(int)));
  MNC_HIP_TRY(hs.up(d_tab, tab.data(), tab.size() * sizeof(LbInst)));
  MNC_HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)at, hs.stream));
  TimedSpan span(g_lb_timer);
  span.begin(hs.stream);
  hipLaunchKernelGGL(lb_masks_kernel, dim3(lb_blocks((long long)H * strips * 64)), dim3(kLbThreads), 0, hs.stream, d_label, H, W, strips,
                     d_tab, n, d_out);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(out_bits, d_out, (size_t)at));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_to_labels(const int* bounds, const long long* offsets, const void* bits, size_t bytes, int n, const float* scores,
                       const int* order, const int* values, int background, int H, int W, int* out, int device_id) {
  const char* who = "mnc_mask_to_labels";
  MNC_REQUIRE(out, "%s: null out", who);
  MNC_REQUIRE(n >= 0 && n <= kTightMaxN, "%s: n=%d not in [0, %d]", who, n, kTightMaxN);
  MNC_REQUIRE(n == 0 || order || scores, "%s: neither order nor scores", who);
  int rc = lb_check_image(who, H, W);
  if (rc) return rc;
  HostMaskSet A;
  rc = A.check(who, "masks", bounds, offsets, bits, bytes, n, nullptr, nullptr);
  if (rc) return rc;
  std::vector<LbSeq> seq((size_t)n);
  if (order) {
    std::vector<char> seen((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
      MNC_REQUIRE(order[k] >= 0 && order[k] < n && !seen[order[k]], "%s: order is not a permutation at %d", who, k);
      seen[order[k]] = 1;
      seq[k].idx = order[k];
    }
  } else {
    std::vector<int> by((size_t)n);
    for (int i = 0; i < n; ++i) {
      MNC_REQUIRE(scores[i] == scores[i], "%s: scores[%d] is NaN", who, i);
      by[i] = i;
    }
    std::stable_sort(by.begin(), by.end(), [&](int p, int q) { return scores[p] > scores[q]; });
    for (int k = 0; k < n; ++k) seq[k].idx = by[k];
  }
  for (int k = 0; k < n; ++k) seq[k].value = values ? values[seq[k].idx] : seq[k].idx + 1;
  const long long total = (long long)H * W;
  if (n == 0) {
    std::fill(out, out + total, background);
    clear_error();
    return MNC_OK;
  }
  const int strips = mask_strips(W);
  LbSeq* d_seq; int* d_out;
  auto layout = [&](WsLayout l) {
    A.take(l);
    d_seq = l.take<LbSeq>(n);
    d_out = l.take<int>((size_t)total);
    return l.bytes();
  };
  HostScope hs;
  rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(A.upload(hs));
  MNC_HIP_TRY(hs.up(d_seq, seq.data(), seq.size() * sizeof(LbSeq)));
  TimedSpan span(g_lb_timer);
  span.begin(hs.stream);
  hipLaunchKernelGGL(lb_paint_kernel, dim3(lb_blocks((long long)H * strips * 64)), dim3(kLbThreads), 0, hs.stream, A.view(), d_seq, n,
                     background, H, W, strips, d_out);
  span.end(hs.stream);
  MNC_HIP_TRY(hipGetLastError());
  MNC_HIP_TRY(hs.down(out, d_out, (size_t)total * sizeof(int)));
  MNC_HIP_TRY(hs.sync());
  span.keep();
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_mask_labels_timing(int on, double* last_ms) { return g_lb_timer.set(on, last_ms); }
