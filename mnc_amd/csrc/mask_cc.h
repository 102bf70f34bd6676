// Connected components of packed masks (include/mnc_hip.h n12): the pieces of csrc/mask_components.hip that work on values and
// on the parent array alone -- the runs of a word, the lock-free union-find, the unions of one word with the row above.  Host and
// device: tests/c/mask_cc_main.cpp drives the same code sequentially on the CPU.  Nothing but the compiler's builtins is used, so
// the file stands without the HIP headers.
#pragma once

#if defined(__HIPCC__)
#define MNC_CC_HD __host__ __device__ inline
#else
#define MNC_CC_HD inline
#endif

namespace mnc {

typedef unsigned long long cc_u64;

// The run starts of a word: the set bits whose neighbour below is unset; carry = the last pixel of the word before in the row.
MNC_CC_HD cc_u64 cc_starts(cc_u64 v, cc_u64 carry) { return v & ~((v << 1) | (carry & 1ull)); }

// The lowest group of neighbouring set bits of v, taken out of v (v != 0).
MNC_CC_HD cc_u64 cc_take_seg(cc_u64& v) {
  const cc_u64 t = v + (v & (~v + 1ull));   // the carry runs through the group (and out of the word, when the group ends at bit 63)
  const cc_u64 seg = v & ~t;
  v &= t;
  return seg;
}

MNC_CC_HD int cc_low_bit(cc_u64 v) { return __builtin_ctzll(v); }

// The run that holds the set bit b of a word whose run starts are `starts` and whose first start has the id `base`: a group that
// goes on from the word before has no start at or below b and belongs to the run before `base`.
MNC_CC_HD int cc_run_at(int base, cc_u64 starts, int b) { return base + __builtin_popcountll(starts & ((2ull << b) - 1ull)) - 1; }

// parent[] is shared between all threads of the union kernel: relaxed atomics at device scope there, plain accesses on the host.
MNC_CC_HD int cc_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
MNC_CC_HD void cc_lower(int* p, int v) {          // *p = min(*p, v)
#if defined(__HIP_DEVICE_COMPILE__)
  (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  if (v < *p) *p = v;
#endif
}
MNC_CC_HD int cc_swap_if(int* p, int expect, int v) {   // -> what *p held; stores v when that was `expect`
#if defined(__HIP_DEVICE_COMPILE__)
  (void)__hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return expect;
#else
  const int old = *p;
  if (old == expect) *p = v;
  return old;
#endif
}

// The root of x, halving the path on the way.
MNC_CC_HD int cc_find(int* parent, int x) {
  // Parents only decrease: cc_unite links a root under a smaller id, and the halving below lowers a parent to a grandparent with an
  // atomic minimum.  So parent[i] <= i holds at every moment, and parent[i] < i once i is no root.  Every turn of this loop goes on
  // from a strictly smaller id (g < q < x): it ends after at most x turns, whatever other threads do meanwhile.
  for (;;) {
    const int q = cc_load(parent + x);
    if (q == x) return x;
    const int g = cc_load(parent + q);
    if (g == q) return q;
    cc_lower(parent + x, g);
    x = g;
  }
}

// The root of x once nothing is united any more; nothing is written.
MNC_CC_HD int cc_root(const int* parent, int x) {
  for (;;) {                                       // parent[x] < x for every x that is no root: strictly down
    const int q = cc_load(parent + x);
    if (q == x) return x;
    x = q;
  }
}

// One set out of the sets of a and b: the larger root goes under the smaller.  Never links upwards.
MNC_CC_HD void cc_unite(int* parent, int a, int b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const int old = cc_swap_if(parent + hi, hi, lo);   // only a root is linked, and only under a smaller id
    if (old == hi) return;
    // hi was linked by another thread in between (old < hi is its parent now): that thread made a link, of which there are fewer
    // than runs, so this loop cannot turn for ever either.  Go on from what is known.
    a = lo;
    b = old;
  }
}

// The unions of one word v with the row above it.  starts / base: v's run starts and the id of its first start; a, a_starts,
// a_base: the same of the word above.  e = 1 (8-connectivity): a run also touches the pixels one column to either side of it in
// the row above; left_run / right_run: the run of the pixel above-left of bit 0 / above-right of bit 63, -1 when that pixel is
// unset.  (The groups of `a & reach` lie in different runs of a, since reach has no gap.)
MNC_CC_HD void cc_link_word(int* parent, cc_u64 v, cc_u64 starts, int base, cc_u64 a, cc_u64 a_starts, int a_base, int left_run,
                            int right_run, int e) {
  while (v) {
    const cc_u64 seg = cc_take_seg(v);
    const int r = cc_run_at(base, starts, cc_low_bit(seg));
    cc_u64 hit = a & (e ? seg | (seg << 1) | (seg >> 1) : seg);
    while (hit) {
      const cc_u64 s = cc_take_seg(hit);
      cc_unite(parent, r, cc_run_at(a_base, a_starts, cc_low_bit(s)));
    }
    if (e && (seg & 1ull) && left_run >= 0) cc_unite(parent, r, left_run);
    if (e && (seg >> 63) && right_run >= 0) cc_unite(parent, r, right_run);
  }
}

}  // namespace mnc
