// Drives mnc_amd/csrc/mask_cc.h -- the run extraction and the union-find of csrc/mask_components.hip -- sequentially on the CPU, so that
// it can be built with -fsanitize=address,undefined and checked without a GPU (tests/test_mask_components_host.py builds and runs it).
//
//   mask_cc_main FILE      FILE: int32 count, then per mask int32 h, w and h * w bytes (0 / 1), row-major.
//
// Every mask is packed into rows of 64-bit words with every padding bit set (the reader clears it, as mask_word does), labelled
// through the helpers at connectivity 4 and 8 with the words visited in three different orders (any order must give the same
// roots), and compared pixel by pixel with a flood fill that numbers the components by their first pixel.  Prints one line per mask,
// "h w count4 count8"; exits 1 at the first difference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mnc_amd/csrc/mask_cc.h"

using mnc::cc_u64;

struct Packed {
  int h, w, strips;
  std::vector<cc_u64> words;
  cc_u64 word(int y, int j) const {   // 0 outside the row, the padding cleared
    if (j < 0 || j >= strips) return 0;
    cc_u64 v = words[(size_t)y * strips + j];
    const int valid = w - j * 64;
    if (valid < 64) v &= (1ull << valid) - 1ull;
    return v;
  }
  cc_u64 starts(int y, int j) const { return mnc::cc_starts(word(y, j), word(y, j - 1) >> 63); }
};

static Packed pack(const std::vector<unsigned char>& m, int h, int w) {
  Packed p;
  p.h = h; p.w = w; p.strips = (w + 63) / 64;
  p.words.assign((size_t)h * p.strips, 0);
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x)
      if (m[(size_t)y * w + x]) p.words[(size_t)y * p.strips + x / 64] |= 1ull << (x % 64);
    if (w % 64) p.words[(size_t)y * p.strips + p.strips - 1] |= ~0ull << (w % 64);   // dirty padding
  }
  return p;
}

// The labels (1 .. count, 0 = background) through mask_cc.h, the words visited in `order` (0 forwards, 1 backwards, 2 in a stride).
static int label_runs(const Packed& p, int e, int order, std::vector<int>* labels) {
  const int nwords = p.h * p.strips;
  std::vector<int> base((size_t)nwords + 1, 0);
  for (int g = 0; g < nwords; ++g) base[g + 1] = base[g] + __builtin_popcountll(p.starts(g / p.strips, g % p.strips));
  const int runs = base[nwords];
  std::vector<int> parent((size_t)runs);
  for (int r = 0; r < runs; ++r) parent[r] = r;
  const int stride = 37;                                 // a permutation unless the count is a multiple of 37 (then: forwards)
  for (int k = 0; k < nwords; ++k) {
    int g = order == 0 ? k : order == 1 ? nwords - 1 - k : (int)(((long long)k * stride) % nwords);
    if (order == 2 && nwords % stride == 0) g = k;
    const int y = g / p.strips, j = g % p.strips;
    if (y == 0) continue;
    const cc_u64 v = p.word(y, j);
    if (!v) continue;
    const cc_u64 a = p.word(y - 1, j), a_prev = p.word(y - 1, j - 1), a_next = p.word(y - 1, j + 1);
    int left_run = -1, right_run = -1;
    if (e && (v & 1ull) && (a_prev >> 63)) left_run = mnc::cc_run_at(base[g - p.strips - 1], p.starts(y - 1, j - 1), 63);
    if (e && (v >> 63) && (a_next & 1ull)) right_run = mnc::cc_run_at(base[g - p.strips + 1], mnc::cc_starts(a_next, a >> 63), 0);
    mnc::cc_link_word(parent.data(), v, p.starts(y, j), base[g], a, p.starts(y - 1, j), base[g - p.strips], left_run, right_run, e);
  }
  for (int r = 0; r < runs; ++r) {
    if (parent[r] > r) { std::printf("parent[%d] = %d points upwards\n", r, parent[r]); std::exit(1); }
    const int root = mnc::cc_root(parent.data(), r);
    mnc::cc_lower(parent.data() + r, root);
  }
  std::vector<int> number((size_t)runs, 0);
  int count = 0;
  for (int r = 0; r < runs; ++r) number[r] = parent[r] == r ? count++ : -1;
  labels->assign((size_t)p.h * p.w, 0);
  for (int g = 0; g < nwords; ++g) {
    const int y = g / p.strips, j = g % p.strips;
    cc_u64 v = p.word(y, j);
    const cc_u64 st = p.starts(y, j);
    while (v) {
      const cc_u64 seg = mnc::cc_take_seg(v);
      const int lo = mnc::cc_low_bit(seg), len = __builtin_popcountll(seg);
      const int r = mnc::cc_run_at(base[g], st, lo);
      if (r < 0 || r >= runs) { std::printf("run id %d outside [0, %d)\n", r, runs); std::exit(1); }
      for (int k = 0; k < len; ++k) (*labels)[(size_t)y * p.w + j * 64 + lo + k] = number[parent[r]] + 1;
    }
  }
  return count;
}

// The same by a flood fill in raster order.
static int label_fill(const std::vector<unsigned char>& m, int h, int w, int e, std::vector<int>* labels) {
  labels->assign((size_t)h * w, 0);
  std::vector<int> stack;
  int count = 0;
  for (int s = 0; s < h * w; ++s) {
    if (!m[s] || (*labels)[s]) continue;
    (*labels)[s] = ++count;
    stack.push_back(s);
    while (!stack.empty()) {
      const int at = stack.back();
      stack.pop_back();
      const int y = at / w, x = at % w;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((!dy && !dx) || (!e && dy && dx)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
          const int to = yy * w + xx;
          if (m[to] && !(*labels)[to]) { (*labels)[to] = count; stack.push_back(to); }
        }
    }
  }
  return count;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: mask_cc_main FILE\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (int i = 0; i < count; ++i) {
    int32_t hw[2];
    if (std::fread(hw, 4, 2, f) != 2) return 2;
    const int h = hw[0], w = hw[1];
    std::vector<unsigned char> m((size_t)h * w);
    if (!m.empty() && std::fread(m.data(), 1, m.size(), f) != m.size()) return 2;
    const Packed p = pack(m, h, w);
    int counts[2];
    for (int e = 0; e < 2; ++e) {
      std::vector<int> want, got;
      counts[e] = label_fill(m, h, w, e, &want);
      for (int order = 0; order < 3; ++order) {
        const int c = label_runs(p, e, order, &got);
        if (c != counts[e] || got != want) {
          std::printf("mask %d (%d x %d), connectivity %d, order %d: %d components, the flood fill has %d\n", i, h, w, e ? 8 : 4, order,
                      c, counts[e]);
          return 1;
        }
      }
    }
    std::printf("%d %d %d %d\n", h, w, counts[0], counts[1]);
  }
  std::fclose(f);
  return 0;
}
