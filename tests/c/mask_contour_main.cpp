// Drives mnc_amd/csrc/mask_contour.h -- the edge masks, the edge ids and the successor of csrc/mask_contours.hip -- sequentially on the
// CPU, so that it can be built with -fsanitize=address,undefined and checked without a GPU (tests/test_mask_contours_host.py builds
// and runs it).
//
//   mask_contour_main FILE   FILE: int32 count, then per mask int32 h, w and h * w bytes (0 / 1), row-major, and for connectivity 4
//                            and then 8 the loops the statement (mnc_amd/contours.py:contours_numpy) finds in it with pixel (0, 0)
//                            at the origin: int32 L, per loop int32 k, int64 area and k pairs of int32 (x, y).
//
// Every mask is packed into rows of 64-bit words with every padding bit set (the reader clears it, as mask_word does).  The edges
// are counted and numbered through the helpers, every successor is taken, and the loops are built the way the kernels build them:
// the rounds of pointer jumping with a running minimum, the cut in front of the leaders, the rounds of list ranking, the slots.  The
// successor must be a permutation, the leaders the smallest ids of their cycles (checked by walking the cycles), and the loops the
// statement's, vertex by vertex.  Prints one line per mask, "h w edges loops4 loops8"; exits 1 at the first difference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mnc_amd/csrc/mask_contour.h"

using mnc::ct_u64;
using mnc::CtEdges;

struct Loop {
  long long area;
  std::vector<int32_t> xy;
  bool operator==(const Loop& o) const { return area == o.area && xy == o.xy; }
};

// The G of ct_successor: the point words of one mask and the id of the first edge of each.
struct Grid {
  int h, w, rs, vs;
  std::vector<ct_u64> words;
  std::vector<int> first;                                // [(h + 1) * vs + 1]
  void row(int y, int j, ct_u64* v, ct_u64* carry) const {   // pixel word j of pixel row y and the pixel before it; 0 outside
    *v = 0; *carry = 0;
    if (y < 0 || y >= h) return;
    *v = word(y, j);
    *carry = word(y, j - 1) >> 63;
  }
  ct_u64 word(int y, int j) const {
    if (j < 0 || j >= rs) return 0;
    ct_u64 v = words[(size_t)y * rs + j];
    const int valid = w - j * 64;
    if (valid < 64) v &= (1ull << valid) - 1ull;
    return v;
  }
  CtEdges edges(int y, int j) const {
    ct_u64 up, upc, dn, dnc;
    row(y - 1, j, &up, &upc);
    row(y, j, &dn, &dnc);
    return mnc::ct_edges(up, upc, dn, dnc);
  }
  int base(int y, int j) const { return first.at((size_t)y * vs + j); }
};

static Grid pack(const std::vector<unsigned char>& m, int h, int w) {
  Grid g;
  g.h = h; g.w = w; g.rs = (w + 63) / 64; g.vs = (w + 64) / 64;
  g.words.assign((size_t)h * g.rs, 0);
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x)
      if (m[(size_t)y * w + x]) g.words[(size_t)y * g.rs + x / 64] |= 1ull << (x % 64);
    if (w % 64) g.words[(size_t)y * g.rs + g.rs - 1] |= ~0ull << (w % 64);   // dirty padding
  }
  const int nwords = (h + 1) * g.vs;
  g.first.assign((size_t)nwords + 1, 0);
  for (int k = 0; k < nwords; ++k) g.first[k + 1] = g.first[k] + mnc::ct_count(g.edges(k / g.vs, k % g.vs));
  return g;
}

static void fail(const char* what, long long a, long long b) {
  std::printf("%s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

// The loops of the mask at this connectivity, as csrc/mask_contours.hip makes them.
static std::vector<Loop> trace(const Grid& g, int eight, int* edge_count) {
  const int nwords = (g.h + 1) * g.vs, E = g.first[nwords];
  *edge_count = E;
  std::vector<int> succ((size_t)E, -1), x((size_t)E), y((size_t)E), dir((size_t)E), vertex((size_t)E, -1);
  for (int k = 0; k < nwords; ++k) {
    const int py = k / g.vs, pj = k % g.vs;
    const CtEdges own = g.edges(py, pj);
    int e = g.first[k];
    for (int b = 0; b < 64; ++b)
      for (int d = 0; d < 4; ++d) {
        if (!((own.d[d] >> b) & 1ull)) continue;
        if (mnc::ct_edge_id(g.first[k], own, b, d) != e) fail("an edge id out of order", e, k);
        if (!((mnc::ct_out(own, b) >> d) & 1)) fail("ct_out misses an edge", e, k);
        int sd = -1;
        const int to = mnc::ct_successor(g, py, pj, own, g.first[k], b, d, eight, &sd);
        if (to < 0 || to >= E) fail("a successor outside the edges", e, to);
        if (vertex[to] >= 0) fail("two edges with one successor", e, to);
        succ[e] = to; x[e] = pj * 64 + b; y[e] = py; dir[e] = d;
        vertex[to] = sd != d;
        ++e;
      }
    if (e != g.first[k + 1]) fail("the edges of a word do not number its count", e, g.first[k + 1]);
  }
  for (int e = 0; e < E; ++e) {
    const int to = succ[e];
    const int dx = (dir[e] == mnc::kCtEast) - (dir[e] == mnc::kCtWest), dy = (dir[e] == mnc::kCtSouth) - (dir[e] == mnc::kCtNorth);
    if (x[to] != x[e] + dx || y[to] != y[e] + dy) fail("a successor that does not leave the head", e, to);
  }
  int rounds = 0;
  while ((1ll << rounds) < E) ++rounds;
  // pointer jumping with a running minimum, two buffers
  std::vector<int> lead[2], next[2], rank[2];
  for (int k = 0; k < 2; ++k) { lead[k].assign((size_t)E, 0); next[k].assign((size_t)E, 0); rank[k].assign((size_t)E, 0); }
  for (int e = 0; e < E; ++e) { lead[0][e] = e; next[0][e] = succ[e]; }
  for (int k = 0; k < rounds; ++k)
    for (int e = 0; e < E; ++e) {
      const int t = next[k & 1][e];
      lead[~k & 1][e] = lead[k & 1][e] < lead[k & 1][t] ? lead[k & 1][e] : lead[k & 1][t];
      next[~k & 1][e] = next[k & 1][t];
    }
  const std::vector<int>& head = lead[rounds & 1];
  // the same by walking every cycle from its smallest edge
  std::vector<int> want((size_t)E, -1);
  for (int e = 0; e < E; ++e)
    if (want[e] < 0)
      for (int t = e; want[t] < 0; t = succ[t]) want[t] = e;
  if (head != want) fail("the jumping rounds do not find the smallest edge of every cycle", E, rounds);
  // the cut, the ranking
  for (int e = 0; e < E; ++e) { next[0][e] = head[succ[e]] == succ[e] ? -1 : succ[e]; rank[0][e] = vertex[e]; }
  for (int k = 0; k < rounds; ++k)
    for (int e = 0; e < E; ++e) {
      const int t = next[k & 1][e];
      rank[~k & 1][e] = rank[k & 1][e] + (t >= 0 ? rank[k & 1][t] : 0);
      next[~k & 1][e] = t >= 0 ? next[k & 1][t] : -1;
    }
  const std::vector<int>& r = rank[rounds & 1];
  std::vector<int> number((size_t)E, -1), first_vertex((size_t)E, 0);
  std::vector<Loop> loops;
  int verts = 0;
  for (int e = 0; e < E; ++e)
    if (head[e] == e) {
      number[e] = (int)loops.size();
      first_vertex[e] = verts;
      verts += r[e];
      loops.push_back(Loop{0, std::vector<int32_t>(2 * (size_t)r[e], INT32_MIN)});
    }
  for (int e = 0; e < E; ++e) {
    Loop& l = loops[(size_t)number[head[e]]];
    if (vertex[e]) {
      const int slot = r[head[e]] - r[e];
      if (slot < 0 || 2 * (size_t)slot + 1 >= l.xy.size() || l.xy[2 * (size_t)slot] != INT32_MIN) fail("a vertex slot taken twice or outside", e, slot);
      l.xy[2 * (size_t)slot] = x[e];
      l.xy[2 * (size_t)slot + 1] = y[e];
    }
    if (dir[e] == mnc::kCtSouth) l.area += x[e];
    if (dir[e] == mnc::kCtNorth) l.area -= x[e];
  }
  return loops;
}

static bool read_loops(std::FILE* f, std::vector<Loop>* loops) {
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1 || count < 0) return false;
  loops->assign((size_t)count, Loop());
  for (Loop& l : *loops) {
    int32_t k = 0;
    int64_t area = 0;
    if (std::fread(&k, 4, 1, f) != 1 || k < 0 || std::fread(&area, 8, 1, f) != 1) return false;
    l.area = area;
    l.xy.assign(2 * (size_t)k, 0);
    if (k && std::fread(l.xy.data(), 4, 2 * (size_t)k, f) != 2 * (size_t)k) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: mask_contour_main FILE\n"); return 2; }
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
    const Grid g = pack(m, h, w);
    size_t found[2];
    int edges = 0;
    for (int eight = 0; eight < 2; ++eight) {
      std::vector<Loop> want;
      if (!read_loops(f, &want)) return 2;
      const std::vector<Loop> got = trace(g, eight, &edges);
      if (!(got == want)) {
        std::printf("mask %d (%d x %d), connectivity %d: %zu loops that are not the statement's %zu\n", i, h, w, eight ? 8 : 4, got.size(),
                    want.size());
        return 1;
      }
      found[eight] = got.size();
    }
    std::printf("%d %d %d %zu %zu\n", h, w, edges, found[0], found[1]);
  }
  std::fclose(f);
  return 0;
}
