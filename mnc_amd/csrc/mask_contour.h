// Outlines of packed masks (include/mnc_hip.h n13): the pieces of csrc/mask_contours.hip that work on values alone -- the boundary
// edges that leave the 64 lattice points of one word, their ids, the turn at a point, the successor of an edge.  Host and device:
// tests/c/mask_contour_main.cpp drives the same code sequentially on the CPU.  Nothing but the compiler's builtins is used, so the
// file stands without the HIP headers.
//
// A w x h mask has (w + 1) x (h + 1) lattice points; point (X, Y) is the top left corner of pixel (X, Y).  The points of a row are
// cut into words of 64 like the pixels: bit b of word j of point row Y is point (64 j + b, Y).  An edge belongs to its TAIL point.
#pragma once

#if defined(__HIPCC__)
#define MNC_CT_HD __host__ __device__ inline
#else
#define MNC_CT_HD inline
#endif

namespace mnc {

typedef unsigned long long ct_u64;

// The direction of an edge, y pointing down: clockwise on screen, so that a right turn is + 1 and a left turn is - 1 (mod 4).
enum { kCtEast = 0, kCtSouth = 1, kCtWest = 2, kCtNorth = 3 };

// The edges that leave the points of one word, one mask per direction.
struct CtEdges {
  ct_u64 d[4];
};

// up / dn: the pixels (64 j + b, Y - 1) and (64 j + b, Y) of the point word, 0 where there is no such row or column, padding
// cleared; up_carry / dn_carry: pixel 64 j - 1 of those rows.  With the set pixel on the right of the edge:
//   east   the top side of pixel (X, Y):            it is set, the one above it is not
//   south  the right side of pixel (X - 1, Y):      it is set, pixel (X, Y) is not
//   west   the bottom side of pixel (X - 1, Y - 1): it is set, the one below it is not
//   north  the left side of pixel (X, Y - 1):       it is set, the one left of it is not
MNC_CT_HD CtEdges ct_edges(ct_u64 up, ct_u64 up_carry, ct_u64 dn, ct_u64 dn_carry) {
  const ct_u64 upl = (up << 1) | (up_carry & 1ull), dnl = (dn << 1) | (dn_carry & 1ull);
  return {{dn & ~up, dnl & ~dn, upl & ~dnl, up & ~upl}};
}

MNC_CT_HD ct_u64 ct_any(const CtEdges& e) { return e.d[0] | e.d[1] | e.d[2] | e.d[3]; }

// At most 256, and at most 128 for a real mask (a point has two edges at the most).
MNC_CT_HD int ct_count(const CtEdges& e) {
  return __builtin_popcountll(e.d[0]) + __builtin_popcountll(e.d[1]) + __builtin_popcountll(e.d[2]) + __builtin_popcountll(e.d[3]);
}

// The directions in which an edge leaves point b of the word: bit d for direction d.
MNC_CT_HD int ct_out(const CtEdges& e, int b) {
  return (int)((e.d[0] >> b) & 1ull) | (int)((e.d[1] >> b) & 1ull) << 1 | (int)((e.d[2] >> b) & 1ull) << 2 | (int)((e.d[3] >> b) & 1ull) << 3;
}

// The id of the edge that leaves point b in direction d, `base` being the id of the word's first edge: the edges of a word are
// numbered by point, then by direction.
MNC_CT_HD int ct_edge_id(int base, const CtEdges& e, int b, int d) {
  const ct_u64 low = (1ull << b) - 1ull;
  int id = base;
  for (int k = 0; k < 4; ++k) id += __builtin_popcountll(e.d[k] & low) + (k < d ? (int)((e.d[k] >> b) & 1ull) : 0);
  return id;
}

// The direction in which the loop goes on from a point it reached in direction d, `out` being the directions that leave the point
// (ct_out, not 0).  One edge leaves, or two at a point where two set pixels touch by a corner alone: those two run left and right
// of d, never straight on and never back.  eight: the left turn, so that the two pixels share a loop; otherwise the right turn.
MNC_CT_HD int ct_turn(int out, int d, int eight) {
  const int first = (d + (eight ? 3 : 1)) & 3, last = (d + (eight ? 1 : 3)) & 3;
  if ((out >> first) & 1) return first;
  if ((out >> d) & 1) return d;
  return last;
}

// The successor of the edge that leaves point b of word j of point row y in direction d -> its id, *sd its direction.  own /
// own_base: the edges of that word and the id of the first.  G gives the same of any word of the instance: g.edges(y, j) and
// g.base(y, j).  (The head of an edge of a mask is a point of the mask's lattice, and an edge leaves it: the side of the set pixel
// that the edge runs along ends there, and so does a side of a neighbour or the next side of the same pixel.)
template <class G>
MNC_CT_HD int ct_successor(const G& g, int y, int j, const CtEdges& own, int own_base, int b, int d, int eight, int* sd) {
  const int hy = y + (d == kCtSouth) - (d == kCtNorth);
  int hb = b + (d == kCtEast) - (d == kCtWest), hj = j;
  if (hb > 63) { hb = 0; ++hj; } else if (hb < 0) { hb = 63; --hj; }
  const bool same = hy == y && hj == j;
  const CtEdges h = same ? own : g.edges(hy, hj);
  const int nd = ct_turn(ct_out(h, hb), d, eight);
  *sd = nd;
  return ct_edge_id(same ? own_base : g.base(hy, hj), h, hb, nd);
}

}  // namespace mnc
