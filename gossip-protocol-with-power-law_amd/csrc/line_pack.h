// line_pack.h -- lane mapping of the packed row gather, plain
// C++ for host and device: tests/test_line_pack.py drives it on the CPU through
// tests/native/line_pack_shim.cpp.
//
// A 64-word Message-List is four 128-B lines of eight 16-B pieces.  The row
// gather of an early-exit pull loads one piece per lane, 32 lanes per row, and
// skips the pieces whose words are complete.  Under the spread order most
// receivers soon miss messages on one or two lines only, and three quarters of
// the lanes of every row load then idle.  The packed layout gives those lanes
// rows of their own: with the 4-bit mask of the lines that are still live,
//   one live line:   an octet of lanes holds that line of one sender's row,
//   two live lines:  a 16-lane group holds both lines (the lower line first),
//   three or four:   32 lanes hold the row as before; the lanes of a dead
//                    line hold nothing.
// The mapping is the same for any lane group whose width is a multiple of 32
// (a wave: 64 lanes, slots 0 .. 64 / lanes_per_row - 1; a half-wave: 32).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GP_LP_HD __host__ __device__ __forceinline__
#else
#define GP_LP_HD inline
#endif

namespace gp {

constexpr int LP_LINES = 4;         // 128-B lines of a 64-word row
constexpr int LP_LINE_PIECES = 8;   // 16-B pieces of a line

GP_LP_HD int lp_count(uint32_t mask) {
  mask &= 0xFu;
  return (int)((mask & 1u) + ((mask >> 1) & 1u) + ((mask >> 2) & 1u) + ((mask >> 3) & 1u));
}
// log2 of the lanes that hold one sender's row (mask != 0)
GP_LP_HD int lp_row_shift(uint32_t mask) {
  const int p = lp_count(mask);
  return p == 1 ? 3 : p == 2 ? 4 : 5;
}
// the j-th (0-based) live line of mask
GP_LP_HD int lp_nth_line(uint32_t mask, int j) {
  int l = 0;
  for (; l < LP_LINES; ++l) {
    if ((mask >> l) & 1u) {
      if (j == 0) break;
      --j;
    }
  }
  return l;
}
// row slot of a lane: which of the rows of one load instruction it loads from
GP_LP_HD int lp_slot(uint32_t mask, int lane) { return lane >> lp_row_shift(mask); }
// the 16-B piece (0 .. 31) of its row that a lane loads; -1: none (the lane
// lies on a dead line of the three-line layout)
GP_LP_HD int lp_piece(uint32_t mask, int lane) {
  const int sh = lp_row_shift(mask);
  if (sh == 5) {
    const int piece = lane & 31;
    return ((mask >> (piece >> 3)) & 1u) ? piece : -1;
  }
  const int j = (lane >> 3) & ((1 << (sh - 3)) - 1);   // octet of the lane inside its row group
  return LP_LINE_PIECES * lp_nth_line(mask, j) + (lane & 7);
}
// the way back: the lane that loads `piece` of the row in `slot`; -1: no lane
// (the piece lies on a dead line)
GP_LP_HD int lp_lane(uint32_t mask, int slot, int piece) {
  const int line = piece >> 3;
  if (!((mask >> line) & 1u)) return -1;
  const int sh = lp_row_shift(mask);
  if (sh == 5) return (slot << 5) + piece;
  int j = 0;   // live lines below this one
  for (int l = 0; l < line; ++l) j += (int)((mask >> l) & 1u);
  return (slot << sh) + LP_LINE_PIECES * j + (piece & 7);
}

}  // namespace gp
