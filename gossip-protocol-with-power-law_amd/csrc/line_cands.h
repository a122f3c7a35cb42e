// line_cands.h -- candidates of the per-line done-neighbour rule (DESIGN.md
// §3.3 "Complete lines of a top in-neighbour").  Plain C++, no HIP: build_hubs
// (setup.hip) calls it once per overlay and hub table, and
// tests/test_line_cands.py drives it on synthetic row_ptr arrays on the CPU.
//
// Before an early-exit pull of a big W = 64 run, k_line_done (pull_aux.hip)
// notes per candidate which 128-B lines of its Message-List already hold
// every message of its component; a receiver whose first two gather-order
// in-neighbours name such a line takes it from its target and fetches it from
// nobody.  Only big vertices are worth the pass: they complete lines first,
// and the gather order puts them at the head of most in-lists.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gp {

// in-degree from which a vertex is a candidate (GP_LINE_DONE_MIN_DEG=k in the
// environment overrides it per context).  profiles/LEDGER.md "Complete lines
// of a top in-neighbour": on the CPU model at 2^22, 64 saves 40 % of round
// 3's row lines and 20 % of round 4's, 256 saves 36 % and 3 %, 1024 26 % and
// none; at 64 the pass reads 2.5 % of the vertices' rows
#ifndef GP_LINE_DONE_MIN_DEG
#define GP_LINE_DONE_MIN_DEG 64
#endif

// row_ptr: in-CSR offsets of the owned vertices [0, nloc] (local ids).
// Returns the vertices of in-degree >= min_deg, ascending (min_deg < 1 counts
// as 1: a vertex without in-arcs holds only what was injected at it).
inline std::vector<int32_t> line_cands(const int64_t* row_ptr, int64_t nloc, int64_t min_deg) {
  if (min_deg < 1) min_deg = 1;
  std::vector<int32_t> out;
  for (int64_t v = 0; v < nloc; ++v)
    if (row_ptr[v + 1] - row_ptr[v] >= min_deg) out.push_back((int32_t)v);
  return out;
}

}  // namespace gp
