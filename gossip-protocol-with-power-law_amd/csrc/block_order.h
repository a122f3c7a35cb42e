// block_order.h -- launch order of k_expand's 64-vertex blocks (DESIGN.md
// §3.3).  Plain C++, no HIP: build_hubs (setup.hip) calls it once per overlay
// and hub table, and tests/test_block_order.py drives it on synthetic row_ptr
// arrays on the CPU.
//
// A wave of k_expand owns 64 consecutive vertices and walks its receivers one
// after the other, so a block's time is bounded below by its longest in-list.
// Vertex ids are a random relabelling: the few long non-hub in-lists sit in
// random blocks, and one that is dispatched late in the grid ends the kernel on
// a drained machine.  Blocks whose longest non-hub in-list exceeds `cut` are
// therefore launched first, longest first (ties by block id); every other
// block keeps its natural place, so consecutive waves still read consecutive
// vertices.  Hubs (in-degree > hub_thr) are scanned by the hub kernels, not by
// their block's wave, and do not count.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace gp {

// row_ptr: in-CSR offsets of the owned vertices [0, nloc] (local ids).
// Returns order[k] = the block the k-th wave takes, a permutation of
// [0, ceil(nloc / 64)).
inline std::vector<int32_t> block_order(const int64_t* row_ptr, int64_t nloc, int64_t hub_thr, int64_t cut) {
  const int64_t nb = (nloc + 63) / 64;
  std::vector<int32_t> order;
  order.reserve((size_t)nb);
  std::vector<std::pair<int64_t, int32_t>> heavy;   // (longest non-hub in-list, block)
  std::vector<uint8_t> first((size_t)nb, 0);
  for (int64_t b = 0; b < nb; ++b) {
    int64_t longest = 0;
    const int64_t v1 = std::min(nloc, (b + 1) * 64);
    for (int64_t v = b * 64; v < v1; ++v) {
      const int64_t d = row_ptr[v + 1] - row_ptr[v];
      if (d <= hub_thr) longest = std::max(longest, d);
    }
    if (longest > cut) {
      heavy.emplace_back(longest, (int32_t)b);
      first[(size_t)b] = 1;
    }
  }
  std::sort(heavy.begin(), heavy.end(), [](const std::pair<int64_t, int32_t>& x, const std::pair<int64_t, int32_t>& y) {
    return x.first != y.first ? x.first > y.first : x.second < y.second;
  });
  for (const auto& h : heavy) order.push_back(h.second);
  for (int64_t b = 0; b < nb; ++b)
    if (!first[(size_t)b]) order.push_back((int32_t)b);
  return order;
}

}  // namespace gp
