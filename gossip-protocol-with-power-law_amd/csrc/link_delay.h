// link_delay.h -- the per-link delay of delayed links (delayed.hip, DESIGN.md
// §2.2, §2.6, §3.19), plain C++ for host and device: tests/test_link_delay.py
// drives it on the CPU through tests/native/link_delay_shim.cpp.
//
// With delay on, the line u puts on arc u -> v in round s has receipt round
// s + d(u, v),
//
//   d(u, v) = 1 + below(draw(stream_key(seed, STREAM_LINK_DELAY),
//                            (u64(min(u, v)) << 32) | u64(max(u, v))), dmax)
//
// with u, v global vertex ids and dmax in [1, LINK_DELAY_MAX].  The delay
// belongs to the unordered pair and the run: a link is as slow one way as the
// other, the same in every round, for every message and row width, and
// parallel arcs of a raw CSR share it.  dmax = 1 gives 1 everywhere: the flood.
#pragma once
#include <cstdint>

#include "gp_common.h"

namespace gp {

// the loss streams STREAM_LOSS + r (r <= 253) end at 0x2FD
constexpr uint64_t STREAM_LINK_DELAY = 0x300;
constexpr int32_t LINK_DELAY_MAX = 8;

GP_HD uint64_t link_delay_key(uint64_t seed) { return stream_key(seed, STREAM_LINK_DELAY); }

// rounds the link between u and v takes under `key` (link_delay_key): 1 .. dmax
GP_HD uint32_t arc_delay(uint64_t key, uint32_t u, uint32_t v, uint32_t dmax) {
  const uint32_t lo = u < v ? u : v, hi = u < v ? v : u;
  return 1u + (uint32_t)below(draw(key, ((uint64_t)lo << 32) | (uint64_t)hi), (uint64_t)dmax);
}

}  // namespace gp
