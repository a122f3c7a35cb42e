// link_loss.h -- the per-arc, per-round draw of lossy links (lossy.hip,
// DESIGN.md §2.2, §2.6, §3.18), plain C++ for host and device:
// tests/test_link_loss.py drives it on the CPU through
// tests/native/link_loss_shim.cpp.
//
// With loss on, the line u puts on arc u -> v in round r arrives iff
//
//   draw(stream_key(seed, STREAM_LOSS + r), (u64(u) << 32) | u64(v)) >= thresh
//
// with u, v global vertex ids and thresh = (uint64_t)ldexp(p, 64) for
// 0 < p < 1 (k_churn's own conversion).  The draw belongs to the ordered pair
// and the round: it is the same for every message and row width, independent
// for u -> v and v -> u, and parallel arcs of a raw CSR share it.  p = 0 has
// thresh 0 (every draw passes: every arc open); p = 1 has no 64-bit threshold
// and is carried as `closed`.
#pragma once
#include <cmath>
#include <cstdint>

#include "gp_common.h"

namespace gp {

// the crash streams STREAM_CRASH + r (r <= 253) end at 0x1FD
constexpr uint64_t STREAM_LOSS = 0x200;   // + round

// what a lossy round's kernels take beside their argument block
struct LossDraw {
  uint64_t key;      // loss_round_key(seed, r)
  uint64_t thresh;   // open iff draw >= thresh
  int32_t closed;    // p = 1: every arc closed, nothing is drawn
};

// p in [0, 1]: the threshold of 0 < p < 1, else 0
inline uint64_t loss_threshold(double p) { return (p > 0.0 && p < 1.0) ? (uint64_t)std::ldexp(p, 64) : 0ull; }

GP_HD uint64_t loss_round_key(uint64_t seed, uint32_t round) { return stream_key(seed, STREAM_LOSS + (uint64_t)round); }

// arc u -> v is open under `key` (one round's) and `thresh`
GP_HD bool arc_open(uint64_t key, uint32_t u, uint32_t v, uint64_t thresh) {
  return draw(key, ((uint64_t)u << 32) | (uint64_t)v) >= thresh;
}

inline LossDraw loss_draw(double p, uint64_t seed, uint32_t round) {
  return LossDraw{loss_round_key(seed, round), loss_threshold(p), p >= 1.0 ? 1 : 0};
}

}  // namespace gp
