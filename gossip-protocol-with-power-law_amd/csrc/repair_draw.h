// repair_draw.h -- the partner draw of anti-entropy repair (repair.hip,
// DESIGN.md §2.2, §2.6, §3.21), plain C++ for host and device:
// tests/test_repair_draw.py drives it on the CPU through
// tests/native/repair_draw_shim.cpp.
//
// Round r is a repair round iff (r + 1) % period == 0.  In one, every up
// receiver v with an in-neighbour pulls the Message-List of
//
//   p_r(v) = col[row_ptr[v] + below(draw(stream_key(seed, STREAM_REPAIR + r), u64(v)), deg_in(v))]
//
// with v a global vertex id and the in-CSR as loaded or built.  The draw sees
// the receiver and the round only: it is the same for every message, row width
// and message block.
#pragma once
#include <cstdint>

#include "gp_common.h"

namespace gp {

// the link-delay stream is 0x300; the loss streams end at 0x2FD
constexpr uint64_t STREAM_REPAIR = 0x400;   // + round (r <= 253: 0x400 .. 0x4FD)
constexpr int32_t REPAIR_PERIOD_MAX = 64;

GP_HD bool repair_round(int32_t r, int32_t period) { return period > 0 && (r + 1) % period == 0; }

GP_HD uint64_t repair_round_key(uint64_t seed, uint32_t round) { return stream_key(seed, STREAM_REPAIR + (uint64_t)round); }

// index into v's in-list of its partner under `key` (one round's); deg > 0
GP_HD uint64_t repair_partner_index(uint64_t key, uint64_t v, uint64_t deg) { return below(draw(key, v), deg); }

}  // namespace gp
