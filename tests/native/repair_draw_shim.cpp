// repair_draw_shim.cpp -- test-only C wrapper around csrc/repair_draw.h (host
// code, no HIP), compiled with g++ by tests/test_repair_draw.py so the partner
// draw the repair kernels compute is checked on the CPU.
#include "repair_draw.h"

extern "C" {

unsigned long long rd_stream() { return gp::STREAM_REPAIR; }

int rd_period_max() { return gp::REPAIR_PERIOD_MAX; }

int rd_repair_round(int r, int period) { return gp::repair_round(r, period) ? 1 : 0; }

unsigned long long rd_round_key(unsigned long long seed, unsigned r) { return gp::repair_round_key(seed, r); }

// idx[i] = index into v[i]'s in-list of its partner in round r[i] under seed[i]
void rd_partner_index(const unsigned long long* seed, const unsigned* r, const unsigned long long* v,
                      const unsigned long long* deg, unsigned long long* idx, long long count) {
  for (long long i = 0; i < count; ++i)
    idx[i] = gp::repair_partner_index(gp::repair_round_key(seed[i], r[i]), v[i], deg[i]);
}

}  // extern "C"
