// link_loss_shim.cpp -- test-only C wrapper around csrc/link_loss.h (host
// code, no HIP), compiled with g++ by tests/test_link_loss.py so the draw the
// lossy kernels compute is checked on the CPU.
#include "link_loss.h"

extern "C" {

unsigned long long ll_threshold(double p) { return gp::loss_threshold(p); }

unsigned long long ll_round_key(unsigned long long seed, unsigned r) { return gp::loss_round_key(seed, r); }

// open[i] = arc u[i] -> v[i] delivers in round r[i] under (seed[i], p)
void ll_open(const unsigned long long* seed, const unsigned* r, const unsigned* u, const unsigned* v, double p,
             unsigned char* open, long long count) {
  for (long long i = 0; i < count; ++i) {
    const gp::LossDraw d = gp::loss_draw(p, seed[i], r[i]);
    open[i] = (!d.closed && gp::arc_open(d.key, u[i], v[i], d.thresh)) ? 1 : 0;
  }
}

}  // extern "C"
