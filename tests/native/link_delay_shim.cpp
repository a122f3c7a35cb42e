// link_delay_shim.cpp -- test-only C wrapper around csrc/link_delay.h (host
// code, no HIP), compiled with g++ by tests/test_link_delay.py so the delay the
// delayed kernels compute is checked on the CPU.
#include "link_delay.h"

extern "C" {

unsigned long long ld_key(unsigned long long seed) { return gp::link_delay_key(seed); }

// out[i] = d(u[i], v[i]) under (seed[i], dmax)
void ld_delay(const unsigned long long* seed, const unsigned* u, const unsigned* v, unsigned dmax, unsigned char* out,
              long long count) {
  for (long long i = 0; i < count; ++i)
    out[i] = (unsigned char)gp::arc_delay(gp::link_delay_key(seed[i]), u[i], v[i], dmax);
}

}  // extern "C"
