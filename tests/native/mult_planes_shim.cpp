// mult_planes_shim.cpp -- test-only C wrapper around csrc/mult_planes.h (plain
// C++, no HIP), compiled with g++ by tests/test_mult_planes.py so the
// saturating bit-sliced counter of k_mult (csrc/mult.hip) is checked on the CPU
// against per-bit integer counting.  A counter crosses the boundary as five
// words: the four count planes, then the sticky plane.
#include <cstdint>

#include "mult_planes.h"

namespace {

gp::MultCounter from(const unsigned long long* w) {
  gp::MultCounter c;
  for (int b = 0; b < gp::MULT_PLANES; ++b) c.p[b] = w[b];
  c.sat = w[gp::MULT_PLANES];
  return c;
}

void to(const gp::MultCounter& c, unsigned long long* w) {
  for (int b = 0; b < gp::MULT_PLANES; ++b) w[b] = c.p[b];
  w[gp::MULT_PLANES] = c.sat;
}

}  // namespace

extern "C" {

int mp_planes() { return gp::MULT_PLANES; }
int mp_words() { return gp::MULT_WORDS; }
int mp_sat() { return gp::MULT_SAT; }
int mp_bins() { return gp::MULT_BINS; }

void mp_zero(unsigned long long* c) { to(gp::mult_zero(), c); }

// c += the words xs[0 .. n), one add each
void mp_add(unsigned long long* c, const unsigned long long* xs, int n) {
  gp::MultCounter k = from(c);
  for (int i = 0; i < n; ++i) gp::mult_add(k, (uint64_t)xs[i]);
  to(k, c);
}

// c += the words xs[0 .. n), four at a time the way a gather batch of k_mult
// adds them (the last batch padded with zero words, as lanes past the list load)
void mp_add4(unsigned long long* c, const unsigned long long* xs, int n) {
  gp::MultCounter k = from(c);
  for (int i = 0; i < n; i += 4) {
    uint64_t x[4] = {0, 0, 0, 0};
    for (int q = 0; q < 4 && i + q < n; ++q) x[q] = (uint64_t)xs[i + q];
    gp::mult_add4(k, x[0], x[1], x[2], x[3]);
  }
  to(k, c);
}

void mp_merge(unsigned long long* a, const unsigned long long* b) {
  gp::MultCounter k = from(a);
  gp::mult_merge(k, from(b));
  to(k, a);
}

// out[0]: untouched and unsaturated positions, out[1 .. 15]: count exactly c, out[16]: saturated
void mp_masks(const unsigned long long* c, unsigned long long* out) {
  const gp::MultCounter k = from(c);
  for (int cnt = 0; cnt < gp::MULT_SAT; ++cnt) out[cnt] = gp::mult_eq(k, cnt);
  out[gp::MULT_SAT] = gp::mult_saturated(k);
}

}  // extern "C"
