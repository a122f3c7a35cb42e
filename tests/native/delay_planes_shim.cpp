// delay_planes_shim.cpp -- test-only C wrapper around csrc/delay_planes.h
// (plain C++, no HIP), compiled with g++ by tests/test_delay_planes.py so the
// plane construction, the weighted sum and the minimum descent of k_delay
// (csrc/delay.hip) are checked on the CPU against per-bit arithmetic.
#include <cstdint>

#include "delay_planes.h"

extern "C" {

int dp_planes_per_word() { return gp::DELAY_PLANES; }
unsigned int dp_no_min() { return gp::DELAY_NO_MIN; }

// planes[b * words + w], as delay_reset builds them
void dp_build(const unsigned char* inject, int m, int words, unsigned long long* planes) {
  gp::delay_build_planes(inject, m, words, reinterpret_cast<uint64_t*>(planes));
}

int dp_uniform(const unsigned char* inject, int m) { return gp::delay_uniform_round(inject, m); }

// one word the way a lane of k_delay takes it: its 8 plane words first
void dp_word(unsigned long long x, const unsigned long long* planes, int words, int w, unsigned int* sum,
             unsigned int* mn) {
  uint64_t p[gp::DELAY_PLANES];
  for (int b = 0; b < gp::DELAY_PLANES; ++b) p[b] = planes[b * words + w];
  *sum = gp::delay_inject_sum((uint64_t)x, p);
  *mn = gp::delay_inject_min((uint64_t)x, p);
}

// one new row of receipt round rr the way its W lanes and their reduction take
// it: out[0] = the row's share of delay_sum, out[1] = its largest delay (0 for
// an empty row, which the kernel's guard never lets through)
void dp_row(const unsigned long long* row, const unsigned long long* planes, int words, unsigned int rr,
            unsigned int* out) {
  unsigned int tot = 0, inj = 0, mn = gp::DELAY_NO_MIN;
  for (int w = 0; w < words; ++w) {
    unsigned int s, m;
    dp_word(row[w], planes, words, w, &s, &m);
    tot += gp::delay_popc((uint64_t)row[w]);
    inj += s;
    mn = m < mn ? m : mn;
  }
  out[0] = rr * tot - inj;
  out[1] = tot ? rr - mn : 0u;
}

int dp_bin(long long deg) { return gp::delay_bin(deg); }

}  // extern "C"
