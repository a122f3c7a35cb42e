// curve_planes_shim.cpp -- test-only C wrapper around csrc/curve_planes.h
// (plain C++, no HIP), compiled with g++ by tests/test_curve_planes.py so the
// add-a-row / add-eight / expand steps of k_curve (csrc/curve.hip) are checked
// on the CPU against per-bit counting.
#include <cstring>

#include "curve_planes.h"

extern "C" {

int cp_capacity() { return gp::CURVE_PLANE_ROWS; }
int cp_group() { return gp::CURVE_GROUP; }

// counts[b] += the rows' bit b, the way a lane of k_curve counts one word
// position: rows enter `group` at a time (8: curve_add8, a short tail padded
// with zero rows and booked as 8; 1: curve_add_row), the planes are expanded
// whenever the next step would not fit and once at the end.  Returns the
// number of expansions.
int cp_count(const unsigned long long* rows, long long n, int group, unsigned int* counts) {
  gp::CurvePlanes p;
  int held = 0, flushes = 0;
  auto flush = [&]() {
    for (int b = 0; b < 64; ++b) counts[b] += gp::curve_count(p, b);
    gp::curve_clear(p);
    held = 0;
    ++flushes;
  };
  if (group == 1) {
    for (long long i = 0; i < n; ++i) {
      if (!gp::curve_fits(held, 1)) flush();
      gp::curve_add_row(p, (uint64_t)rows[i]);
      ++held;
    }
  } else {
    for (long long i = 0; i < n; i += gp::CURVE_GROUP) {
      uint64_t x[gp::CURVE_GROUP];
      for (int k = 0; k < gp::CURVE_GROUP; ++k) x[k] = i + k < n ? (uint64_t)rows[i + k] : 0ull;
      if (!gp::curve_fits(held, gp::CURVE_GROUP)) flush();
      gp::curve_add8(p, x);
      held += gp::CURVE_GROUP;
    }
  }
  if (held > 0) flush();
  return flushes;
}

// the planes alone, no expansion in between: what n rows leave in them
// (n <= capacity is the caller's business; beyond it the counts wrap)
void cp_raw(const unsigned long long* rows, long long n, unsigned int* counts) {
  gp::CurvePlanes p;
  for (long long i = 0; i < n; ++i) gp::curve_add_row(p, (uint64_t)rows[i]);
  for (int b = 0; b < 64; ++b) counts[b] = gp::curve_count(p, b);
}

}  // extern "C"
