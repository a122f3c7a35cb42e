// curve_planes.h -- bit-sliced row counting of the spread curve (curve.hip,
// DESIGN.md §3.7), plain C++ for host and device: tests/test_curve_planes.py
// drives it on the CPU through tests/native/curve_planes_shim.cpp.
//
// One CurvePlanes holds, for each of the 64 bit columns of one word position,
// how many of the rows added so far had the bit set, as an 11-bit number whose
// binary digits are spread over 11 words: ones / twos / fours and 8 planes of
// eights (Harley-Seal carry-save adders, as bitcount.hip counts whole
// Message-Lists).  Eight rows enter through a CSA tree for ~15 logic ops per
// row word instead of a per-bit loop's 64 adds; the planes are expanded into
// per-bit counts only when they are full or the caller's range ends.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GP_CURVE_HD __host__ __device__ __forceinline__
#else
#define GP_CURVE_HD inline
#endif

namespace gp {

// rows the planes can hold per bit column: 3 low planes + 8 planes of eights
constexpr int CURVE_PLANE_ROWS = 2047;
constexpr int CURVE_GROUP = 8;   // rows of one curve_add8

struct CurvePlanes {
  uint64_t o1 = 0, o2 = 0, o4 = 0;
  uint64_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

GP_CURVE_HD void curve_clear(CurvePlanes& p) {
  p.o1 = p.o2 = p.o4 = 0;
  for (int j = 0; j < 8; ++j) p.e[j] = 0;
}

// room for `adding` more rows after `held`?  (held counts rows as the caller
// books them: an upper bound is enough)
GP_CURVE_HD bool curve_fits(int held, int adding) { return held + adding <= CURVE_PLANE_ROWS; }

GP_CURVE_HD void curve_csa(uint64_t& h, uint64_t& l, uint64_t a, uint64_t b, uint64_t c) {
  const uint64_t u = a ^ b;
  h = (a & b) | (u & c);
  l = u ^ c;
}

// carry `t8` (weight 8) into the planes of eights
GP_CURVE_HD void curve_carry8(CurvePlanes& p, uint64_t t8) {
  for (int j = 0; j < 8; ++j) {
    const uint64_t cj = p.e[j] & t8;
    p.e[j] ^= t8;
    t8 = cj;
  }
}

// add one row word (ripple through the low planes)
GP_CURVE_HD void curve_add_row(CurvePlanes& p, uint64_t x) {
  uint64_t c = p.o1 & x;
  p.o1 ^= x;
  uint64_t c2 = p.o2 & c;
  p.o2 ^= c;
  const uint64_t c4 = p.o4 & c2;
  p.o4 ^= c2;
  curve_carry8(p, c4);
}

// add eight row words through the CSA tree
GP_CURVE_HD void curve_add8(CurvePlanes& p, const uint64_t* x) {
  uint64_t t2a, t2b, t4a, t4b, t8;
  curve_csa(t2a, p.o1, p.o1, x[0], x[1]);
  curve_csa(t2b, p.o1, p.o1, x[2], x[3]);
  curve_csa(t4a, p.o2, p.o2, t2a, t2b);
  curve_csa(t2a, p.o1, p.o1, x[4], x[5]);
  curve_csa(t2b, p.o1, p.o1, x[6], x[7]);
  curve_csa(t4b, p.o2, p.o2, t2a, t2b);
  curve_csa(t8, p.o4, p.o4, t4a, t4b);
  curve_carry8(p, t8);
}

// expand: the count of bit column b
GP_CURVE_HD uint32_t curve_count(const CurvePlanes& p, int b) {
  uint32_t hi = 0;
  for (int j = 0; j < 8; ++j) hi |= (uint32_t)((p.e[j] >> b) & 1ull) << j;
  return (uint32_t)((p.o1 >> b) & 1ull) + 2u * (uint32_t)((p.o2 >> b) & 1ull) +
         4u * (uint32_t)((p.o4 >> b) & 1ull) + 8u * hi;
}

}  // namespace gp
