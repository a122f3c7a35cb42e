// mult_planes.h -- saturating bit-sliced deliverer counter of the delivery
// multiplicity record (mult.hip), plain C++ for host and
// device: tests/test_mult_planes.py drives it on the CPU through
// tests/native/mult_planes_shim.cpp.
//
// A first receipt's multiplicity is the number of in-arcs whose sender's
// frontier row holds the message.  Per 64-message word the counter keeps, for
// all 64 positions at once, that number in four count planes (plane b = bit b
// of the count modulo 16) and a sticky plane `sat` that is set exactly when the
// true count is 16 or more:
//   add a word x     ripple-carry increment of the positions of x; a carry out
//                    of plane 3 sets sat (the four planes wrap to 0 and go on
//                    counting modulo 16 -- sat is what is read from then on)
//   add four words   the same as four adds, as a carry-save tree (mult_add4)
//   merge a, b       bit-sliced add of the planes; sat = a.sat | b.sat | carry
//                    out.  With neither sticky both counts are < 16, so the
//                    carry out is exactly "sum >= 16"; with one sticky the sum
//                    is >= 16 whatever the planes hold.  Hence sat <=> true
//                    count >= 16 after any sequence of adds and merges, in any
//                    order: addition modulo 16 and OR are commutative and
//                    associative
//   eq(c), 1..15     ~sat & (planes spell c): positions whose count is exactly c
//   saturated        sat
// A lane of k_mult holds one counter per word of its row piece.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define GP_MULT_HD __host__ __device__ __forceinline__
#else
#define GP_MULT_HD inline
#endif

namespace gp {

constexpr int MULT_PLANES = 4;                  // count planes
constexpr int MULT_WORDS = MULT_PLANES + 1;     // ... and the sticky plane: words a counter takes
constexpr int MULT_SAT = 1 << MULT_PLANES;      // 16: counts from here on are one class
constexpr int MULT_BINS = MULT_SAT + 1;         // histogram bins 0 .. 16

struct MultCounter {
  uint64_t p[MULT_PLANES];
  uint64_t sat;
};

GP_MULT_HD MultCounter mult_zero() {
  MultCounter c;
#pragma unroll
  for (int b = 0; b < MULT_PLANES; ++b) c.p[b] = 0ull;
  c.sat = 0ull;
  return c;
}

// one more deliverer for every position of x
GP_MULT_HD void mult_add(MultCounter& c, uint64_t x) {
  uint64_t carry = x;
#pragma unroll
  for (int b = 0; b < MULT_PLANES; ++b) {
    const uint64_t t = c.p[b] & carry;
    c.p[b] ^= carry;
    carry = t;
  }
  c.sat |= carry;
}

// full adder, position by position: a + b + c = s + 2 k
GP_MULT_HD void mult_full_add(uint64_t a, uint64_t b, uint64_t c, uint64_t& s, uint64_t& k) {
  const uint64_t t = a ^ b;
  s = t ^ c;
  k = (a & b) | (t & c);
}

// four adds at once (a gather batch of k_mult), as a carry-save tree: two full
// adders take the four words and plane 0 to one bit of weight 1 and two of
// weight 2, a third takes those and plane 1 to weight 4, and a half adder each
// carries through planes 2 and 3 -- 20 word operations against 52 for four
// mult_add.  The count grows by at most 4 < 16, so one carry out of plane 3 is
// all there can be, and it is set exactly when the count reaches 16: the same
// counter as four mult_add in any order
GP_MULT_HD void mult_add4(MultCounter& c, uint64_t x0, uint64_t x1, uint64_t x2, uint64_t x3) {
  uint64_t s, k1, k2, k4, p0, p1;
  mult_full_add(x0, x1, x2, s, k1);
  mult_full_add(s, x3, c.p[0], p0, k2);
  mult_full_add(k1, k2, c.p[1], p1, k4);
  c.p[0] = p0;
  c.p[1] = p1;
  const uint64_t k8 = c.p[2] & k4;
  c.p[2] ^= k4;
  const uint64_t k16 = c.p[3] & k8;
  c.p[3] ^= k8;
  c.sat |= k16;
}

// a += b, position by position
GP_MULT_HD void mult_merge(MultCounter& a, const MultCounter& b) {
  uint64_t carry = 0ull;
#pragma unroll
  for (int k = 0; k < MULT_PLANES; ++k) {
    const uint64_t x = a.p[k], y = b.p[k];
    a.p[k] = x ^ y ^ carry;
    carry = (x & y) | (carry & (x ^ y));
  }
  a.sat |= b.sat | carry;
}

// positions whose count is exactly cnt (1 .. 15; 0 gives the untouched positions)
GP_MULT_HD uint64_t mult_eq(const MultCounter& c, int cnt) {
  uint64_t m = ~c.sat;
#pragma unroll
  for (int b = 0; b < MULT_PLANES; ++b) m &= ((cnt >> b) & 1) ? c.p[b] : ~c.p[b];
  return m;
}

// positions with 16 or more
GP_MULT_HD uint64_t mult_saturated(const MultCounter& c) { return c.sat; }

}  // namespace gp
