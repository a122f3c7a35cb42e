// delay_planes.h -- bit-sliced inject-round arithmetic of the per-peer receipt
// delays (delay.hip), plain C++ for host and device:
// tests/test_delay_planes.py drives it on the CPU through
// tests/native/delay_planes_shim.cpp.
//
// A receipt's delay is its receipt round minus the message's inject round, so
// a new row's share of delay_sum / delay_max needs, per 64-message word x, the
// sum and the minimum of the inject rounds of x's set bits.  Inject rounds are
// 8-bit numbers (<= 253, gp_set_messages); plane b of word w is the mask of the
// word's messages whose inject round has bit b set:
//   sum = sum_b popc(x & P_b) << b          (8 and + popc, no per-bit loop)
//   min = descent from bit 7: keep the candidates with bit b clear when there
//         are any, else bit b of the minimum is 1
// A lane of k_delay holds the 8 plane words of its word position in registers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define GP_DELAY_HD __host__ __device__ __forceinline__
#else
#define GP_DELAY_HD inline
#endif

namespace gp {

constexpr int DELAY_PLANES = 8;            // bits of an inject round
constexpr uint32_t DELAY_NO_MIN = 0xFFFFu; // delay_inject_min of an empty word: above every round

GP_DELAY_HD uint32_t delay_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}

// planes[b * words + w] for the table inject[0 .. m) (bits past m stay clear)
inline void delay_build_planes(const uint8_t* inject, int32_t m, int32_t words, uint64_t* planes) {
  for (int32_t t = 0; t < DELAY_PLANES * words; ++t) planes[t] = 0ull;
  for (int32_t k = 0; k < m; ++k)
    for (int b = 0; b < DELAY_PLANES; ++b)
      if ((inject[k] >> b) & 1u) planes[b * words + (k >> 6)] |= 1ull << (k & 63);
}

// the table's one inject round, or -1 when its messages start in different rounds
inline int32_t delay_uniform_round(const uint8_t* inject, int32_t m) {
  if (m < 1) return -1;
  for (int32_t k = 1; k < m; ++k)
    if (inject[k] != inject[0]) return -1;
  return (int32_t)inject[0];
}

// p: the 8 plane words of x's word position.  Sum of the inject rounds of x's bits
GP_DELAY_HD uint32_t delay_inject_sum(uint64_t x, const uint64_t* p) {
  uint32_t s = 0;
#pragma unroll
  for (int b = 0; b < DELAY_PLANES; ++b) s += delay_popc(x & p[b]) << b;
  return s;
}

// ... and their minimum (DELAY_NO_MIN for x = 0)
GP_DELAY_HD uint32_t delay_inject_min(uint64_t x, const uint64_t* p) {
  if (x == 0ull) return DELAY_NO_MIN;
  uint64_t cand = x;
  uint32_t mn = 0;
#pragma unroll
  for (int b = DELAY_PLANES - 1; b >= 0; --b) {
    const uint64_t t = cand & ~p[b];
    if (t) cand = t;
    else mn |= 1u << b;
  }
  return mn;
}

// degree bin of gp_read_delay_bins: 0 for deg <= 1, else floor(log2(deg))
GP_DELAY_HD int delay_bin(int64_t deg) {
  return deg <= 1 ? 0 : 63 - __builtin_clzll((unsigned long long)deg);
}

}  // namespace gp
