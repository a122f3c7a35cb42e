// lane_ops.h -- cross-lane reductions in registers.  The
// `__shfl_xor` butterflies of gp_device.h compile to ds_bpermute_b32: an LDS
// instruction with a lane-address VGPR and an lgkmcnt wait per level.  gfx950
// does the same in the VALU: DPP row operations inside a 16-lane row,
// v_permlane16_swap / v_permlane32_swap across rows and halves, v_readlane for
// a wave-uniform result.  Sums, xors and ORs of integers are order-free, so
// every result is bit for bit the butterfly's.
//
// EVERY operation here needs all 64 lanes of the wave active: a DPP read or a
// swap takes nothing from an inactive lane.  A call under divergent control
// flow keeps the LDS shuffle.  Only builtins, no inline assembly: the hazard
// recogniser places the wait states between a VALU write and a swap / readlane.
//
// GP_LANE_OPS: 1 = the pull family (pull.hip, hub.hip) uses
// these; 0 = it compiles the LDS shuffles, as every other unit does.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#ifndef GP_LANE_OPS
#define GP_LANE_OPS 1
#endif

namespace gp {
namespace lane {

typedef unsigned long long u64;
constexpr bool ON = GP_LANE_OPS != 0;

// DPP controls (valid on every gfx9-family target)
constexpr int QUAD_XOR1 = 0xB1;          // quad_perm:[1,0,3,2]  lane ^ 1
constexpr int QUAD_XOR2 = 0x4E;          // quad_perm:[2,3,0,1]  lane ^ 2
constexpr int ROW_ROR4 = 0x124;          // row_ror:4   the lane 4 away in its row, cyclically
constexpr int ROW_ROR8 = 0x128;          // row_ror:8   lane ^ 8
constexpr int ROW_HALF_MIRROR = 0x141;   // lane ^ 7: the other quad of an octet, once quads are uniform
constexpr int ROW_MIRROR = 0x140;        // lane ^ 15: the other octet of a row, once octets are uniform

struct Add {
  template <class T> static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};
struct Xor {
  template <class T> static __device__ __forceinline__ T op(T a, T b) { return a ^ b; }
};
struct Or {
  template <class T> static __device__ __forceinline__ T op(T a, T b) { return a | b; }
};

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ u64 dpp(u64 x) {
  return ((u64)dpp<CTRL>((uint32_t)(x >> 32)) << 32) | (u64)dpp<CTRL>((uint32_t)x);
}

// x[l] op x[l ^ 16] in every lane: the swap exchanges the odd rows of its
// first operand with the even rows of its second, so with both operands x one
// result holds the lane's own value and the other its partner's, whichever row
template <class OP>
__device__ __forceinline__ uint32_t xor16(uint32_t x) {
  const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
  return OP::op((uint32_t)r[0], (uint32_t)r[1]);
}
// x[l] op x[l ^ 32]: the same with the wave's halves
template <class OP>
__device__ __forceinline__ uint32_t xor32(uint32_t x) {
  const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return OP::op((uint32_t)r[0], (uint32_t)r[1]);
}
template <class OP>
__device__ __forceinline__ u64 xor16(u64 x) {
  const auto lo = __builtin_amdgcn_permlane16_swap((uint32_t)x, (uint32_t)x, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((uint32_t)(x >> 32), (uint32_t)(x >> 32), false, false);
  return OP::op(((u64)(uint32_t)hi[0] << 32) | (u64)(uint32_t)lo[0], ((u64)(uint32_t)hi[1] << 32) | (u64)(uint32_t)lo[1]);
}
template <class OP>
__device__ __forceinline__ u64 xor32(u64 x) {
  const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)x, (uint32_t)x, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)(x >> 32), (uint32_t)(x >> 32), false, false);
  return OP::op(((u64)(uint32_t)hi[0] << 32) | (u64)(uint32_t)lo[0], ((u64)(uint32_t)hi[1] << 32) | (u64)(uint32_t)lo[1]);
}

// Reduction over aligned groups of N = 4, 8, 16, 32 or 64 lanes; every lane
// ends with its group's result.  All 64 lanes active.
template <class OP, int N, class T>
__device__ __forceinline__ T group(T x) {
  static_assert(N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "aligned groups of 4 .. 64 lanes");
  x = OP::op(x, dpp<QUAD_XOR1>(x));
  x = OP::op(x, dpp<QUAD_XOR2>(x));
  if constexpr (N >= 8) x = OP::op(x, dpp<ROW_HALF_MIRROR>(x));
  if constexpr (N >= 16) x = OP::op(x, dpp<ROW_MIRROR>(x));
  if constexpr (N >= 32) x = xor16<OP>(x);
  if constexpr (N >= 64) x = xor32<OP>(x);
  return x;
}

__device__ __forceinline__ uint32_t read_lane(uint32_t x, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)x, l);
}
__device__ __forceinline__ u64 read_lane(u64 x, int l) {
  return ((u64)read_lane((uint32_t)(x >> 32), l) << 32) | (u64)read_lane((uint32_t)x, l);
}

// Reduction over the whole wave, wave-uniform (SGPRs): the four rows reduce
// in the VALU, their results meet in the SALU.  All 64 lanes active.
template <class OP, class T>
__device__ __forceinline__ T wave(T x) {
  x = group<OP, 16>(x);
  return OP::op(OP::op(read_lane(x, 0), read_lane(x, 16)), OP::op(read_lane(x, 32), read_lane(x, 48)));
}

template <int N> __device__ __forceinline__ uint32_t group_sum_u32(uint32_t x) { return group<Add, N>(x); }
template <int N> __device__ __forceinline__ u64 group_sum_u64(u64 x) { return group<Add, N>(x); }
template <int N> __device__ __forceinline__ u64 group_xor_u64(u64 x) { return group<Xor, N>(x); }
template <int N> __device__ __forceinline__ u64 group_or_u64(u64 x) { return group<Or, N>(x); }
template <int N> __device__ __forceinline__ bool group_or_bool(bool x) { return group<Or, N>(x ? 1u : 0u) != 0u; }
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) { return wave<Add>(x); }
__device__ __forceinline__ u64 wave_sum_u64(u64 x) { return wave<Add>(x); }
__device__ __forceinline__ u64 wave_xor_u64(u64 x) { return wave<Xor>(x); }
__device__ __forceinline__ u64 wave_or_u64(u64 x) { return wave<Or>(x); }
__device__ __forceinline__ bool wave_or_bool(bool x) { return wave<Or>(x ? 1u : 0u) != 0u; }

// OR over the row slots of a wave: lanes LPR, 2 LPR, .. 32 apart combine, every
// lane ends with the OR of its residue class modulo LPR (LPR = 32, 16, 8, 4:
// rows of W = 64, 32, 16, 8 words).  Inside a row the rotations walk the
// class (l, l + 4, l + 8, l + 12 after row_ror:4 and row_ror:8): a cyclic
// order, which an OR does not see.  All 64 lanes active.
template <int LPR>
__device__ __forceinline__ u64 slots_or(u64 x) {
  static_assert(LPR == 4 || LPR == 8 || LPR == 16 || LPR == 32, "row slots of 4 .. 32 lanes");
  if constexpr (LPR <= 4) x |= dpp<ROW_ROR4>(x);
  if constexpr (LPR <= 8) x |= dpp<ROW_ROR8>(x);
  if constexpr (LPR <= 16) x = xor16<Or>(x);
  return xor32<Or>(x);
}
// the same for a run-time slot width of 1 << sh lanes (sh = 3, 4, 5; wave-uniform)
__device__ __forceinline__ u64 slots_or_sh(u64 x, int sh) {
  if (sh <= 3) x |= dpp<ROW_ROR8>(x);
  if (sh <= 4) x = xor16<Or>(x);
  return xor32<Or>(x);
}

}  // namespace lane
}  // namespace gp
