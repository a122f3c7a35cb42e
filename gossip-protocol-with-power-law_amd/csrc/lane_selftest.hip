// lane_selftest.hip -- gp_selftest_lane_ops (include/gossip_capi.h): one small
// kernel evaluates every operation of lane_ops.h beside its `__shfl_xor` form
// on the same data and counts the lanes that differ.  Nothing else calls it.
#include "gp_internal.h"
#include "lane_ops.h"

namespace gp {

namespace {

constexpr int LS_OPS = GP_LANE_SELFTEST_OPS;
constexpr int LS_WAVES = 4;
constexpr int LS_PATTERNS = 68;   // zero, ones, one lane set (64), lane index, random
static_assert(LS_OPS == 32, "5 kinds x 5 sizes, 4 row widths, 3 packed layouts");

__device__ __forceinline__ u64 ls_mix(u64 z) {   // splitmix64's finalizer
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the value lane l of wave w holds in pattern p (tests/test_gpu_lane_ops.py forms the same)
__device__ __forceinline__ u64 ls_value(u64 seed, int p, int w, int l) {
  if (p == 0) return 0ull;
  if (p == 1) return ~0ull;
  if (p < 66) return l == p - 2 ? (ls_mix(seed ^ (u64)(w + 1)) | 1ull) : 0ull;
  if (p == 66) return (u64)l * 0x0000000100000001ull;
  return ls_mix(seed ^ ((u64)(w * 64 + l + 1) * 0xD1B54A32D192ED03ull));
}

// the LDS forms: the butterflies of gp_device.h
template <class OP, int N, class T>
__device__ __forceinline__ T shfl_group(T x) {
#pragma unroll
  for (int s = 1; s < N; s <<= 1) x = OP::op(x, (T)__shfl_xor(x, s));
  return x;
}
template <int LPR>
__device__ __forceinline__ u64 shfl_slots(u64 x, int from = LPR) {
#pragma unroll
  for (int s = 4; s < 64; s <<= 1)
    if (s >= from) x |= __shfl_xor(x, s);
  return x;
}

struct Tally {
  uint32_t bad[LS_OPS];
  u64 sum[LS_OPS];
};
template <int K, class T>
__device__ __forceinline__ void note(Tally& t, T got, T ref) {
  t.bad[K] += got != ref ? 1u : 0u;
  t.sum[K] += (u64)got;
}
// one kind (operation and type) at its five sizes: ops 5 KIND .. 5 KIND + 4
template <int KIND, class OP, class T>
__device__ __forceinline__ void kind(Tally& t, T x) {
  note<5 * KIND + 0>(t, lane::group<OP, 4>(x), shfl_group<OP, 4>(x));
  note<5 * KIND + 1>(t, lane::group<OP, 8>(x), shfl_group<OP, 8>(x));
  note<5 * KIND + 2>(t, lane::group<OP, 16>(x), shfl_group<OP, 16>(x));
  note<5 * KIND + 3>(t, lane::group<OP, 32>(x), shfl_group<OP, 32>(x));
  note<5 * KIND + 4>(t, lane::wave<OP>(x), shfl_group<OP, 64>(x));
}

__global__ __launch_bounds__(64 * LS_WAVES) void k_lane_selftest(u64 seed, u64* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Tally t;
#pragma unroll
  for (int k = 0; k < LS_OPS; ++k) {
    t.bad[k] = 0u;
    t.sum[k] = 0ull;
  }
  // (wave-uniform control flow throughout: every lane is active in every operation)
#pragma unroll 1
  for (int p = 0; p < LS_PATTERNS; ++p) {
    const u64 x = ls_value(seed, p, w, lane);
    kind<0, lane::Add>(t, (uint32_t)x);
    kind<1, lane::Add>(t, x);
    kind<2, lane::Xor>(t, x);
    kind<3, lane::Or>(t, x);
    kind<4, lane::Or>(t, (uint32_t)(x & 1ull));   // (bool: lane_ops.h reduces it as a word)
    note<25>(t, lane::slots_or<32>(x), shfl_slots<32>(x));
    note<26>(t, lane::slots_or<16>(x), shfl_slots<16>(x));
    note<27>(t, lane::slots_or<8>(x), shfl_slots<8>(x));
    note<28>(t, lane::slots_or<4>(x), shfl_slots<4>(x));
#pragma unroll 1
    for (int sh = 5; sh >= 3; --sh) {   // the packed gather's run-time layouts
      const u64 got = lane::slots_or_sh(x, sh), ref = shfl_slots<8>(x, 1 << sh);
      if (sh == 5) note<29>(t, got, ref);
      else if (sh == 4) note<30>(t, got, ref);
      else note<31>(t, got, ref);
    }
  }
#pragma unroll
  for (int k = 0; k < LS_OPS; ++k) {
    if (t.bad[k]) atomicAdd(out + k, (u64)t.bad[k]);
    atomicAdd(out + LS_OPS + k, t.sum[k]);
  }
}

}  // namespace

}  // namespace gp

extern "C" int gp_selftest_lane_ops(int device, uint64_t seed, uint64_t* out_mismatches) {
  using namespace gp;
  if (!out_mismatches) return set_error(GP_EINVAL, "null out_mismatches");
  int n = 0;
  GP_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return set_error(GP_EINVAL, "no such device");
  GP_HIP(hipSetDevice(device));
  u64* d = nullptr;
  GP_HIP(hipMalloc(&d, 2 * LS_OPS * sizeof(u64)));
  hipError_t e = hipMemset(d, 0, 2 * LS_OPS * sizeof(u64));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_lane_selftest, dim3(1), dim3(64 * LS_WAVES), 0, 0, (u64)seed, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out_mismatches, d, 2 * LS_OPS * sizeof(u64), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return set_error(GP_EHIP, std::string("lane-ops self-test: ") + hipGetErrorString(e));
  return 0;
}
