// watch_bytes.h -- the byte store of the watched peers' record (watch.hip,
// DESIGN.md §3.17), plain C++ for host and device: tests/test_watch_bytes.py
// drives it on the CPU through tests/native/watch_bytes_shim.cpp.
//
// A record row holds one byte per message: 255 = never, else the receipt round.
// Message 64 w + b is bit b of word w of a frontier row and byte 64 w + b of the
// record row, so 8 message bits map to one little-endian u64 of the record.
// Every byte starts at 0xFF and is written at most once per run with a value
// <= 254 (a second write can only repeat the value), so a store needs no test of
// what is there: with mask8 = 0xFF in the bytes whose bit is set,
//
//   p' = p & (~mask8 | value * 0x0101010101010101)
//
// leaves the bytes outside the mask alone and turns 0xFF -- or the value -- into
// the value inside it: idempotent, and independent of the old content of the
// bytes it writes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define GP_WATCH_HD __host__ __device__ __forceinline__
#else
#define GP_WATCH_HD inline
#endif

namespace gp {

constexpr uint8_t WATCH_NEVER = 0xFF;
constexpr uint64_t WATCH_ONES = 0x0101010101010101ull;

// 8 bits -> 8 bytes, branch-free: byte i of the result is 0xFF iff bit i of
// `bits` (< 256) is set.  The product copies the 8 bits into every byte (no
// carries: bits < 256), the AND keeps bit i in byte i, so a byte is 0 or
// 1 << i <= 0x80; adding 0x7F raises bit 7 of exactly the nonzero bytes and
// never carries into the next one; bit 7 times 0xFF fills its byte
GP_WATCH_HD uint64_t watch_expand8(uint32_t bits) {
  const uint64_t sel = ((uint64_t)(bits & 0xFFu) * WATCH_ONES) & 0x8040201008040201ull;
  const uint64_t top = (sel + 0x7F7F7F7F7F7F7F7Full) & 0x8080808080808080ull;
  return (top >> 7) * 0xFFull;
}

// the record word after `value` went into the bytes of mask8 (header)
GP_WATCH_HD uint64_t watch_merge(uint64_t old, uint64_t mask8, uint32_t value) {
  return old & (~mask8 | (uint64_t)(value & 0xFFu) * WATCH_ONES);
}

// 16 message bits -> the two record words they cover
GP_WATCH_HD void watch_merge16(uint64_t& lo, uint64_t& hi, uint32_t bits16, uint32_t value) {
  lo = watch_merge(lo, watch_expand8(bits16 & 0xFFu), value);
  hi = watch_merge(hi, watch_expand8((bits16 >> 8) & 0xFFu), value);
}

}  // namespace gp
