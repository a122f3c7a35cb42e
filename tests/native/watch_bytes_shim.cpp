// watch_bytes_shim.cpp -- test-only C wrapper around csrc/watch_bytes.h (plain
// C++, no HIP), compiled with g++ by tests/test_watch_bytes.py so the byte
// store of k_watch / k_watch_own (csrc/watch.hip) is checked on the CPU.
#include <cstdint>
#include <cstring>

#include "watch_bytes.h"

extern "C" {

unsigned long long wb_expand8(unsigned int bits) { return gp::watch_expand8(bits); }

unsigned long long wb_merge(unsigned long long old, unsigned long long mask8, unsigned int value) {
  return gp::watch_merge(old, mask8, value);
}

// one 16-byte piece of a record row the way the kernels take it: 16 message
// bits, both words read, merged and written back
void wb_put16(unsigned char* piece, unsigned int bits16, unsigned int value) {
  uint64_t lo, hi;
  std::memcpy(&lo, piece, 8);
  std::memcpy(&hi, piece + 8, 8);
  gp::watch_merge16(lo, hi, bits16, value);
  std::memcpy(piece, &lo, 8);
  std::memcpy(piece + 8, &hi, 8);
}

// a whole frontier row of `words` 64-bit words into a record row of 64 * words bytes
void wb_row(const unsigned long long* row, int words, unsigned int value, unsigned char* out) {
  for (int p = 0; p < 4 * words; ++p) {
    const unsigned int bits16 = (unsigned int)((row[p / 4] >> (16 * (p % 4))) & 0xFFFFu);
    if (bits16) wb_put16(out + 16 * p, bits16, value);
  }
}

}  // extern "C"
