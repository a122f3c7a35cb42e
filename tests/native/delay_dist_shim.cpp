// delay_dist_shim.cpp -- test-only C wrapper around csrc/delay_dist.h (plain
// C++, no HIP), compiled with g++ by tests/test_delay_dist.py so the
// inject-round masks, the per-round window and the packed row arithmetic of
// k_delay_dist (csrc/delay_dist.hip) are checked on the CPU.
#include <cstdint>
#include <cstring>

#include "delay_dist.h"

extern "C" {

int dd_bins() { return gp::DELAY_DIST_BINS; }
int dd_window_size() { return gp::DELAY_DIST_WINDOW; }

// the messages of word w with inject round t (planes as delay_build_planes makes them)
unsigned long long dd_eq_mask(const unsigned long long* planes, int words, int w, unsigned int t) {
  uint64_t p[gp::DELAY_PLANES];
  for (int b = 0; b < gp::DELAY_PLANES; ++b) p[b] = planes[b * words + w];
  return gp::delay_eq_mask(p, t);
}

// the table's presence set: 4 words
void dd_present(const unsigned char* inject, int m, unsigned long long* out) {
  const gp::DelayPresent s = gp::delay_present_build(inject, m);
  for (int i = 0; i < 4; ++i) out[i] = s.w[i];
}

// the window of receipt round rr: returns n, fills t[14] and *dmask
int dd_window(const unsigned char* inject, int m, unsigned int rr, unsigned char* t, unsigned int* dmask) {
  const gp::DelayWindow win = gp::delay_window(gp::delay_present_build(inject, m), rr);
  std::memcpy(t, win.t, sizeof(win.t));
  *dmask = win.dmask;
  return (int)win.n;
}

unsigned long long dd_pack(int d, unsigned int count) { return gp::dist_pack(d, count); }
void dd_add(unsigned long long* row, int d, unsigned int count) {
  gp::dist_add(reinterpret_cast<uint64_t*>(row), d, count);
}
unsigned int dd_unpack(const unsigned long long* row, int d) {
  return gp::dist_unpack(reinterpret_cast<const uint64_t*>(row), d);
}

// one new row of receipt round rr the way k_delay_dist takes it: per word the
// window's masks and dist_word, the words' packed shares added as the lanes'
// reduction adds them, then the packed add into the record row `out` (16 u16 in
// memory order, column 0 untouched)
void dd_row(const unsigned long long* row, const unsigned char* inject, int m, int words, unsigned int rr,
            unsigned short* out) {
  uint64_t planes[gp::DELAY_PLANES * 64];
  gp::delay_build_planes(inject, m, words, planes);
  const gp::DelayWindow win = gp::delay_window(gp::delay_present_build(inject, m), rr);
  gp::DistRow sum{};
  for (int w = 0; w < words; ++w) {
    uint64_t p[gp::DELAY_PLANES], eq[gp::DELAY_DIST_WINDOW];
    for (int b = 0; b < gp::DELAY_PLANES; ++b) p[b] = planes[b * words + w];
    gp::dist_eq_masks(p, rr, win.dmask, eq);
    gp::DistRow acc{};
    gp::dist_word((uint64_t)row[w], eq, win.dmask, acc);
    for (int i = 0; i < 2 * gp::DELAY_DIST_WORDS; ++i) sum.h[i] += acc.h[i];
  }
  uint32_t rec[2 * gp::DELAY_DIST_WORDS];
  std::memcpy(rec, out, sizeof(rec));
  for (int i = 0; i < 2 * gp::DELAY_DIST_WORDS; ++i) rec[i] += sum.h[i];
  std::memcpy(out, rec, sizeof(rec));
}

}  // extern "C"
