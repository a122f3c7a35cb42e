// delay_dist.h -- arithmetic of the per-peer delay distributions
// (delay_dist.hip), plain C++ for host and device:
// tests/test_delay_dist.py drives it on the CPU through
// tests/native/delay_dist_shim.cpp.
//
// delay_dist[v][d] counts v's receipts with min(delay, 15) = d, so a new row of
// receipt round rr needs, per 64-message word x, the number of x's bits per
// inject round t = rr - d.  With the 8 inject-round planes of the word
// (delay_planes.h) the messages of inject round t are one mask,
//   eq(t) = AND_b (bit b of t ? P_b : ~P_b),
// and only the inject rounds the table holds need one: the presence set of the
// table (256 bits, built at gp_reset) gives the window of a round, the present t
// with rr - 14 <= t <= rr - 1.  Later inject rounds are not injected yet, older
// ones land in column 15 as popc(x) minus the listed counts.
//
// A row of the record is 16 u16 = four u64 words of four 16-bit fields (field
// d & 3 of word d >> 2).  A vertex receives each message once, so a field never
// exceeds m <= 4096 over a run and adding such words never carries from one
// field into the next: the commit is a plain add of packed words.
#pragma once
#include <cstdint>

#include "delay_planes.h"

namespace gp {

constexpr int DELAY_DIST_BINS = 16;                      // columns of a row: delays 0 .. 14, 15 or more
constexpr int DELAY_DIST_WINDOW = DELAY_DIST_BINS - 2;   // delays with a mask of their own: 1 .. 14
constexpr int DELAY_DIST_WORDS = DELAY_DIST_BINS / 4;    // packed u64 words of a row

// the messages of a word whose inject round is t (p: the 8 plane words of the
// word position; bits past m are clear in every plane, so they match t = 0:
// a row never has them set)
GP_DELAY_HD uint64_t delay_eq_mask(const uint64_t* p, uint32_t t) {
  uint64_t m = ~0ull;
#pragma unroll
  for (int b = 0; b < DELAY_PLANES; ++b) m &= ((t >> b) & 1u) ? p[b] : ~p[b];
  return m;
}

// the inject rounds a table holds: bit t & 63 of word t >> 6
struct DelayPresent {
  uint64_t w[4];
};

inline DelayPresent delay_present_build(const uint8_t* inject, int32_t m) {
  DelayPresent s{{0ull, 0ull, 0ull, 0ull}};
  for (int32_t k = 0; k < m; ++k) s.w[inject[k] >> 6] |= 1ull << (inject[k] & 63);
  return s;
}

GP_DELAY_HD bool delay_present(const DelayPresent& s, int32_t t) {
  return t >= 0 && t < 256 && ((s.w[t >> 6] >> (t & 63)) & 1ull) != 0ull;
}

// the window of receipt round rr = round + 1: the present inject rounds t with
// rr - 14 <= t <= rr - 1, newest first, each with the delay d = rr - t; dmask
// has bit d set for every listed t (what k_delay_dist walks: its fields are
// then compile-time positions)
struct DelayWindow {
  uint32_t n;                      // listed inject rounds, <= 14
  uint32_t dmask;                  // bits 1 .. 14
  uint8_t t[DELAY_DIST_WINDOW];    // t[i], i < n (the rest 0)
};

inline DelayWindow delay_window(const DelayPresent& s, uint32_t rr) {
  DelayWindow win{};
  for (int d = 1; d <= DELAY_DIST_WINDOW; ++d) {
    const int32_t t = (int32_t)rr - d;
    if (!delay_present(s, t)) continue;
    win.t[win.n++] = (uint8_t)t;
    win.dmask |= 1u << d;
  }
  return win;
}

// a row in registers: 8 u32 of two fields each (field d & 1 of half d >> 1, the
// memory layout of four u64 of four fields on a little-endian machine)
struct DistRow {
  uint32_t h[2 * DELAY_DIST_WORDS];
};

// `count` receipts of delay column d (d < 16, count < 2^16) as a packed u64 of
// word d >> 2
GP_DELAY_HD uint64_t dist_pack(int d, uint32_t count) { return (uint64_t)count << (16 * (d & 3)); }

// the packed add: no carry leaves a field while every field stays < 2^16
GP_DELAY_HD void dist_add(uint64_t* row, int d, uint32_t count) { row[d >> 2] += dist_pack(d, count); }

GP_DELAY_HD uint32_t dist_unpack(const uint64_t* row, int d) {
  return (uint32_t)(row[d >> 2] >> (16 * (d & 3))) & 0xFFFFu;
}

// one word of a new row of receipt round rr: eq[d - 1] = delay_eq_mask(p, rr - d)
// for the bits d of dmask.  Adds the word's receipts to acc, column 0 never
template <int D>
GP_DELAY_HD void dist_word_step(uint64_t x, const uint64_t* eq, uint32_t dmask, DistRow& acc, uint32_t& listed) {
  if ((dmask >> D) & 1u) {   // (wave-uniform on the device)
    const uint32_t c = delay_popc(x & eq[D - 1]);
    acc.h[D >> 1] += c << (16 * (D & 1));
    listed += c;
  }
  if constexpr (D < DELAY_DIST_WINDOW) dist_word_step<D + 1>(x, eq, dmask, acc, listed);
}

GP_DELAY_HD void dist_word(uint64_t x, const uint64_t* eq, uint32_t dmask, DistRow& acc) {
  uint32_t listed = 0;
  dist_word_step<1>(x, eq, dmask, acc, listed);
  acc.h[(DELAY_DIST_BINS - 1) >> 1] += (delay_popc(x) - listed) << 16;   // 15 rounds or later
}

// the masks of a word position for a window (eq[d - 1] = 0 where d is not listed)
template <int D>
GP_DELAY_HD void dist_eq_step(const uint64_t* p, uint32_t rr, uint32_t dmask, uint64_t* eq) {
  eq[D - 1] = ((dmask >> D) & 1u) ? delay_eq_mask(p, rr - D) : 0ull;
  if constexpr (D < DELAY_DIST_WINDOW) dist_eq_step<D + 1>(p, rr, dmask, eq);
}

GP_DELAY_HD void dist_eq_masks(const uint64_t* p, uint32_t rr, uint32_t dmask, uint64_t* eq) {
  dist_eq_step<1>(p, rr, dmask, eq);
}

}  // namespace gp
