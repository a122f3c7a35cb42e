// Stand-alone check of csrc/load_seg.h: the owner search and segment
// bookkeeping of the per-peer traffic pass (csrc/load.hip k_load), walked the
// way the kernel's wave walks them -- 64 receivers, their in-arcs as one flat
// sequence in chunks of 64 positions, every lane searching its owner (lanes
// past the end the last position's), a chunk inside one row reduced as a
// whole, the others lane by lane -- against a plain row-by-row sum.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I <csrc> load_seg_check.cpp && ./a.out
//
// Exit status 0 and "load_seg ok" when every case matches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "load_seg.h"

using namespace gp;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

struct Case {
  std::vector<int64_t> row_ptr;   // [n + 1]
  std::vector<int32_t> col;
  std::vector<uint32_t> x;
  std::vector<uint8_t> down;
  int64_t hub_thr;
};

// one wave's receivers [v0, v0 + 64): acc[k] as k_load leaves it; *uniform
// counts the chunks that took the one-row path
typedef int64_t P;   // flat positions, as k_load's

static void wave(const Case& c, int64_t v0, uint64_t* acc, int64_t* uniform) {
  const int64_t n = (int64_t)c.row_ptr.size() - 1;
  std::vector<P> pre(LOAD_ROWS + 1);   // exact sizes: the sanitizer sees an overrun
  std::vector<int64_t> beg(LOAD_ROWS);
  pre[0] = 0;
  for (int k = 0; k < LOAD_ROWS; ++k) {
    const int64_t v = v0 + k;
    int64_t b = 0, e = 0;
    bool up = false;
    if (v < n) {
      b = c.row_ptr[v];
      e = c.row_ptr[v + 1];
      up = !c.down[v];
    }
    beg[k] = b;
    pre[k + 1] = pre[k] + (P)load_row_len(b, e, up, c.hub_thr);
    acc[k] = 0;
  }
  const P total = pre[LOAD_ROWS];
  for (P pc = 0; pc < total; pc += 64) {
    const P p1 = pc + 64 < total ? pc + 64 : total;
    const int o0 = load_owner(pre.data(), pc);
    const bool one = load_chunk_in_row(pre.data(), o0, p1);
    if (one) ++*uniform;
    uint64_t sum = 0;
    for (int lane = 0; lane < 64; ++lane) {
      const P p = pc + (P)lane;
      const int o = load_owner(pre.data(), p < p1 - 1 ? p : p1 - 1);
      if (one && o != o0) {
        fprintf(stderr, "one-row chunk at %lld: lane %d has owner %d, lane 0 %d\n", (long long)pc, lane, o, o0);
        exit(1);
      }
      if (p >= total) continue;
      if (o < 0 || o >= LOAD_ROWS || !(pre[o] <= p && p < pre[o + 1])) {
        fprintf(stderr, "owner of %lld is %d\n", (long long)p, o);
        exit(1);
      }
      const int64_t j = load_arc(pre.data(), beg.data(), o, p);
      if (j < c.row_ptr[v0 + o] || j >= c.row_ptr[v0 + o + 1]) {
        fprintf(stderr, "arc %lld outside row %lld\n", (long long)j, (long long)(v0 + o));
        exit(1);
      }
      const uint32_t val = c.x.at((size_t)c.col.at((size_t)j));
      if (one) sum += val;
      else acc[o] += val;
    }
    if (one) acc[o0] += sum;
  }
}

static int64_t run(const Case& c) {
  const int64_t n = (int64_t)c.row_ptr.size() - 1;
  int64_t uniform = 0;
  for (int64_t v0 = 0; v0 < n; v0 += LOAD_ROWS) {
    uint64_t acc[LOAD_ROWS];
    wave(c, v0, acc, &uniform);
    for (int k = 0; k < LOAD_ROWS; ++k) {
      const int64_t v = v0 + k;
      uint64_t exp = 0;
      if (v < n && !c.down[v] && c.row_ptr[v + 1] - c.row_ptr[v] <= c.hub_thr)
        for (int64_t j = c.row_ptr[v]; j < c.row_ptr[v + 1]; ++j) exp += c.x[(size_t)c.col[(size_t)j]];
      if (acc[k] != exp) {
        fprintf(stderr, "receiver %lld: %llu != %llu\n", (long long)v, (unsigned long long)acc[k],
                (unsigned long long)exp);
        exit(1);
      }
    }
  }
  return uniform;
}

// rows of the given lengths; columns and x random, every `down_every`-th vertex down
static Case make(const std::vector<int64_t>& len, int64_t hub_thr, int down_every) {
  Case c;
  const size_t n = len.size();
  c.hub_thr = hub_thr;
  c.row_ptr.assign(n + 1, 0);
  for (size_t v = 0; v < n; ++v) c.row_ptr[v + 1] = c.row_ptr[v] + len[v];
  c.col.resize((size_t)c.row_ptr[n]);
  for (auto& u : c.col) u = (int32_t)(rnd() % n);
  c.x.resize(n);
  for (auto& t : c.x) t = (uint32_t)(rnd() % 4097);   // 0 .. 4096 messages
  c.down.assign(n, 0);
  if (down_every > 0)
    for (size_t v = 0; v < n; v += (size_t)down_every) c.down[v] = 1;
  return c;
}

int main() {
  // fewer receivers than one wave; empty rows at both ends
  run(make({0, 3, 0, 0, 1}, 64, 0));
  run(make({0, 0, 0}, 64, 0));
  // every row the same short length: chunks span many rows
  for (int64_t d : {1, 2, 7, 63, 64, 65}) run(make(std::vector<int64_t>(130, d), 1 << 30, 0));
  // one long row among short ones, hubs skipped or walked
  for (int64_t thr : {(int64_t)64, (int64_t)1 << 30}) {
    std::vector<int64_t> len(200, 2);
    len[0] = 1000;
    len[63] = 129;
    len[64] = 64;
    len[199] = 5000;
    Case c = make(len, thr, 0);
    const int64_t uniform = run(c);
    if (thr > 5000 && uniform < 5000 / 64 - 1) {
      fprintf(stderr, "the long rows took the per-lane path (%lld one-row chunks)\n", (long long)uniform);
      return 1;
    }
  }
  // random power-law-ish lengths, every third vertex down, sizes around the wave
  for (int n : {1, 63, 64, 65, 127, 128, 129, 1000}) {
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<int64_t> len((size_t)n);
      for (auto& d : len) {
        const uint64_t r = rnd() % 1000;
        d = r < 300 ? 0 : r < 900 ? (int64_t)(rnd() % 8) : r < 990 ? (int64_t)(rnd() % 200) : (int64_t)(rnd() % 3000);
      }
      run(make(len, rep & 1 ? 64 : 1 << 30, rep & 2 ? 3 : 0));
    }
  }
  printf("load_seg ok\n");
  return 0;
}
