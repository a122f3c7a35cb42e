// load_seg.h -- segment bookkeeping of the per-peer traffic pass (load.hip,
// DESIGN.md §3.10), as plain C++ so that the host tests drive the very code the
// kernel runs (tests/native/load_seg_check.cpp).
//
// A wave takes LOAD_ROWS consecutive receivers and streams their in-arcs as
// one flat sequence.  Receiver k contributes load_row_len arcs (none when it
// is down, past the end, or a hub: the hub items carry those), pre[] is the
// exclusive prefix of these lengths (pre[0] = 0, pre[LOAD_ROWS] = the wave's
// arcs) and beg[k] the receiver's first arc in the CSR.
//
// Flat positions are int64_t: 64 receivers below a hub_threshold of 2^30 can
// hold 2^36 arcs.  (32-bit positions for overlays under 2^32 arcs halve the
// search's compares and measured the same at C4: the pass waits for its
// probes and gathers, profiles/r12_load_cost.txt.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GP_LOAD_HD __host__ __device__ __forceinline__
#else
#define GP_LOAD_HD inline
#endif

namespace gp {

constexpr int LOAD_ROWS = 64;   // receivers per wave: one per lane

GP_LOAD_HD int64_t load_row_len(int64_t beg, int64_t end, bool up, int64_t hub_thr) {
  const int64_t d = end - beg;
  return up && d > 0 && d <= hub_thr ? d : 0;
}

// owner of flat position p, 0 <= p < pre[LOAD_ROWS]: the largest k with
// pre[k] <= p.  pre[k + 1] > p then, so the owner is never an empty row
GP_LOAD_HD int load_owner(const int64_t* pre, int64_t p) {
  int k = 0;
#pragma unroll
  for (int s = LOAD_ROWS / 2; s > 0; s >>= 1)
    if (pre[k + s] <= p) k += s;   // (k + s <= LOAD_ROWS - 1)
  return k;
}

// positions [p, p1) with owner(p) = k all lie in row k
GP_LOAD_HD bool load_chunk_in_row(const int64_t* pre, int k, int64_t p1) { return p1 <= pre[k + 1]; }

// CSR index of flat position p of row k
GP_LOAD_HD int64_t load_arc(const int64_t* pre, const int64_t* beg, int k, int64_t p) { return beg[k] + (p - pre[k]); }

}  // namespace gp
