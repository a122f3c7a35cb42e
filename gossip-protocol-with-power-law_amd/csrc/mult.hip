// mult.hip -- delivery multiplicity: how many
// in-neighbours delivered each first receipt.  With frontier_r(u) u's frontier
// after L_r and I_r and new_r(v) the bits v first receives in E_r, for every
// k in new_r(v)
//
//   mult_r(v, k) = #{ arcs j of row v of the in-CSR : k in frontier_r(col[j]) }
//
// (parallel arcs count separately, >= 1), and the record keeps
//
//   mult_hist[c]  receipts with exactly c deliverers (c = 1 .. 15), 16 or more
//                 in bin 16 (bin 0, the injections, comes from the rounds'
//                 counters at the read)
//   sole_recv[v]  v's receipts with one deliverer
//   sole_sent[u]  the receipts, over u's out-arcs, u alone delivered
//
// every round, at the end of round_launch (driver.hip) beside
// fresh_count_round, after the event that ends expand_ms.  The operands are
// fresh.hip's: d_frx[cur ^ 1] behind fpop[cur ^ 1] != 0 is new_r, d_frx[cur]
// behind fpop[cur] != 0 is frontier_r; a row behind a zero guard is stale and
// is never loaded, which is all liveness needs (k_churn zeroed a crashed
// sender's guard).
//
// k_mult is k_fresh's gather with another multiply: one-wave blocks, 64
// receivers each, one coalesced load of the guard words and a ballot.  A live
// receiver keeps its new row in registers (Geo<W>: 16 B per lane, every row
// slot the same pieces) and the wave walks its in-list 64 arcs at a time --
// column ids, the neighbours' guards, the live ones staged in LDS, their rows
// gathered MULT_RIF wave-instructions in flight; a lane whose own piece is zero
// loads nothing.  Each gathered piece, masked by the receiver's, is one add to
// the lane's bit-sliced counter (mult_planes.h: 4 count planes and a sticky
// "16 or more" plane per word, 20 VGPRs), a batch of four as one carry-save
// add.  After the list the Geo<W>::RPI row slots hold partial counts of the
// same positions: a butterfly of bit-sliced adds over shuffles leaves every
// lane with the row's counter.  The lanes of slot 0 add the popcounts of their
// first word's "equals c" masks, the lanes of slot 1 their second word's, to 16
// per-lane u32 bins that live in LDS for the whole block (a column per lane; 64
// receivers x 64 bits: no overflow), reduced over the wave once at its end and added to one of
// MULT_SLOTS copies of the device histogram -- at most 16 atomics per 64
// receivers, spread over 256 x 16 addresses.  popc(sole) goes to sole_recv[v],
// lane = vertex, one plain read-modify-write per block (this wave is the only
// writer of its non-hub receivers).
//
// The senders' side needs the finished mask, so it is a second walk -- only of
// a receiver with at least one sole bit, with the sole mask in the place of the
// own row (a lane without sole bits loads nothing): popc(row & sole) per arc,
// reduced over the row's lanes, one 64-bit atomicAdd to sole_sent[u], as
// fresh's SCATTER form.  Exactly one arc holds each sole bit, so the adds of a
// receiver sum to popc(sole).  Integer adds commute: the totals are
// deterministic.  The in-CSR alone is walked, so a directed overlay needs
// nothing else.
//
// Receivers above hub_threshold are split over the HubItem table; counts of
// one position in different items must be added before "equals c" means
// anything.  k_mult_hub: one wave per item, the same walk, the item's counter
// (row slots merged) stored to scratch [item][5][W].  k_mult_hub_final: one
// wave per hub merges its items' counters, Geo<W>::RPI items per step, then the
// row slots; tallies the histogram and sole_recv[v]; stores the sole mask
// [hub][W].  k_mult_hub_sole: one wave per item walks its arcs with the hub's
// merged mask, and returns at once when the mask is empty.  All three skip a
// hub whose guard is zero, so stale scratch is never read.
//
// Widths.  A position's count is exact below 16 and sticky from 16 on
// (mult_planes.h argues the merge).  A receiver adds at most 4096 to
// sole_recv per run (each message is first received once): u32.  sole_sent[u]
// is bounded by out-degree x 4096 < 2^36: u64, as fresh_sent.  The per-lane
// bins: 4096 per block at most; their wave sums < 2^18.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "delay_planes.h"
#include "gp_device.h"
#include "mult_planes.h"

namespace gp {

constexpr int MULT_RIF = 4;        // neighbour rows per lane in flight (fresh.hip's; one mult_add4 per batch)
static_assert(MULT_RIF == 4, "a gather batch is one mult_add4");
constexpr int MULT_SLOTS = 256;    // copies of the device histogram (spread the atomics)
constexpr int SOLE_BIN_ROWS = GP_SOLE_BINS, SOLE_BIN_COLS = GP_SOLE_COLS;
static_assert(MULT_BINS == GP_MULT_BINS, "the C-ABI's bin count is the counter's");

struct MultArgs {
  const int64_t* __restrict__ row_ptr;   // the in-CSR
  const int32_t* __restrict__ col;
  const u64* __restrict__ own_rows;      // new_r: [n][W], valid where own_guard != 0
  const uint32_t* __restrict__ own_guard;
  const u64* __restrict__ nb_rows;       // frontier_r: [n][W], valid where nb_guard != 0
  const uint32_t* __restrict__ nb_guard;
  const HubItem* __restrict__ items;
  const int32_t* __restrict__ hubs;          // [n_hubs] hub vertex
  const int32_t* __restrict__ hub_item_ptr;  // [n_hubs + 1]
  u64* __restrict__ hist;                // [MULT_SLOTS][MULT_BINS]
  uint32_t* __restrict__ sole_recv;      // [n]
  u64* __restrict__ sole_sent;           // [n]
  u64* __restrict__ scratch;             // [n_items][MULT_WORDS][W] the items' counters
  u64* __restrict__ hub_sole;            // [n_hubs][W] the hubs' merged sole masks
  int64_t n, n_items, n_hubs;
  int64_t hub_thr;
};

// a lane's counters: one per word of its row piece (W == 1: y stays zero)
struct MultLane {
  MultCounter x, y;
};

// arcs [b, e) of one receiver whose row pieces the lanes hold in `own`.
// SOLE = false: every live in-neighbour's piece & own is one add to the lane's
// counter.  SOLE = true: own is the receiver's sole mask, and each arc's
// popc(row & own) goes to the sender's total
template <int W, bool SOLE>
__device__ __forceinline__ void mult_arcs(const MultArgs& a, int32_t* idx, u64x2 own, int64_t b, int64_t e, int lane,
                                          int g, int lw, MultLane& c) {
  constexpr int RPI = Geo<W>::RPI, LPR = Geo<W>::LPR;
  const bool mine = (own.x | own.y) != 0ull;
  for (int64_t j0 = b; j0 < e; j0 += 64) {
    const int n = (int)std::min<int64_t>(64, e - j0);
    int32_t u = -1;
    if (lane < n) {
      u = a.col[j0 + lane];
      if (a.nb_guard[u] == 0u) u = -1;   // its row is stale
    }
    const u64 m = __ballot(u >= 0);
    if (m == 0ull) continue;
    if (u >= 0) idx[lane_rank(m)] = u;
    wave_sync_lds();
    const int cnt = __popcll(m);
    for (int k0 = 0; k0 < cnt; k0 += MULT_RIF * RPI) {
      u64x2 r[MULT_RIF];
#pragma unroll
      for (int q = 0; q < MULT_RIF; ++q) {
        const int k = k0 + g + q * RPI;
        r[q] = u64x2{0, 0};
        if (k < cnt && mine) r[q] = load_piece<W>(a.nb_rows, idx[k], lw);
      }
      if constexpr (SOLE) {
#pragma unroll
        for (int q = 0; q < MULT_RIF; ++q) {
          const int k = k0 + g + q * RPI;
          const uint32_t cq = (uint32_t)(__popcll(own.x & r[q].x) + __popcll(own.y & r[q].y));
          const uint32_t arc = group_sum<LPR>(cq);   // <= 4096
          if (lw == 0 && arc) atomicAdd(&a.sole_sent[idx[k]], (u64)arc);   // (arc != 0: k < cnt)
        }
      } else {   // the batch's four pieces in one carry-save add (a piece not loaded is zero)
        mult_add4(c.x, own.x & r[0].x, own.x & r[1].x, own.x & r[2].x, own.x & r[3].x);
        if constexpr (W >= 2) mult_add4(c.y, own.y & r[0].y, own.y & r[1].y, own.y & r[2].y, own.y & r[3].y);
      }
    }
    wave_sync_lds();
  }
}

__device__ __forceinline__ void mult_shfl_merge(MultCounter& c, int s) {
  MultCounter o;
#pragma unroll
  for (int b = 0; b < MULT_PLANES; ++b) o.p[b] = (uint64_t)__shfl_xor((u64)c.p[b], s);
  o.sat = (uint64_t)__shfl_xor((u64)c.sat, s);
  mult_merge(c, o);
}

// add up the row slots' counters: afterwards every lane holds the row's
// counter for its lw column (reduce_slots with the bit-sliced add for OR)
template <int W>
__device__ __forceinline__ void mult_reduce_slots(MultLane& c) {
  constexpr int LPR = Geo<W>::LPR;
#pragma unroll
  for (int s = LPR; s < 64; s <<= 1) {
    mult_shfl_merge(c.x, s);
    if constexpr (W >= 2) mult_shfl_merge(c.y, s);
  }
}

// the finished counter of one receiver, which every row slot holds: the lanes
// of slot 0 add the "equals c" popcounts of their first word to their bins
// h[c - 1], the lanes of slot 1 those of their second word (W >= 2 has at least
// two slots: half the instructions of one slot taking both); returns the sole
// mask (every lane)
template <int W>
__device__ __forceinline__ u64x2 mult_tally(const MultLane& c, int g, uint32_t (*h)[64], int lane) {
  static_assert(W == 1 || Geo<W>::RPI >= 2, "slot 1 takes the second word");
  if (g < (W >= 2 ? 2 : 1)) {
    MultCounter t = c.x;
    if (W >= 2 && g == 1) t = c.y;
#pragma unroll
    for (int k = 1; k < MULT_SAT; ++k) h[k - 1][lane] += (uint32_t)__popcll((u64)mult_eq(t, k));
    h[MULT_SAT - 1][lane] += (uint32_t)__popcll((u64)mult_saturated(t));
  }
  u64x2 sole;
  sole.x = (u64)mult_eq(c.x, 1);
  sole.y = W >= 2 ? (u64)mult_eq(c.y, 1) : 0ull;
  return sole;
}

__device__ __forceinline__ uint32_t mult_sole_count(u64x2 sole, int g) {
  return wave_sum_u32(g == 0 ? (uint32_t)(__popcll(sole.x) + __popcll(sole.y)) : 0u);
}

// a wave-uniform 64-bit value, into scalar registers
__device__ __forceinline__ int64_t uniform64(int64_t x) {
  const uint32_t lo = (uint32_t)uniform((int)(uint32_t)x), hi = (uint32_t)uniform((int)(uint32_t)((u64)x >> 32));
  return (int64_t)(((u64)hi << 32) | lo);
}

// the wave's bins, once: lane c - 1 adds bin c to this block's copy of the histogram
__device__ __forceinline__ void mult_flush_hist(const MultArgs& a, const uint32_t (*h)[64], int lane) {
  u64* slot = a.hist + (size_t)(blockIdx.x % MULT_SLOTS) * MULT_BINS;
#pragma unroll
  for (int k = 0; k < MULT_SAT; ++k) {
    const uint32_t t = wave_sum_u32(h[k][lane]);
    if (lane == k && t) atomicAdd(&slot[k + 1], (u64)t);
  }
}

template <int W>
__global__ __launch_bounds__(64) void k_mult(MultArgs a) {
  static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W: a power of two up to 64");
  constexpr int LPR = Geo<W>::LPR;
  __shared__ int32_t idx[64];
  const int lane = threadIdx.x;
  const int g = lane / LPR, lw = lane % LPR;
  // per-lane state that is touched once per receiver lives in LDS, not in
  // registers: the in-list bounds and the sole count of the wave's vertices
  // (read back wave-uniform), and the 16 bins (a lane reads and writes its own
  // column only: no barrier).  W = 64: 73 VGPRs and 6 waves per SIMD against 102
  // and 4 with all of it in registers, a quarter of the pass (profiles/r17_mult_cost.txt)
  __shared__ int64_t rp[2][64];
  __shared__ uint32_t tot[64];
  __shared__ uint32_t h[MULT_SAT][64];
  const int64_t v0 = (int64_t)blockIdx.x * 64;
  const int64_t v = v0 + lane;
  const uint32_t gd = v < a.n ? a.own_guard[v] : 0u;
  u64 gm = __ballot(gd != 0u);   // live receivers of the chunk (bits past n are 0)
  if (gm == 0ull) return;
  rp[0][lane] = gd ? a.row_ptr[v] : 0;
  rp[1][lane] = gd ? a.row_ptr[v + 1] : 0;
  tot[lane] = 0u;   // receiver v0 + k's sole receipts of the round
#pragma unroll
  for (int k = 0; k < MULT_SAT; ++k) h[k][lane] = 0u;
  wave_sync_lds();
  while (gm) {
    const int k = __ffsll((long long)gm) - 1;
    gm &= gm - 1;
    const int64_t bk = uniform64(rp[0][k]), ek = uniform64(rp[1][k]);
    if (ek == bk || ek - bk > a.hub_thr) continue;   // (a hub: the hub kernels walk its items)
    const u64x2 own = load_piece<W>(a.own_rows, v0 + k, lw);
    MultLane c{mult_zero(), mult_zero()};
    mult_arcs<W, false>(a, idx, own, bk, ek, lane, g, lw, c);
    mult_reduce_slots<W>(c);
    const u64x2 sole = mult_tally<W>(c, g, h, lane);
    const uint32_t ns = mult_sole_count(sole, g);
    if (ns == 0u) continue;
    if (lane == 0) tot[k] = ns;
    mult_arcs<W, true>(a, idx, sole, bk, ek, lane, g, lw, c);
  }
  wave_sync_lds();
  if (tot[lane]) a.sole_recv[v0 + lane] += tot[lane];   // this wave alone writes its non-hub receivers (nonzero: v < n)
  mult_flush_hist(a, h, lane);
}

// one item of a hub: its arcs' counter, row slots merged, to scratch
template <int W>
__global__ __launch_bounds__(64) void k_mult_hub(MultArgs a) {
  constexpr int LPR = Geo<W>::LPR;
  __shared__ int32_t idx[64];
  const int lane = threadIdx.x;
  const int g = lane / LPR, lw = lane % LPR;
  if ((int64_t)blockIdx.x >= a.n_items) return;
  const HubItem h = a.items[blockIdx.x];
  if (a.own_guard[h.v] == 0u) return;
  const u64x2 own = load_piece<W>(a.own_rows, h.v, lw);
  MultLane c{mult_zero(), mult_zero()};
  mult_arcs<W, false>(a, idx, own, h.beg, h.end, lane, g, lw, c);
  mult_reduce_slots<W>(c);
  if (g == 0) {   // (every item of a live hub stores its whole counter, zero or not)
    const int64_t row = (int64_t)blockIdx.x * MULT_WORDS;
#pragma unroll
    for (int p = 0; p < MULT_PLANES; ++p) store_piece<W>(a.scratch, row + p, lw, u64x2{(u64)c.x.p[p], (u64)c.y.p[p]});
    store_piece<W>(a.scratch, row + MULT_PLANES, lw, u64x2{(u64)c.x.sat, (u64)c.y.sat});
  }
}

// one hub: its items' counters merged, then what k_mult does with a finished counter
template <int W>
__global__ __launch_bounds__(64) void k_mult_hub_final(MultArgs a) {
  constexpr int LPR = Geo<W>::LPR, RPI = Geo<W>::RPI;
  const int lane = threadIdx.x;
  const int g = lane / LPR, lw = lane % LPR;
  if ((int64_t)blockIdx.x >= a.n_hubs) return;
  const int32_t v = a.hubs[blockIdx.x];
  if (a.own_guard[v] == 0u) return;
  const int32_t i0 = a.hub_item_ptr[blockIdx.x], i1 = a.hub_item_ptr[blockIdx.x + 1];
  MultLane c{mult_zero(), mult_zero()};
  for (int32_t i = i0 + g; i < i1; i += RPI) {   // row slot g: items i0 + g, i0 + g + RPI, ...
    const int64_t row = (int64_t)i * MULT_WORDS;
    MultLane o;
#pragma unroll
    for (int p = 0; p < MULT_PLANES; ++p) {
      const u64x2 t = load_piece<W>(a.scratch, row + p, lw);
      o.x.p[p] = t.x;
      o.y.p[p] = t.y;
    }
    const u64x2 t = load_piece<W>(a.scratch, row + MULT_PLANES, lw);
    o.x.sat = t.x;
    o.y.sat = t.y;
    mult_merge(c.x, o.x);
    if constexpr (W >= 2) mult_merge(c.y, o.y);
  }
  mult_reduce_slots<W>(c);
  __shared__ uint32_t h[MULT_SAT][64];   // (a lane reads and writes its own column only: no barrier)
#pragma unroll
  for (int k = 0; k < MULT_SAT; ++k) h[k][lane] = 0u;
  const u64x2 sole = mult_tally<W>(c, g, h, lane);
  const uint32_t ns = mult_sole_count(sole, g);
  if (lane == 0 && ns) a.sole_recv[v] += ns;   // (k_mult skips the hubs: one writer)
  if (g == 0) store_piece<W>(a.hub_sole, blockIdx.x, lw, sole);
  mult_flush_hist(a, h, lane);
}

// one item of a hub with sole bits: its arcs' share of sole_sent
template <int W>
__global__ __launch_bounds__(64) void k_mult_hub_sole(MultArgs a) {
  constexpr int LPR = Geo<W>::LPR;
  __shared__ int32_t idx[64];
  const int lane = threadIdx.x;
  const int g = lane / LPR, lw = lane % LPR;
  if ((int64_t)blockIdx.x >= a.n_items) return;
  const HubItem h = a.items[blockIdx.x];
  if (a.own_guard[h.v] == 0u) return;   // (k_mult_hub_final stored no mask)
  const u64x2 sole = load_piece<W>(a.hub_sole, h.hub, lw);
  if (!__any((sole.x | sole.y) != 0ull)) return;
  MultLane c{mult_zero(), mult_zero()};
  mult_arcs<W, true>(a, idx, sole, h.beg, h.end, lane, g, lw, c);
}

// out[b][0..3]: peers, receipts (seenpop), sole_recv, sole_sent of the vertices
// of [0, count) with delay_bin(in-degree) = b (k_delay_bins' scheme)
__global__ __launch_bounds__(BLOCK) void k_sole_bins(const int64_t* __restrict__ row_ptr,
                                                     const uint32_t* __restrict__ seenpop,
                                                     const uint32_t* __restrict__ sole_recv,
                                                     const u64* __restrict__ sole_sent, int64_t count,
                                                     u64* __restrict__ out) {
  constexpr int CELLS = SOLE_BIN_ROWS * SOLE_BIN_COLS;
  __shared__ u64 tb[CELLS];
  for (int t = threadIdx.x; t < CELLS; t += BLOCK) tb[t] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t chunks = (count + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); c < chunks; c += (int64_t)gridDim.x * WAVES) {
    const int64_t v = c * 64 + lane;
    const bool in = v < count;
    int bin = -1;
    uint32_t sp = 0, sr = 0;
    u64 ss = 0;
    if (in) {
      bin = std::min(delay_bin(row_ptr[v + 1] - row_ptr[v]), SOLE_BIN_ROWS - 1);   // (a degree is < 2^31: the clamp only guards LDS)
      sp = seenpop[v];
      sr = sole_recv[v];
      ss = sole_sent[v];
    }
    u64 todo = __ballot(in);
    while (todo) {   // one pass per bin the wave's vertices fall into
      const int b = __shfl(bin, __ffsll((long long)todo) - 1);
      const bool mine = bin == b;
      const u64 mm = __ballot(mine);
      // u32: 64 vertices x 4096 messages = 2^18 receipts
      const uint32_t rec = wave_sum_u32(mine ? sp : 0u);
      const uint32_t sol = wave_sum_u32(mine ? sr : 0u);
      const u64 snt = wave_sum_u64(mine ? ss : 0ull);
      if (lane == 0) {
        u64* cell = tb + b * SOLE_BIN_COLS;
        atomicAdd(&cell[0], (u64)__popcll(mm));
        if (rec) atomicAdd(&cell[1], (u64)rec);
        if (sol) atomicAdd(&cell[2], (u64)sol);
        if (snt) atomicAdd(&cell[3], snt);
      }
      todo &= ~mm;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < CELLS; t += BLOCK)
    if (tb[t]) atomicAdd(&out[t], tb[t]);
}

static void mult_free(Ctx* c) {
  dfree(&c->d_sole_recv);
  dfree(&c->d_sole_sent);
  dfree(&c->d_mult_hist);
  dfree(&c->d_sole_bins);
  dfree(&c->d_mult_scratch);
  dfree(&c->d_mult_hub_sole);
  c->mult_rows = c->mult_scratch_words = c->mult_hub_words = 0;
  record_off(c->rec[R_MULT]);
}

// gp_reset: gp_track_mult takes effect (u32 + u64 per vertex, the histogram's
// copies, the bins' device result, the hubs' scratch -- or nothing), cleared.
// The scratch follows the hub table and the row width, so another overlay,
// hub_threshold or message table re-sizes it.  The exact frontier rows are
// alloc_state's (setup.hip: frx_rows)
static int mult_reset(Ctx* c) {
  const size_t n = (size_t)c->n, W = (size_t)c->words;
  const size_t sw = (size_t)c->n_hub_items * MULT_WORDS * W, hw = (size_t)c->n_hubs * W;
  if (!c->d_sole_recv || c->mult_rows != n || c->mult_scratch_words != sw || c->mult_hub_words != hw) {
    mult_free(c);
    if (dalloc(&c->d_sole_recv, n) != 0 || dalloc(&c->d_sole_sent, n) != 0 ||
        dalloc(&c->d_mult_hist, (size_t)MULT_SLOTS * MULT_BINS) != 0 ||
        dalloc(&c->d_sole_bins, (size_t)SOLE_BIN_ROWS * SOLE_BIN_COLS) != 0 || dalloc(&c->d_mult_scratch, sw) != 0 ||
        dalloc(&c->d_mult_hub_sole, hw) != 0) {
      mult_free(c);
      return GP_ENOMEM;
    }
    c->mult_rows = n;
    c->mult_scratch_words = sw;
    c->mult_hub_words = hw;
  }
  GP_HIP(hipMemsetAsync(c->d_sole_recv, 0, std::max<size_t>(n, 1) * 4, c->stream));
  GP_HIP(hipMemsetAsync(c->d_sole_sent, 0, std::max<size_t>(n, 1) * 8, c->stream));
  GP_HIP(hipMemsetAsync(c->d_mult_hist, 0, (size_t)MULT_SLOTS * MULT_BINS * 8, c->stream));
  return 0;
}

template <int W>
static void launch_mult_w(Ctx* c, const MultArgs& a) {
  hipStream_t s = c->stream;
  hipLaunchKernelGGL((k_mult<W>), dim3(grid_for(a.n, 64)), dim3(64), 0, s, a);
  if (a.n_items > 0 && a.n_hubs > 0) {
    hipLaunchKernelGGL((k_mult_hub<W>), dim3(grid_for(a.n_items, 1)), dim3(64), 0, s, a);
    hipLaunchKernelGGL((k_mult_hub_final<W>), dim3(grid_for(a.n_hubs, 1)), dim3(64), 0, s, a);
    hipLaunchKernelGGL((k_mult_hub_sole<W>), dim3(grid_for(a.n_items, 1)), dim3(64), 0, s, a);
  }
}

// after E_r: the deliverer counts of round r's first receipts
static int mult_count_round(Ctx* c) {
  if (c->n <= 0) return 0;
  GP_TRY(record_need_rows(c, mult_record, c->n));
  if (c->mult_scratch_words != (size_t)c->n_hub_items * MULT_WORDS * (size_t)c->words ||
      c->mult_hub_words != (size_t)c->n_hubs * (size_t)c->words)
    return set_error(GP_ESTATE, "internal: delivery multiplicity scratch does not match the hub table");
  const int cur = c->cur;
  MultArgs a{};
  a.row_ptr = c->d_row_ptr;
  a.col = c->d_col;
  a.own_rows = c->d_frx[cur ^ 1];
  a.own_guard = c->d_fpop[cur ^ 1];
  a.nb_rows = c->d_frx[cur];
  a.nb_guard = c->d_fpop[cur];
  a.items = c->d_hub_items;
  a.hubs = c->d_hubs;
  a.hub_item_ptr = c->d_hub_item_ptr;
  a.hist = c->d_mult_hist;
  a.sole_recv = c->d_sole_recv;
  a.sole_sent = c->d_sole_sent;
  a.scratch = c->d_mult_scratch;
  a.hub_sole = c->d_mult_hub_sole;
  a.n = c->n;
  a.n_items = c->n_hub_items;
  a.n_hubs = c->n_hubs;
  a.hub_thr = c->cfg.hub_threshold;
  GP_TRY(with_words(c->words, [&](auto w) { launch_mult_w<w()>(c, a); }));
  GP_HIP(hipGetLastError());
  return 0;
}

GP_RECORD_OPS(mult_record) = {R_MULT, "delivery multiplicity", "gp_track_mult", true, 5, nullptr, nullptr, mult_reset,
                               mult_free, mult_count_round, nullptr, nullptr};

int mult_read(Ctx* c, int32_t what, void* host, int64_t bytes) {
  GP_TRY(record_readable(c, mult_record));
  const int64_t want = what == GP_SOLE_SENT ? c->n * 8 : c->n * 4;
  if (bytes != want) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(want));
  if (bytes == 0) return 0;
  return copy_sync(c, host, what == GP_SOLE_SENT ? (const void*)c->d_sole_sent : (const void*)c->d_sole_recv,
                   (size_t)bytes, hipMemcpyDeviceToHost);
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_track_mult(gp_ctx* c, int32_t on) { return record_track(c, mult_record, on); }

int gp_read_mult_hist(gp_ctx* c, uint64_t* hist, int32_t bins) {
  if (!c || !hist) return set_error(GP_EINVAL, "null argument");
  GP_TRY(record_readable(c, mult_record));
  if (bins != MULT_BINS) return set_error(GP_EINVAL, "bins must be " + std::to_string(MULT_BINS));
  GP_HIP(hipSetDevice(c->device));
  std::vector<u64> copies((size_t)MULT_SLOTS * MULT_BINS);
  GP_TRY(copy_sync(c, copies.data(), c->d_mult_hist, copies.size() * 8, hipMemcpyDeviceToHost));
  uint64_t sum[MULT_BINS] = {};
  for (int s = 0; s < MULT_SLOTS; ++s)
    for (int b = 1; b < MULT_BINS; ++b) sum[b] += copies[(size_t)s * MULT_BINS + b];
  // bin 0, the receipts without a deliverer: the injections at up origins the rounds counted
  for (const gp_round_stats& st : c->run_stats) sum[0] += st.injected;
  for (int b = 0; b < MULT_BINS; ++b) hist[b] = sum[b];
  return 0;
}

int gp_read_sole_bins(gp_ctx* c, uint64_t* out, int32_t bins) {
  if (!c || !out) return set_error(GP_EINVAL, "null argument");
  GP_TRY(record_readable(c, mult_record));
  if (bins != SOLE_BIN_ROWS) return set_error(GP_EINVAL, "bins must be " + std::to_string(SOLE_BIN_ROWS));
  GP_HIP(hipSetDevice(c->device));
  constexpr size_t BYTES = (size_t)SOLE_BIN_ROWS * SOLE_BIN_COLS * 8;
  GP_HIP(hipMemsetAsync(c->d_sole_bins, 0, BYTES, c->stream));
  const int64_t count = c->n;
  if (count > 0) {
    const int grid = std::max(1, std::min(grid_for((count + 63) / 64, WAVES), c->cu_count * 4));
    hipLaunchKernelGGL(k_sole_bins, dim3(grid), dim3(BLOCK), 0, c->stream, (const int64_t*)c->d_row_ptr,
                       (const uint32_t*)c->d_seenpop, (const uint32_t*)c->d_sole_recv, (const u64*)c->d_sole_sent, count,
                       c->d_sole_bins);
    GP_HIP(hipGetLastError());
  }
  return copy_sync(c, out, c->d_sole_bins, BYTES, hipMemcpyDeviceToHost);
}

}  // extern "C"
