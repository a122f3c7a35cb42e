// fresh.hip -- per-peer fresh deliveries: of the lines
// the traffic record counts (load.hip), the ones that told the receiver
// something it did not hold.  With frontier_r(u) u's frontier after L_r and I_r
// and new_r(v) the bits v first receives in E_r,
//
//   fresh_sent[u] += sum_{v in Out(u)} |frontier_r(u) & new_r(v)|
//   fresh_recv[v] += sum_{u in In(v)}  |frontier_r(u) & new_r(v)|
//
// every round, at the end of round_launch (driver.hip), after the event that
// ends expand_ms.  There d_frx[cur] behind fpop[cur] != 0 is frontier_r
// (k_churn zeroed a crashing sender's count, k_inject added round r's
// injections) and d_frx[cur ^ 1] behind fpop_next != 0 is new_r (every commit
// path stores it; round r + 1's injections are not in it yet) -- the argument
// of curve.hip.  A row behind a zero guard is stale and is never loaded.
//
// The pass is an integer SpMV whose multiply is popc(owner row & neighbour row)
// over W words.  k_fresh: one-wave blocks, 64 owners each: one coalesced load
// of the 64 guard words and a ballot, and nothing else when no owner of the
// chunk is live (an early or late round costs the guard sweep).  A live owner
// keeps its row in registers, 16 B per lane (Geo<W>: W / 2 lanes per row, every
// row slot the same pieces), and the wave walks its arc list 64 arcs at a time:
// column ids, the neighbours' guard words (4 B each), the live neighbours
// staged in LDS, then their rows gathered 128 / W per wave-instruction,
// FRESH_RIF instructions in flight; a lane whose owner piece is zero loads
// nothing.  Owners above hub_threshold are left to k_fresh_hub, one wave per
// HubItem of the existing hub table and one 64-bit atomicAdd per item.
//
// Both totals are this gather with the roles swapped: owner = receiver over
// the in-CSR gives fresh_recv, owner = sender over the out-CSR gives
// fresh_sent.  Two forms follow.  SCATTER: the receiver pass alone, each arc's
// count also going to the sender's total with one 64-bit atomicAdd (integer
// adds commute: the totals are deterministic) -- every overlay's form, and
// the only one a directed overlay has (the hub table is the in-CSR's).
// Gather twice: an undirected overlay's out-CSR is its in-CSR, hub table
// included, so the kernel can run once per role and no atomic touches a
// non-hub entry; it reads every row pair twice and measured 134 ms against 89
// per C4 run (profiles/r13_fresh_cost.txt), so it is kept behind
// GP_FRESH_GATHER=1 at gp_create as the A/B lever and a second
// implementation the tests hold the first to.
//
// Widths.  One arc adds at most 4096 (messages per context).  The sum of one
// 64-arc chunk is at most 2^18 over the whole wave, so a lane keeps it in a
// u32; the sum over an owner's chunks is u64 from the lane on: hub_threshold
// may leave a 2^24-arc in-list whole, and 2^24 arcs x 4096 = 2^36.  The arrays
// are u64: a peer's total over a run is bounded by its degree x 4096.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "gp_device.h"

namespace gp {

constexpr int FRESH_RIF = 4;   // neighbour rows per lane in flight (profiles/r13_fresh_cost.txt)

struct FreshArgs {
  const int64_t* __restrict__ row_ptr;   // the CSR of the owners' neighbour lists
  const int32_t* __restrict__ col;
  const u64* __restrict__ own_rows;      // [n][W], valid where own_guard != 0
  const uint32_t* __restrict__ own_guard;
  const u64* __restrict__ nb_rows;       // [n][W], valid where nb_guard != 0
  const uint32_t* __restrict__ nb_guard;
  const HubItem* __restrict__ items;
  u64* __restrict__ out;                 // [n] the owners' totals
  u64* __restrict__ other;               // SCATTER: [n] the neighbours' totals
  int64_t n, n_items;
  int64_t hub_thr;
};

// arcs [b, e) of one owner whose row pieces the lanes hold in `own`; returns
// this lane's share of sum_arcs popc(own row & neighbour row)
template <int W, bool SCATTER>
__device__ __forceinline__ u64 fresh_arcs(const FreshArgs& a, int32_t* idx, u64x2 own, int64_t b, int64_t e, int lane,
                                          int g, int lw) {
  constexpr int RPI = Geo<W>::RPI, LPR = Geo<W>::LPR;
  const bool mine = (own.x | own.y) != 0ull;
  u64 sum = 0;   // over the owner's chunks: u64 (header)
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
    uint32_t part = 0;   // one chunk: at most 64 rows x 128 bits per lane
    for (int k0 = 0; k0 < cnt; k0 += FRESH_RIF * RPI) {
      u64x2 r[FRESH_RIF];
#pragma unroll
      for (int q = 0; q < FRESH_RIF; ++q) {
        const int k = k0 + g + q * RPI;
        r[q] = u64x2{0, 0};
        if (k < cnt && mine) r[q] = load_piece<W>(a.nb_rows, idx[k], lw);
      }
#pragma unroll
      for (int q = 0; q < FRESH_RIF; ++q) {
        const uint32_t cq = (uint32_t)(__popcll(own.x & r[q].x) + __popcll(own.y & r[q].y));
        part += cq;
        if constexpr (SCATTER) {
          const int k = k0 + g + q * RPI;
          const uint32_t arc = group_sum<LPR>(cq);   // <= 4096
          if (lw == 0 && arc) atomicAdd(&a.other[idx[k]], (u64)arc);   // (arc != 0: k < cnt)
        }
      }
    }
    sum += part;
    wave_sync_lds();
  }
  return sum;
}

template <int W, bool SCATTER>
__global__ __launch_bounds__(64) void k_fresh(FreshArgs a) {
  static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W: a power of two up to 64");
  constexpr int LPR = Geo<W>::LPR;
  __shared__ int32_t idx[64];
  const int lane = threadIdx.x;
  const int g = lane / LPR, lw = lane % LPR;
  const int64_t v0 = (int64_t)blockIdx.x * 64, v = v0 + lane;
  const uint32_t gd = v < a.n ? a.own_guard[v] : 0u;
  u64 gm = __ballot(gd != 0u);   // live owners of the chunk (bits past n are 0)
  if (gm == 0ull) return;
  int64_t b = 0, e = 0;
  if (gd) {
    b = a.row_ptr[v];
    e = a.row_ptr[v + 1];
  }
  u64 total = 0;   // owner v's sum, in its lane
  while (gm) {
    const int k = __ffsll((long long)gm) - 1;
    gm &= gm - 1;
    const int64_t bk = __shfl((long long)b, k), ek = __shfl((long long)e, k);
    if (ek == bk || ek - bk > a.hub_thr) continue;   // (a hub: k_fresh_hub walks its items)
    const u64x2 own = load_piece<W>(a.own_rows, v0 + k, lw);
    const u64 s = wave_sum_u64(fresh_arcs<W, SCATTER>(a, idx, own, bk, ek, lane, g, lw));
    if (lane == k) total = s;
  }
  if (total) a.out[v] += total;   // this wave alone writes its non-hub owners
}

template <int W, bool SCATTER>
__global__ __launch_bounds__(64) void k_fresh_hub(FreshArgs a) {
  constexpr int LPR = Geo<W>::LPR;
  __shared__ int32_t idx[64];
  const int lane = threadIdx.x;
  const int g = lane / LPR, lw = lane % LPR;
  if ((int64_t)blockIdx.x >= a.n_items) return;
  const HubItem h = a.items[blockIdx.x];
  if (a.own_guard[h.v] == 0u) return;
  const u64x2 own = load_piece<W>(a.own_rows, h.v, lw);
  const u64 s = wave_sum_u64(fresh_arcs<W, SCATTER>(a, idx, own, h.beg, h.end, lane, g, lw));
  if (lane == 0 && s) atomicAdd(&a.out[h.v], s);
}

bool fresh_env_gather() {
  const char* e = getenv("GP_FRESH_GATHER");
  return e && e[0] == '1';
}

static void fresh_free(Ctx* c) {
  dfree(&c->d_fresh_sent);
  dfree(&c->d_fresh_recv);
  record_off(c->rec[R_FRESH]);
}

// gp_reset: gp_track_fresh takes effect (two u64[n], or none), cleared.  The
// exact frontier rows are alloc_state's (setup.hip: frx_rows)
static int fresh_reset(Ctx* c) {
  if (!c->d_fresh_sent) {
    const size_t n = (size_t)c->n;
    if (dalloc(&c->d_fresh_sent, n) != 0 || dalloc(&c->d_fresh_recv, n) != 0) {
      fresh_free(c);
      return GP_ENOMEM;
    }
  }
  GP_HIP(hipMemsetAsync(c->d_fresh_sent, 0, (size_t)c->n * 8, c->stream));
  GP_HIP(hipMemsetAsync(c->d_fresh_recv, 0, (size_t)c->n * 8, c->stream));
  return 0;
}

template <int W, bool SCATTER>
static void launch_fresh_w(Ctx* c, const FreshArgs& a) {
  hipStream_t s = c->stream;
  hipLaunchKernelGGL((k_fresh<W, SCATTER>), dim3(grid_for(a.n, 64)), dim3(64), 0, s, a);
  if (a.n_items > 0)
    hipLaunchKernelGGL((k_fresh_hub<W, SCATTER>), dim3(grid_for(a.n_items, 1)), dim3(64), 0, s, a);
}

template <bool SCATTER>
static int launch_fresh(Ctx* c, const FreshArgs& a) {
  GP_TRY(with_words(c->words, [&](auto w) { launch_fresh_w<w(), SCATTER>(c, a); }));
  GP_HIP(hipGetLastError());
  return 0;
}

// after E_r: round r's deliveries that were first receipts, per receiver and per sender
static int fresh_count_round(Ctx* c) {
  if (c->n <= 0) return 0;
  GP_TRY(record_need_rows(c, fresh_record, c->n));
  const int cur = c->cur;
  FreshArgs a{};
  a.items = c->d_hub_items;
  a.n = c->n;
  a.n_items = c->n_hub_items;
  a.hub_thr = c->cfg.hub_threshold;
  // owner = receiver: its new_r row against its in-neighbours' frontier rows
  a.row_ptr = c->d_row_ptr;
  a.col = c->d_col;
  a.own_rows = c->d_frx[cur ^ 1];
  a.own_guard = c->d_fpop[cur ^ 1];
  a.nb_rows = c->d_frx[cur];
  a.nb_guard = c->d_fpop[cur];
  a.out = c->d_fresh_recv;
  a.other = c->d_fresh_sent;
  if (c->directed || !c->fresh_gather) return launch_fresh<true>(c, a);
  GP_TRY(launch_fresh<false>(c, a));
  // owner = sender: its frontier row against its out-neighbours' new rows (the
  // out-CSR of an undirected overlay is its in-CSR, hub table included)
  std::swap(a.own_rows, a.nb_rows);
  std::swap(a.own_guard, a.nb_guard);
  a.out = c->d_fresh_sent;
  a.other = nullptr;
  return launch_fresh<false>(c, a);
}

GP_RECORD_OPS(fresh_record) = {R_FRESH, "fresh deliveries", "gp_track_fresh", true, 2, nullptr, nullptr, fresh_reset,
                                fresh_free, fresh_count_round, nullptr, nullptr};

int fresh_read(Ctx* c, int32_t what, void* host, int64_t bytes) {
  GP_TRY(record_readable(c, fresh_record));
  if (bytes != c->n * 8) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(c->n * 8));
  return copy_sync(c, host, what == GP_FRESH_SENT ? c->d_fresh_sent : c->d_fresh_recv, (size_t)bytes,
                   hipMemcpyDeviceToHost);
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_track_fresh(gp_ctx* c, int32_t on) { return record_track(c, fresh_record, on); }

}  // extern "C"
