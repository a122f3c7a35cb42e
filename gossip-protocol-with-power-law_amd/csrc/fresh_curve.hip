// fresh_curve.hip -- fresh-delivery curves: for message
// k and round r, how many of the sends that carried k delivered a first
// receipt.  With frontier_r(u) and new_r(v) as in fresh.hip,
//
//   fresh_curve[r + 1][k] = #{ arcs u -> v, u in In(v) : k in frontier_r(u) & new_r(v) }
//
// rows indexed by receipt round, beside the spread curve's (curve.hip): the
// ratio of the two rows is the deliverers per first receipt.  It is fresh.hip's
// pass with the popcount taken per bit column instead of per arc: the same
// guarded rows at the same point of round_launch (d_frx[cur] behind fpop[cur]
// is frontier_r, d_frx[cur ^ 1] behind fpop[cur ^ 1] is new_r), read the same
// way, receivers as owners over the in-CSR.  Only that side exists: nothing is
// added per sender, so there is no scatter form and no per-arc atomic, and a
// directed overlay takes the path of an undirected one.
//
// k_fresh_curve: persistent waves in 4-wave blocks.  A wave strides over
// 64-owner chunks: one coalesced load of the 64 guard words and a ballot, and
// nothing else when no owner of the chunk is live.  A live owner keeps its row
// in registers, 16 B per lane (Geo<W>), and the wave walks its arc list 64
// arcs at a time: column ids, the neighbours' guard words, the live neighbours
// staged in LDS, their rows gathered 128 / W per wave-instruction, FC_RIF in
// flight; a lane whose owner piece is zero loads nothing.  Where k_fresh
// popcounts own & r[q], each lane adds the two words of own & r[q] into one
// CurvePlanes per word (curve_planes.h): eight rows through curve_add8, a tail
// of one or two through curve_add_row.  A lane holds the same word positions
// for every owner and every arc, so its planes persist across arcs, owners and
// chunks; they are expanded only when booking the next batch would pass
// CURVE_PLANE_ROWS (`held`, wave-uniform, as k_curve's) or the wave's range
// ends -- into the block's LDS counts, and from there each nonzero column goes
// to the u64 row with one atomic.  Integer adds commute: the row is
// deterministic.  Owners above hub_threshold are left to k_fresh_curve_hub,
// one wave per HubItem of the existing table with the same planes, flushed at
// the item's end.
//
// Widths.  A plane set holds CURVE_PLANE_ROWS = 2,047 rows per bit column; the
// booking counts the rows a lane may add (an upper bound), so one receiver
// with more simultaneous deliverers than that flushes mid-list.  A block's LDS
// count is u32: it is bounded by the arcs the block walks, at most the
// context's (a 2^24-arc row left whole by hub_threshold adds at most 2^24 to a
// column), and fresh_curve_reset refuses a context of 2^32 arcs or more.  The
// output is u64: a column of one row is bounded by the arcs, a column sum by
// the arcs too (a receiver takes a message once).
//
// Registers and shape (gfx950): no scratch at any width; W = 64 takes 124
// VGPRs, 4 waves per SIMD, and 17.4 KB of LDS per block.  Both choices below
// were measured (profiles/r14_fresh_curve_cost.txt: the passes of a C4 run
// summed, library variants alternating on one box): 4-wave blocks sharing one
// count array with full planes 81.9-82.5 ms; one-wave blocks with 16 KiB of
// counts each 128.5-129.6 ms (LDS leaves 3 waves per SIMD); shallower planes,
// which buy registers with more flushes, 88.0-88.4 ms with 4 planes of eights
// (127 rows, 100 VGPRs) and 124.6-125.1 ms with 2 (31 rows, 90 VGPRs, 5 waves
// per SIMD).  k_fresh's scatter pass over the same row pairs: 88.4 ms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "curve_planes.h"
#include "gp_device.h"

namespace gp {

constexpr int FRESH_CURVE_ROWS = 255;   // receipt rounds 0 .. 254, the spread curve's cap (curve.hip)
constexpr int FC_RIF = 4;               // neighbour rows per lane in flight (k_fresh's, profiles/r13_fresh_cost.txt)
constexpr int FC_WAVES = 4;             // waves of a block: they share the LDS counts (1: 129 ms against 82, header)
constexpr int FC_BLOCK = FC_WAVES * 64;
constexpr int FC_BLOCKS_PER_CU = 4;     // the persistent grid: 16 waves per CU (2: 124 ms; 8 and 16: 82, as 4)

struct FreshCurveArgs {
  const int64_t* __restrict__ row_ptr;   // the in-CSR: owners are receivers
  const int32_t* __restrict__ col;
  const u64* __restrict__ own_rows;      // [n][W] new_r, valid where own_guard != 0
  const uint32_t* __restrict__ own_guard;
  const u64* __restrict__ nb_rows;       // [n][W] frontier_r, valid where nb_guard != 0
  const uint32_t* __restrict__ nb_guard;
  const HubItem* __restrict__ items;
  u64* __restrict__ out;                 // [W * 64] row r + 1 of the record
  int64_t n, n_items;
  int64_t hub_thr;
};

// expand the lane's planes into the block's counts ([bit][word], as k_curve's)
template <int W>
__device__ __forceinline__ void fc_flush(CurvePlanes (&p)[Geo<W>::WPL], int& held, uint32_t* lc, int lw) {
  constexpr int WPL = Geo<W>::WPL;
#pragma unroll
  for (int j = 0; j < WPL; ++j) {
    const int w = lw * WPL + j;
#pragma unroll 4
    for (int b = 0; b < 64; ++b) {
      const uint32_t cnt = curve_count(p[j], b);
      if (cnt) atomicAdd(&lc[b * W + w], cnt);
    }
    curve_clear(p[j]);
  }
  held = 0;
}

// arcs [b, e) of one owner whose row pieces the lanes hold in `own`: every
// live neighbour's own & row goes into the lane's planes
template <int W>
__device__ __forceinline__ void fc_arcs(const FreshCurveArgs& a, int32_t* idx, uint32_t* lc, u64x2 own, int64_t b,
                                        int64_t e, int lane, int g, int lw, CurvePlanes (&p)[Geo<W>::WPL], int& held,
                                        bool& flushed) {
  constexpr int RPI = Geo<W>::RPI, WPL = Geo<W>::WPL;
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
    for (int k0 = 0; k0 < cnt; k0 += CURVE_GROUP * RPI) {
      // rows a lane adds in this step, at most (wave-uniform: the booking)
      const int adding = std::min(CURVE_GROUP, (cnt - k0 + RPI - 1) / RPI);
      if (!curve_fits(held, adding)) {
        fc_flush<W>(p, held, lc, lw);
        flushed = true;
      }
      held += adding;
      if (adding <= 2) {   // a tail (every step of the narrow widths: 64 arcs are one or two rows per lane)
        u64x2 r[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int k = k0 + g + q * RPI;
          r[q] = u64x2{0, 0};
          if (k < cnt && mine) r[q] = load_piece<W>(a.nb_rows, idx[k], lw);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          curve_add_row(p[0], own.x & r[q].x);
          if constexpr (WPL == 2) curve_add_row(p[1], own.y & r[q].y);
        }
        continue;
      }
      uint64_t x[CURVE_GROUP], y[CURVE_GROUP];
#pragma unroll
      for (int h = 0; h < CURVE_GROUP; h += FC_RIF) {
        u64x2 r[FC_RIF];
#pragma unroll
        for (int q = 0; q < FC_RIF; ++q) {
          const int k = k0 + g + (h + q) * RPI;
          r[q] = u64x2{0, 0};
          if (k < cnt && mine) r[q] = load_piece<W>(a.nb_rows, idx[k], lw);
        }
#pragma unroll
        for (int q = 0; q < FC_RIF; ++q) {
          x[h + q] = own.x & r[q].x;
          y[h + q] = own.y & r[q].y;
        }
      }
      curve_add8(p[0], x);
      if constexpr (WPL == 2) curve_add8(p[1], y);
    }
    wave_sync_lds();
  }
}

// the block's counts to the output row, one atomic per nonzero column
template <int W>
__device__ __forceinline__ void fc_drain(const uint32_t* lc, u64* __restrict__ out) {
  for (int t = threadIdx.x; t < W * 64; t += FC_BLOCK) {
    const uint32_t cnt = lc[t];
    if (cnt) atomicAdd(&out[(t % W) * 64 + t / W], (u64)cnt);
  }
}

template <int W>
__global__ __launch_bounds__(FC_BLOCK) void k_fresh_curve(FreshCurveArgs a) {
  static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W: a power of two up to 64");
  static_assert(FC_RIF * 2 == CURVE_GROUP, "a curve_add8 batch is two half-batches of loads");
  constexpr int LPR = Geo<W>::LPR, WPL = Geo<W>::WPL, M = W * 64;
  __shared__ uint32_t lc[M];
  __shared__ int32_t idx[FC_WAVES][64];
  __shared__ int any;
  for (int t = threadIdx.x; t < M; t += FC_BLOCK) lc[t] = 0u;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int g = lane / LPR, lw = lane % LPR;
  const int64_t chunks = (a.n + 63) >> 6;
  const int64_t nw = (int64_t)gridDim.x * FC_WAVES;

  CurvePlanes p[WPL];
  int held = 0;           // rows booked into the planes (wave-uniform)
  bool flushed = false;   // the wave added to the block's counts (wave-uniform)
  for (int64_t c = (int64_t)blockIdx.x * FC_WAVES + wib; c < chunks; c += nw) {
    const int64_t v0 = c * 64, v = v0 + lane;
    const uint32_t gd = v < a.n ? a.own_guard[v] : 0u;
    u64 gm = __ballot(gd != 0u);   // live owners of the chunk (bits past n are 0)
    if (gm == 0ull) continue;
    int64_t b = 0, e = 0;
    if (gd) {
      b = a.row_ptr[v];
      e = a.row_ptr[v + 1];
    }
    while (gm) {
      const int k = __ffsll((long long)gm) - 1;
      gm &= gm - 1;
      const int64_t bk = __shfl((long long)b, k), ek = __shfl((long long)e, k);
      if (ek == bk || ek - bk > a.hub_thr) continue;   // (a hub: k_fresh_curve_hub walks its items)
      const u64x2 own = load_piece<W>(a.own_rows, v0 + k, lw);
      fc_arcs<W>(a, idx[wib], lc, own, bk, ek, lane, g, lw, p, held, flushed);
    }
  }
  if (held > 0) {
    fc_flush<W>(p, held, lc, lw);
    flushed = true;
  }
  if (flushed && lane == 0) any = 1;
  __syncthreads();
  if (any) fc_drain<W>(lc, a.out);
}

template <int W>
__global__ __launch_bounds__(FC_BLOCK) void k_fresh_curve_hub(FreshCurveArgs a) {
  constexpr int LPR = Geo<W>::LPR, WPL = Geo<W>::WPL, M = W * 64;
  __shared__ uint32_t lc[M];
  __shared__ int32_t idx[FC_WAVES][64];
  __shared__ int any;
  for (int t = threadIdx.x; t < M; t += FC_BLOCK) lc[t] = 0u;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int g = lane / LPR, lw = lane % LPR;
  const int64_t item = (int64_t)blockIdx.x * FC_WAVES + wib;
  if (item < a.n_items) {   // (wave-uniform)
    const HubItem h = a.items[item];
    if (a.own_guard[h.v] != 0u) {
      CurvePlanes p[WPL];
      int held = 0;
      bool flushed = false;
      const u64x2 own = load_piece<W>(a.own_rows, h.v, lw);
      fc_arcs<W>(a, idx[wib], lc, own, h.beg, h.end, lane, g, lw, p, held, flushed);
      if (held > 0) fc_flush<W>(p, held, lc, lw);   // the item's planes end here
      if (lane == 0) any = 1;
    }
  }
  __syncthreads();
  if (any) fc_drain<W>(lc, a.out);
}

int fresh_curve_env_grid() {
  const char* e = getenv("GP_FRESH_CURVE_GRID");
  if (!e) return 0;
  const long k = strtol(e, nullptr, 10);
  return k >= 1 && k <= (1 << 20) ? (int)k : 0;
}

static void fresh_curve_free(Ctx* c) {
  dfree(&c->d_fresh_curve);
  c->fresh_curve_words = 0;
  record_off(c->rec[R_FRESH_CURVE]);
}

// gp_reset: gp_track_fresh_curve takes effect ([255][W * 64] u64, or nothing),
// cleared.  The exact frontier rows are alloc_state's (setup.hip: frx_rows)
static int fresh_curve_reset(Ctx* c) {
  if (c->nnz >= (int64_t)1 << 32) {   // (the u32 LDS counts of a block: header)
    fresh_curve_free(c);
    return set_error(GP_EINVAL, "gp_track_fresh_curve: an overlay of 2^32 arcs or more is not counted");
  }
  const size_t words = (size_t)FRESH_CURVE_ROWS * (size_t)c->words * 64;
  if (!c->d_fresh_curve || c->fresh_curve_words != words) {
    fresh_curve_free(c);
    if (dalloc(&c->d_fresh_curve, words) != 0) return GP_ENOMEM;
    c->fresh_curve_words = words;
  }
  GP_HIP(hipMemsetAsync(c->d_fresh_curve, 0, words * 8, c->stream));
  return 0;
}

template <int W>
static void launch_fresh_curve_w(Ctx* c, const FreshCurveArgs& a) {
  hipStream_t s = c->stream;
  const int64_t chunks = (a.n + 63) / 64;
  int64_t grid = std::min<int64_t>((chunks + FC_WAVES - 1) / FC_WAVES, (int64_t)std::max(c->cu_count, 1) * FC_BLOCKS_PER_CU);
  if (c->fresh_curve_grid > 0) grid = std::min<int64_t>(grid, c->fresh_curve_grid);
  hipLaunchKernelGGL((k_fresh_curve<W>), dim3((unsigned)std::max<int64_t>(grid, 1)), dim3(FC_BLOCK), 0, s, a);
  if (a.n_items > 0)
    hipLaunchKernelGGL((k_fresh_curve_hub<W>), dim3(grid_for(a.n_items, FC_WAVES)), dim3(FC_BLOCK), 0, s, a);
}

// after E_r: row r + 1, the deliverers of round r's first receipts per message
static int fresh_curve_count_round(Ctx* c) {
  if (c->n <= 0) return 0;
  const int r = c->round;
  if (r + 1 >= FRESH_CURVE_ROWS) return set_error(GP_ESTATE, "internal: fresh-delivery curve past its last row");
  GP_TRY(record_need_rows(c, fresh_curve_record, c->n));
  const int cur = c->cur;
  FreshCurveArgs a{};
  a.row_ptr = c->d_row_ptr;
  a.col = c->d_col;
  a.own_rows = c->d_frx[cur ^ 1];
  a.own_guard = c->d_fpop[cur ^ 1];
  a.nb_rows = c->d_frx[cur];
  a.nb_guard = c->d_fpop[cur];
  a.items = c->d_hub_items;
  a.out = c->d_fresh_curve + (size_t)(r + 1) * (size_t)c->words * 64;
  a.n = c->n;
  a.n_items = c->n_hub_items;
  a.hub_thr = c->cfg.hub_threshold;
  GP_TRY(with_words(c->words, [&](auto w) { launch_fresh_curve_w<w()>(c, a); }));
  GP_HIP(hipGetLastError());
  return 0;
}

GP_RECORD_OPS(fresh_curve_record) = {R_FRESH_CURVE, "fresh-delivery curves", "gp_track_fresh_curve", true, 3, nullptr,
                                      nullptr, fresh_curve_reset, fresh_curve_free, fresh_curve_count_round, nullptr,
                                      nullptr};

}  // namespace gp

using namespace gp;

extern "C" {

int gp_track_fresh_curve(gp_ctx* c, int32_t on) { return record_track(c, fresh_curve_record, on); }

int gp_read_fresh_curve(gp_ctx* c, uint64_t* host, int32_t cap_rows, int32_t* rows_out) {
  if (!c || !host || !rows_out) return set_error(GP_EINVAL, "null argument");
  GP_TRY(record_readable(c, fresh_curve_record));
  const int32_t rows = c->round + 1;
  if (cap_rows < rows) return set_error(GP_EINVAL, "cap_rows < " + std::to_string(rows) + " rows");
  GP_HIP(hipSetDevice(c->device));
  GP_HIP(hipStreamSynchronize(c->stream));
  GP_HIP(hipMemcpy2D(host, (size_t)c->m * 8, c->d_fresh_curve, (size_t)c->words * 64 * 8, (size_t)c->m * 8,
                     (size_t)rows, hipMemcpyDeviceToHost));
  *rows_out = rows;
  return 0;
}

}  // extern "C"
