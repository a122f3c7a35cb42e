// link.hip -- per-link fresh deliveries: the news every
// arc of the overlay carried.  With frontier_r(u) and new_r(v) as in fresh.hip,
// for arc j of the in-CSR (row_ptr[v] <= j < row_ptr[v + 1], u = col[j]: sender
// u, receiver v)
//
//   link_fresh[j] += |frontier_r(u) & new_r(v)|
//
// every round, at the end of round_launch (driver.hip) after the fresh-delivery
// curve's pass: fresh_recv and fresh_sent are this matrix's row and column
// sums.  The reading side is k_fresh's: d_frx[cur] behind fpop[cur] != 0 is
// frontier_r, d_frx[cur ^ 1] behind fpop[cur ^ 1] != 0 is new_r, receivers own
// and the in-CSR is walked (a directed overlay takes the same path).  k_link:
// one-wave blocks, 64 owners each: one coalesced load of the guard words and a
// ballot, and nothing else when no owner of the chunk is live.  A live owner
// keeps its new_r row in registers as Geo<W> pieces and the wave walks its arc
// list 64 arcs at a time: column ids, the neighbours' guard words, the live
// neighbours compacted into LDS, their rows gathered LINK_RIF in flight; a lane
// whose owner piece is zero loads nothing.
//
// What is new is the output side.  The compaction drops an arc's position in
// its 64-arc chunk, so each live neighbour's position is staged beside its id
// (pos[], 64 bytes).  After group_sum<LPR> one lane per row adds the arc's
// count to link[j0 + pos] with a plain 16-bit read-modify-write, and only when
// the count is not zero.  No atomic: an arc belongs to one owner, the owners
// above hub_threshold are skipped by k_link and walked per HubItem by
// k_link_hub, and the items partition a hub's arc range -- every arc is written
// by at most one lane of one wave per round, and rounds follow each other on
// the engine stream.  The record is deterministic.  Arcs on either side of an
// item or owner boundary may share a dword; the 2-byte stores leave the other
// half alone.  Arc offsets are 64-bit throughout (C5 has 2^30 arcs).
//
// Widths.  link_fresh[j] <= m <= 4096 over a whole run: v receives each message
// for the first time once, so over all rounds arc j counts a message at most
// once.  The record is therefore u16 per arc (0.5 GB at C4, 2 GB at C5), and
// the bound is attained: on a path with every message injected at one end,
// each arc pointing away from it carries all of them.
//
// k_link_hist (gp_read_link_hist only, never in a round): link_hist[c] = arcs
// with link_fresh = c, c = 0 .. 4096, in one streaming pass, 16 bytes per lane
// and step.  A block counts its zeros in registers and the rest in an LDS
// histogram of 4,097 u32 bins, and flushes the non-zero bins with one 64-bit
// atomicAdd each; link_hist_grid keeps a block's arcs below 2^32.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gp_device.h"

namespace gp {

constexpr int LINK_RIF = 4;           // neighbour rows per lane in flight (k_fresh's, profiles/r13_fresh_cost.txt)
constexpr int LINK_BINS = 4097;       // counts 0 .. 4096
constexpr int LH_BLOCK = 256;
constexpr int LH_VEC = 8;             // u16 per 16-byte load
constexpr int64_t LH_MAX_ARCS = (int64_t)1 << 31;   // arcs one block may count (u32 bins)

struct LinkArgs {
  const int64_t* __restrict__ row_ptr;   // the in-CSR: owners are receivers
  const int32_t* __restrict__ col;
  const u64* __restrict__ own_rows;      // [n][W] new_r, valid where own_guard != 0
  const uint32_t* __restrict__ own_guard;
  const u64* __restrict__ nb_rows;       // [n][W] frontier_r, valid where nb_guard != 0
  const uint32_t* __restrict__ nb_guard;
  const HubItem* __restrict__ items;
  uint16_t* __restrict__ link;           // [nnz] the record, in-CSR arc order
  int64_t n, n_items;
  int64_t hub_thr;
};

// arcs [b, e) of one owner whose row pieces the lanes hold in `own`: every arc
// with a live sender gets popc(own row & sender row) added where it lives
template <int W>
__device__ __forceinline__ void link_arcs(const LinkArgs& a, int32_t* idx, uint8_t* pos, u64x2 own, int64_t b,
                                          int64_t e, int lane, int g, int lw) {
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
    if (u >= 0) {
      const int rk = lane_rank(m);
      idx[rk] = u;
      pos[rk] = (uint8_t)lane;   // the arc is j0 + lane
    }
    wave_sync_lds();
    const int cnt = __popcll(m);
    for (int k0 = 0; k0 < cnt; k0 += LINK_RIF * RPI) {
      u64x2 r[LINK_RIF];
#pragma unroll
      for (int q = 0; q < LINK_RIF; ++q) {
        const int k = k0 + g + q * RPI;
        r[q] = u64x2{0, 0};
        if (k < cnt && mine) r[q] = load_piece<W>(a.nb_rows, idx[k], lw);
      }
#pragma unroll
      for (int q = 0; q < LINK_RIF; ++q) {
        const uint32_t cq = (uint32_t)(__popcll(own.x & r[q].x) + __popcll(own.y & r[q].y));
        const uint32_t arc = group_sum<LPR>(cq);   // <= 4096
        if (lw == 0 && arc) {                      // (arc != 0: k < cnt)
          uint16_t* p = a.link + (j0 + (int64_t)pos[k0 + g + q * RPI]);
          *p = (uint16_t)(*p + arc);               // the run's total stays <= 4096 (header)
        }
      }
    }
    wave_sync_lds();
  }
}

template <int W>
__global__ __launch_bounds__(64) void k_link(LinkArgs a) {
  static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W: a power of two up to 64");
  constexpr int LPR = Geo<W>::LPR;
  __shared__ int32_t idx[64];
  __shared__ uint8_t pos[64];
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
  while (gm) {
    const int k = __ffsll((long long)gm) - 1;
    gm &= gm - 1;
    const int64_t bk = __shfl((long long)b, k), ek = __shfl((long long)e, k);
    if (ek == bk || ek - bk > a.hub_thr) continue;   // (a hub: k_link_hub walks its items)
    const u64x2 own = load_piece<W>(a.own_rows, v0 + k, lw);
    link_arcs<W>(a, idx, pos, own, bk, ek, lane, g, lw);
  }
}

template <int W>
__global__ __launch_bounds__(64) void k_link_hub(LinkArgs a) {
  constexpr int LPR = Geo<W>::LPR;
  __shared__ int32_t idx[64];
  __shared__ uint8_t pos[64];
  const int lane = threadIdx.x;
  const int g = lane / LPR, lw = lane % LPR;
  if ((int64_t)blockIdx.x >= a.n_items) return;
  const HubItem h = a.items[blockIdx.x];
  if (a.own_guard[h.v] == 0u) return;
  const u64x2 own = load_piece<W>(a.own_rows, h.v, lw);
  link_arcs<W>(a, idx, pos, own, h.beg, h.end, lane, g, lw);
}

// hist[c] += arcs of [0, nnz) with link[j] == c; each block strides over
// 8-arc vectors (the array is hipMalloc-aligned), block 0 takes the tail
__global__ __launch_bounds__(LH_BLOCK) void k_link_hist(const uint16_t* __restrict__ link, int64_t nnz,
                                                         u64* __restrict__ hist) {
  __shared__ uint32_t lh[LINK_BINS];
  for (int t = threadIdx.x; t < LINK_BINS; t += LH_BLOCK) lh[t] = 0u;
  __syncthreads();
  uint32_t zeros = 0;   // (most arcs of a sparse record: kept off the one hot bin)
  const int64_t nvec = nnz / LH_VEC;
  const uint4* __restrict__ vec = reinterpret_cast<const uint4*>(link);
  for (int64_t i = (int64_t)blockIdx.x * LH_BLOCK + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * LH_BLOCK) {
    const uint4 x = vec[i];
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = w[k] & 0xFFFFu, hi = w[k] >> 16;
      if (lo == 0u) ++zeros;
      else atomicAdd(&lh[min(lo, (uint32_t)LINK_BINS - 1)], 1u);   // (a count is <= 4096: the clamp only guards LDS)
      if (hi == 0u) ++zeros;
      else atomicAdd(&lh[min(hi, (uint32_t)LINK_BINS - 1)], 1u);
    }
  }
  if (blockIdx.x == 0) {
    for (int64_t j = nvec * LH_VEC + threadIdx.x; j < nnz; j += LH_BLOCK) {
      const uint32_t x = link[j];
      if (x == 0u) ++zeros;
      else atomicAdd(&lh[min(x, (uint32_t)LINK_BINS - 1)], 1u);
    }
  }
  if (zeros) atomicAdd(&lh[0], zeros);
  __syncthreads();
  for (int t = threadIdx.x; t < LINK_BINS; t += LH_BLOCK) {
    const uint32_t cnt = lh[t];
    if (cnt) atomicAdd(&hist[t], (u64)cnt);
  }
}

// blocks of k_link_hist: enough to fill the device, few enough that the flush
// is short, and never so few that one block counts LH_MAX_ARCS arcs or more
static int64_t link_hist_grid(const Ctx* c, int64_t nnz) {
  const int64_t work = (nnz / LH_VEC + LH_BLOCK - 1) / LH_BLOCK;
  int64_t grid = std::min<int64_t>(std::max<int64_t>(work, 1), (int64_t)std::max(c->cu_count, 1) * 8);
  grid = std::max<int64_t>(grid, (nnz + LH_MAX_ARCS - 1) / LH_MAX_ARCS);
  return grid;
}

static void link_free(Ctx* c) {
  dfree(&c->d_link);
  dfree(&c->d_link_hist);
  c->link_arcs = 0;
  record_off(c->rec[R_LINK]);
}

// gp_reset: gp_track_link_fresh takes effect (u16[nnz] and the histogram's
// u64[4097], or nothing), cleared.  A new overlay freed the array
// (finish_graph), so it is sized for the arcs of this one.  The exact frontier
// rows are alloc_state's (setup.hip: frx_rows)
static int link_reset(Ctx* c) {
  const size_t arcs = (size_t)c->nnz;
  if (!c->d_link || c->link_arcs != arcs) {
    link_free(c);
    if (dalloc(&c->d_link, arcs) != 0 || dalloc(&c->d_link_hist, (size_t)LINK_BINS) != 0) {
      link_free(c);
      return GP_ENOMEM;
    }
    c->link_arcs = arcs;
  }
  if (arcs) GP_HIP(hipMemsetAsync(c->d_link, 0, arcs * sizeof(uint16_t), c->stream));
  return 0;
}

template <int W>
static void launch_link_w(Ctx* c, const LinkArgs& a) {
  hipStream_t s = c->stream;
  hipLaunchKernelGGL((k_link<W>), dim3(grid_for(a.n, 64)), dim3(64), 0, s, a);
  if (a.n_items > 0) hipLaunchKernelGGL((k_link_hub<W>), dim3(grid_for(a.n_items, 1)), dim3(64), 0, s, a);
}

// after E_r: round r's first-receipt deliveries, added to the arcs they came over
static int link_count_round(Ctx* c) {
  if (c->n <= 0 || c->nnz <= 0) return 0;
  GP_TRY(record_need_rows(c, link_record, c->n));
  const int cur = c->cur;
  LinkArgs a{};
  a.row_ptr = c->d_row_ptr;
  a.col = c->d_col;
  a.own_rows = c->d_frx[cur ^ 1];
  a.own_guard = c->d_fpop[cur ^ 1];
  a.nb_rows = c->d_frx[cur];
  a.nb_guard = c->d_fpop[cur];
  a.items = c->d_hub_items;
  a.link = c->d_link;
  a.n = c->n;
  a.n_items = c->n_hub_items;
  a.hub_thr = c->cfg.hub_threshold;
  GP_TRY(with_words(c->words, [&](auto w) { launch_link_w<w()>(c, a); }));
  GP_HIP(hipGetLastError());
  return 0;
}

GP_RECORD_OPS(link_record) = {R_LINK, "per-link fresh deliveries", "gp_track_link_fresh", true, 4, nullptr, nullptr,
                               link_reset, link_free, link_count_round, nullptr, nullptr};

int link_read(Ctx* c, void* host, int64_t bytes) {
  GP_TRY(record_readable(c, link_record));
  if (bytes != c->nnz * 2) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(c->nnz * 2));
  if (bytes == 0) return 0;
  return copy_sync(c, host, c->d_link, (size_t)bytes, hipMemcpyDeviceToHost);
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_track_link_fresh(gp_ctx* c, int32_t on) { return record_track(c, link_record, on); }

int gp_read_link_hist(gp_ctx* c, uint64_t* hist, int32_t bins) {
  if (!c || !hist) return set_error(GP_EINVAL, "null argument");
  GP_TRY(record_readable(c, link_record));
  if (bins != LINK_BINS) return set_error(GP_EINVAL, "bins must be " + std::to_string(LINK_BINS));
  GP_HIP(hipSetDevice(c->device));
  GP_HIP(hipMemsetAsync(c->d_link_hist, 0, (size_t)LINK_BINS * 8, c->stream));
  if (c->nnz > 0) {
    hipLaunchKernelGGL(k_link_hist, dim3((unsigned)link_hist_grid(c, c->nnz)), dim3(LH_BLOCK), 0, c->stream,
                       (const uint16_t*)c->d_link, c->nnz, c->d_link_hist);
    GP_HIP(hipGetLastError());
  }
  return copy_sync(c, hist, c->d_link_hist, (size_t)LINK_BINS * 8, hipMemcpyDeviceToHost);
}

}  // extern "C"
