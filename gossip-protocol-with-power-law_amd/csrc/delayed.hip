// delayed.hip -- the expansion E_r over links that take one to eight rounds
// (DESIGN.md §2.2, §3.19): next[v] = OR over v's in-neighbours u of
// frontier_{r + 1 - d(u, v)}[u], & ~seen[v], with d(u, v) the per-link delay of
// link_delay.h.  A receiver gathers exact frontier rows of up to dmax past
// rounds, chosen per arc; with loss on as well, the line sent in round s
// arrives iff arc u -> v was open in round s (link_loss.h's draw, unchanged).
//
// The ring.  Frontier rows of round s live in d_lag_frx[s % (dmax + 1)]: dmax
// rounds to read and the one this round's commits write.  Every other reader of
// d_frx[cur] / d_frx[cur ^ 1] (injection, forwards, curve, delays, frontier())
// stays as it is, because lag_rotate points those two at the ring's slots of
// rounds r and r + 1 before the round is enqueued.  A frontier row is valid
// only behind its guard and fpop is overwritten every round, so the guard of
// round s is kept as k_mkbits made it in round s -- after L_s and I_s -- in row
// s % dmax of d_lag_bits (k_lag_bits copies it there and rebuilds the OR of all
// rows, which the lane phase's prefilter probes).  A line already sent still
// arrives if its sender crashes later; a receiver down in the arrival round
// loses it for good (the receiver's eligibility is this round's).
//
// k_arc_delays writes d(u, v) as one byte per arc of the in-CSR at gp_reset, so
// a round loads it coalesced beside the column id instead of drawing.
// k_expand_delayed: k_expand_lossy's lane phase and commit (finish_row,
// commit_vertices: every output of a commit comes from the same code).  Per
// in-arc a lane loads the column id and the delay byte, tests the sender's bit
// in the bitmap of round r + 1 - d, makes that round's loss draw when loss is
// on, and stages (d - 1) << 28 | u into LDS; the 16-B pieces of the staged rows
// are then gathered from the ring slot the entry names, RowsInFlight<W>
// wave-instructions in flight.  (28 bits of sender id: gp_reset refuses delay
// on more than 2^28 local vertices.)  The per-delay tables -- bitmap, ring slot
// and loss key of send round r + 1 - d -- travel in LagArgs, a block of their
// own beside ExpandArgs, and are copied to LDS once per wave so that a lane can
// index them by its arc's delay.
// k_hub_delayed: receivers above hub_threshold over the hub table, committed by
// the push's tail as k_hub_lossy's are.
// The narrow-row groups of lossy.hip (lossy_groups) are not built here.
//
// Also the delay setting's half of the C-ABI (gp_link_delay,
// gp_link_delay_info), what gp_reset does with it (lag_reset, lag_prepare) and
// the GP_ARC_DELAY read.
#include "gp_device.h"
#include "link_delay.h"
#include "link_loss.h"

namespace gp {

constexpr int LAG_ID_BITS = 28;
constexpr int32_t LAG_ID_MASK = (1 << LAG_ID_BITS) - 1;

// one delayed round's arguments beside the pull's block; entry d - 1 of each
// table belongs to send round r + 1 - d (an all-zero bitmap while that is < 0)
struct LagArgs {
  const u64* frx[LINK_DELAY_MAX];    // exact frontier rows of the send round, valid behind its bitmap
  const u64* bits[LINK_DELAY_MAX];   // k_mkbits' activity bitmap of the send round
  uint64_t key[LINK_DELAY_MAX];      // loss_round_key of the send round (loss on)
  const u64* __restrict__ any;       // OR of the live bitmaps
  const uint8_t* __restrict__ arc;   // [nnz] d(u, v)
  uint64_t thresh;                   // open iff draw >= thresh (loss on)
  int32_t lossy;                     // loss is in force: draw per arc behind a set guard
  int32_t closed;                    // p = 1: every arc closed
};

struct LagLds {
  const u64* frx[LINK_DELAY_MAX];
  const u64* bits[LINK_DELAY_MAX];
  uint64_t key[LINK_DELAY_MAX];
};

// (static indices: the argument block stays in scalar registers)
__device__ __forceinline__ void lag_tables(const LagArgs& la, LagLds& T, int lane) {
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < LINK_DELAY_MAX; ++d) {
      T.frx[d] = la.frx[d];
      T.bits[d] = la.bits[d];
      T.key[d] = la.key[d];
    }
  }
  wave_sync_lds();
}

// arcs [b, e) of receiver v's in-list: OR of the rows that arrive this round
template <int W>
__device__ __forceinline__ void lag_scan(const ExpandArgs& a, const LagArgs& la, const LagLds& T, int v, int64_t b,
                                         int64_t e, WaveLds& L, int lane, int g, int lw, u64x2& acc, WaveStats& st) {
  constexpr int RPI = Geo<W>::RPI;
  constexpr int RIF = RowsInFlight<W>::value;
  for (int64_t j0 = b; j0 < e; j0 += 64) {
    const int n = (int)min((int64_t)64, e - j0);
    st.add(S_ARCS, n);
    int32_t ent = -1;
    if (lane < n && !la.closed) {
      const int32_t u = a.col[j0 + lane];
      const int d = (int)la.arc[j0 + lane] - 1;   // 0 .. dmax - 1 (k_arc_delays)
      // (a crash zeroes fpop before k_mkbits: a vertex down in its send round was no sender)
      if (((T.bits[d][u >> 6] >> (u & 63)) & 1ull) &&
          (!la.lossy || arc_open(T.key[d], (uint32_t)(a.vbegin + u), (uint32_t)(a.vbegin + v), la.thresh)))
        ent = (d << LAG_ID_BITS) | u;
    }
    const int cnt = stage_pass(L, ent);
    if (cnt == 0) continue;
    for (int k0 = 0; k0 < cnt; k0 += RIF * RPI) {
      u64x2 r[RIF];
      u64 pieces = 0;
#pragma unroll
      for (int q = 0; q < RIF; ++q) {
        const int k = k0 + g + q * RPI;
        r[q] = u64x2{0, 0};
        if (k < cnt) {
          const int32_t s = L.idx[k];
          r[q] = load_piece<W>(T.frx[s >> LAG_ID_BITS], s & LAG_ID_MASK, lw);
        }
        pieces += line_pieces<W>(__ballot(k < cnt));
      }
#pragma unroll
      for (int q = 0; q < RIF; ++q) acc |= r[q];
      st.add(S_GATHERED, (u64)min(RIF * RPI, cnt - k0));
      st.add(S_ROW_BYTES, pieces * (u64)(8 * Geo<W>::WPL));
    }
    wave_sync_lds();   // L.idx is restaged by the next pass
  }
}

template <int W>
__global__ EXPAND_BOUNDS void k_expand_delayed(ExpandArgs a, LagArgs la) {
  constexpr int LPR = Geo<W>::LPR;
  __shared__ WaveLds s_w[EWAVES];
  __shared__ LagLds s_t[EWAVES];
  const int lane = threadIdx.x & 63;
  const int wib = uniform(threadIdx.x >> 6);
  const int g = lane / LPR, lw = lane % LPR;
  WaveLds& L = s_w[wib];
  LagLds& T = s_t[wib];
  WaveStats st;
  ws_zero<EWAVES>(st);
  const int64_t base = ((int64_t)blockIdx.x * EWAVES + wib) * 64;
  if (base < a.nloc) {
    const int64_t li = base + lane;
    const bool valid = li < a.nloc;
    bool need = false, act = false;
    u64 sends = 0;
    uint32_t slot_of = SLOT_NONE;
    uint32_t pre_arcs = 0;   // arcs the lane phase probed for the receivers it dropped
    if (valid) {
      const int v = (int)(a.vbegin + li);
      const uint32_t fp = a.fpop[v];
      act = fp != 0u;
      // attempted sends, counted in the send round
      if (act) sends = (u64)fp * (u64)(uint32_t)max(a.deg_live[v], 0);
      const int64_t b = a.row_ptr[v], e = a.row_ptr[v + 1];
      L.rp[lane] = b;
      if (lane == 63 || li + 1 == a.nloc) L.rp[lane + 1] = e;
      const bool hub = e - b > a.hub_thr;   // split over waves by k_hub_delayed
      need = !(a.state[v] & ST_DOWN) && a.seenpop[li] < a.done_at[v] && !hub && e > b && !la.closed;
      if (need && e - b <= PRE_MAX_DEG) {   // no in-neighbour sent in any live round: nothing to scan
        const int deg = (int)(e - b);
        bool any = false;
#pragma unroll
        for (int h = 0; h < PRE_MAX_DEG / PRE_IDS; ++h) {
          if (h * PRE_IDS < deg) {
            int32_t c[PRE_IDS];
            u64 w[PRE_IDS];
#pragma unroll
            for (int q = 0; q < PRE_IDS; ++q) c[q] = h * PRE_IDS + q < deg ? a.col[b + h * PRE_IDS + q] : -1;
#pragma unroll
            for (int q = 0; q < PRE_IDS; ++q) w[q] = c[q] >= 0 ? la.any[c[q] >> 6] : 0ull;
#pragma unroll
            for (int q = 0; q < PRE_IDS; ++q) any = any || (c[q] >= 0 && ((w[q] >> (c[q] & 63)) & 1ull));
          }
        }
        if (!any) {
          need = false;
          pre_arcs = (uint32_t)deg;
        }
      }
      slot_of = a.sp[v];
    }
    st.add(S_ARCS, (u64)wave_sum_u32(pre_arcs));
    st.add(S_SENDS, wave_sum_u64(sends));
    st.add(S_ACTIVE, (u64)__popcll(__ballot(act)));
    st.add(S_VISITED, (u64)__popcll(__ballot(need)));
    L.tot[lane] = 0u;
    L.dig[lane] = 0ull;
    L.lmn[lane] = 0;
    alive_zero<W>(a, L.alive, lane);
    lag_tables(la, T, lane);   // (syncs the wave's LDS)
    u64 m = __ballot(need);
    while (m) {
      const int k = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int64_t i = base + k;
      const int v = uniform((int)(a.vbegin + i));
      const uint32_t sv_slot = (uint32_t)__builtin_amdgcn_readlane((int)slot_of, k);
      u64x2 acc = {0, 0};
      lag_scan<W>(a, la, T, v, L.rp[k], L.rp[k + 1], L, lane, g, lw, acc, st);
      reduce_slots<W>(acc);
      finish_row<W, true, false>(a, v, i, acc, lane, g, lw, st, L, false, sv_slot, k);
    }
    alive_flush<W>(a, L.alive, lane);
    commit_vertices(a, L, li, need, st);   // (fpop_next of every other vertex was zeroed before the launch)
  }
  flush_stats<EWAVES>(st, a.partial);
}

// receivers above hub_threshold: one wave per item of the hub table
template <int W>
__global__ __launch_bounds__(64) void k_hub_delayed(ExpandArgs a, LagArgs la) {
  constexpr int LPR = Geo<W>::LPR;
  constexpr int WPL = Geo<W>::WPL;
  __shared__ WaveLds s_w[1];
  __shared__ LagLds s_t[1];
  const int lane = threadIdx.x & 63;
  const int g = lane / LPR, lw = lane % LPR;
  WaveStats st;
  ws_zero<1>(st);
  const int64_t it = (int64_t)blockIdx.x;
  if (it < a.n_items) {
    const HubItem h = a.hub_items[it];
    const int64_t i = h.v - a.vbegin;
    if (!(a.state[h.v] & ST_DOWN) && a.seenpop[i] < a.done_at[h.v]) {
      lag_tables(la, s_t[0], lane);
      u64x2 acc = {0, 0};
      lag_scan<W>(a, la, s_t[0], h.v, h.beg, h.end, s_w[0], lane, g, lw, acc, st);
      reduce_slots<W>(acc);
      const u64 wx = __ballot(g == 0 && acc.x != 0ull), wy = __ballot(g == 0 && acc.y != 0ull);
      if (wx | wy) {
        // order-free, so bit-exact; the row is read and zeroed again by k_apply
        if (g == 0) {
          u64* row = a.acc + (size_t)h.v * W + lw * WPL;   // (indexed by v, as push_arcs and k_apply do)
          if (acc.x) atomicOr(row, acc.x);
          if (WPL == 2 && acc.y) atomicOr(row + 1, acc.y);
        }
        if (lane == 0) atomicOr(&a.tbits[h.v >> 6], 1ull << (h.v & 63));
        st.add(S_ATOMICS, (u64)(__popcll(wx) + __popcll(wy) + 1));
      }
    }
  }
  flush_stats<1>(st, a.partial);
}

// d(u, v) of every arc of the in-CSR: one wave per receiver, its in-list 64 arcs a step
__global__ __launch_bounds__(BLOCK) void k_arc_delays(const int64_t* __restrict__ row_ptr,
                                                      const int32_t* __restrict__ col, int64_t n, uint64_t key,
                                                      uint32_t dmax, uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * WAVES;
  for (int64_t v = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); v < n; v += stride) {
    const int64_t b = row_ptr[v], e = row_ptr[v + 1];
    for (int64_t j = b + lane; j < e; j += 64) out[j] = (uint8_t)arc_delay(key, (uint32_t)col[j], (uint32_t)v, dmax);
  }
}

// this round's bitmap into its row of the ring, and the OR of the ring's rows
__global__ __launch_bounds__(BLOCK) void k_lag_bits(const u64* __restrict__ abits, u64* __restrict__ ring,
                                                    int64_t nw, int32_t dmax, int32_t row) {
  const int64_t w = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (w >= nw) return;
  const u64 x = abits[w];
  u64 any = x;
  for (int32_t k = 0; k < dmax; ++k)
    if (k != row) any |= ring[(size_t)k * nw + w];
  ring[(size_t)row * nw + w] = x;
  ring[(size_t)dmax * nw + w] = any;
}

template <int W>
void launch_expand_delayed_w(Ctx* c, const ExpandArgs& a) {
  const int32_t r = c->round, dmax = c->lag_dmax, R = c->lag_ring;   // (launch_expand checked lag_ready)
  const size_t nw = (size_t)c->lag_nw;
  LagArgs la{};
  for (int32_t d = 1; d <= LINK_DELAY_MAX; ++d) {
    const int32_t s = r + 1 - std::min(d, dmax);   // (entries above dmax are never indexed: the arc bytes are <= dmax)
    la.frx[d - 1] = c->d_lag_frx[((s % R) + R) % R];
    la.bits[d - 1] = c->d_lag_bits + (size_t)(((s % dmax) + dmax) % dmax) * nw;
    la.key[d - 1] = c->loss_on && s >= 0 ? loss_round_key(c->loss_seed, (uint32_t)s) : 0ull;
  }
  la.any = c->d_lag_bits + (size_t)dmax * nw;
  la.arc = c->d_lag_arc;
  la.thresh = c->loss_on ? loss_threshold(c->loss_p) : 0ull;
  la.lossy = c->loss_on ? 1 : 0;
  la.closed = c->loss_on && c->loss_p >= 1.0 ? 1 : 0;
  hipStream_t s = c->stream;
  (void)hipEventRecord(c->ev[4], s);
  hipLaunchKernelGGL(k_lag_bits, dim3(grid_for((int64_t)nw, BLOCK)), dim3(BLOCK), 0, s, (const u64*)c->d_abits,
                     c->d_lag_bits, (int64_t)nw, dmax, r % dmax);
  if (c->n_hub_items > 0) {   // first: their chains are the round's longest
    ExpandArgs h = a;
    h.n_items = c->n_hub_items;
    hipLaunchKernelGGL(k_hub_delayed<W>, dim3(grid_for(h.n_items, 1)), dim3(64), 0, s, h, la);
  }
  if (a.nloc > 0)
    hipLaunchKernelGGL(k_expand_delayed<W>, dim3(grid_for(a.nloc, (int64_t)EWAVES * 64)), dim3(EBLOCK), 0, s, a, la);
  if (c->n_hub_items > 0) launch_apply_touched_w<W>(c, a);
  (void)hipEventRecord(c->ev[5], s);
}
#define V(W) template void launch_expand_delayed_w<W>(Ctx*, const ExpandArgs&);
V(1) V(2) V(4) V(8) V(16) V(32) V(64)
#undef V

// gp_reset, before anything changes: the request can become the setting in
// force (lag_prepare makes it so) -- or the reset is refused
int lag_reset(Ctx* c) {
  if (c->lag_want) {
    if (const RecordOps* rec = records_arc_walker(c))
      return set_error(GP_EINVAL, std::string("link delay is on and so is ") + rec->call +
                                      ": the record walks arcs and takes every line to arrive in its send round");
    if (c->local || c->nranks > 1)
      return set_error(GP_EINVAL, "link delay is not supported in a vertex-partitioned context");
    if (c->jnranks > 0)
      return set_error(GP_EINVAL, "link delay is not supported in a message-shard job (gp_shard_*): the job record "
                                  "takes a round's receivers to have heard that round's senders");
    if (c->n_alloc > ((int64_t)1 << LAG_ID_BITS))
      return set_error(GP_EINVAL, "link delay: more than 2^28 vertices (the staged sender ids carry the ring slot)");
  }
  return 0;
}

void lag_release(Ctx* c) {
  if (c->lag_ring > 0) {   // (whatever the rotation left in d_frx: the ring's first two are alloc_state's)
    c->d_frx[0] = c->d_lag_frx[0];
    c->d_frx[1] = c->d_lag_frx[1];
    for (int32_t k = 2; k < c->lag_ring; ++k) dfree(&c->d_lag_frx[k]);
  }
  for (u64*& p : c->d_lag_frx) p = nullptr;
  c->lag_ring = 0;
  c->lag_nw = 0;
  dfree(&c->d_lag_bits);
  dfree(&c->d_lag_arc);
}

bool lag_ready(const Ctx* c) {
  return c->lag_ring == c->lag_dmax + 1 && c->d_lag_bits && c->d_lag_arc && c->d_frx[0] && c->frx_rows >= c->n_alloc &&
         c->jnranks == 0;
}

void lag_rotate(Ctx* c) {
  if (!c->lag_on || c->lag_ring < 2) return;
  c->d_frx[c->cur] = c->d_lag_frx[c->round % c->lag_ring];
  c->d_frx[c->cur ^ 1] = c->d_lag_frx[(c->round + 1) % c->lag_ring];
}

// with the run state in place (alloc_state kept the frontier rows: lag_want)
int lag_prepare(Ctx* c) {
  c->lag_hist = 0;
  c->lag_on = false;   // (until the ring stands: the setting in force and the ring always agree)
  c->lag_dmax = 1;
  c->lag_seed = 0;
  if (!c->lag_want) {
    lag_release(c);
    return 0;
  }
  const int32_t R = c->lag_dmax_want + 1;
  const int64_t nw = (c->n_alloc + 63) / 64;
  if (c->lag_ring != R || c->lag_nw != nw) {
    lag_release(c);
    if (!c->d_frx[0] || !c->d_frx[1] || c->frx_rows < c->n_alloc)
      return set_error(GP_ESTATE, "internal: link delay without frontier rows");
    int rc = dalloc(&c->d_lag_bits, (size_t)R * (size_t)nw);
    if (rc == 0) rc = dalloc(&c->d_lag_arc, (size_t)std::max<int64_t>(c->nnz_l, 1));
    u64* own[9] = {};
    for (int32_t k = 2; k < R && rc == 0; ++k) rc = dalloc(&own[k], (size_t)c->frx_rows * (size_t)c->words);
    if (rc != 0) {   // (GP_ENOMEM: nothing of the ring stays and no delay is in force; the request stands for the next gp_reset)
      for (int32_t k = 2; k < R; ++k) dfree(&own[k]);
      dfree(&c->d_lag_bits);
      dfree(&c->d_lag_arc);
      (void)hipGetLastError();
      return rc;
    }
    c->d_lag_frx[0] = c->d_frx[0];
    c->d_lag_frx[1] = c->d_frx[1];
    for (int32_t k = 2; k < R; ++k) c->d_lag_frx[k] = own[k];
    c->lag_ring = R;
    c->lag_nw = nw;
  }
  c->lag_on = true;
  c->lag_dmax = c->lag_dmax_want;
  c->lag_seed = c->lag_seed_want;
  c->d_frx[0] = c->d_lag_frx[0];   // round 0, cur 0
  c->d_frx[1] = c->d_lag_frx[1];
  hipStream_t s = c->stream;
  GP_HIP(hipMemsetAsync(c->d_lag_bits, 0, (size_t)R * (size_t)nw * 8, s));   // frontier_s is empty for s < 0
  if (c->nnz_l > 0)
    hipLaunchKernelGGL(k_arc_delays, dim3(std::max(1, std::min(grid_for(c->nloc(), WAVES), c->cu_count * 8 * GS))),
                       dim3(BLOCK), 0, s, (const int64_t*)c->d_row_ptr, (const int32_t*)c->d_col, c->nloc(),
                       link_delay_key(c->lag_seed), (uint32_t)c->lag_dmax, c->d_lag_arc);
  GP_HIP(hipGetLastError());
  return 0;
}

// send rounds s in [round + 1 - dmax, round - 1] with a sender: their lines may
// still arrive.  lag_hist is the run's own record (bit k: round - 1 - k had a
// sender; round_collect shifts it), so nothing that clears the kept round stats
// -- a shard transport joined mid-run -- changes the count
int32_t lag_in_flight(const Ctx* c) {
  if (!c->lag_on) return 0;
  return __builtin_popcount(c->lag_hist & ((1u << (c->lag_dmax - 1)) - 1u));
}

// before a round is enqueued: the ring the setting in force needs is there
int lag_check_round(const Ctx* c) {
  if (!c->lag_on || lag_ready(c)) return 0;
  if (c->jnranks > 0)
    return set_error(GP_ESTATE, "link delay is in force and a message-shard job (gp_shard_*) was joined since the "
                                "reset: not supported together, gp_reset refuses it by name");
  return set_error(GP_ESTATE, "link delay is in force but its frontier-row ring is gone: gp_reset first");
}

int lag_read(Ctx* c, void* host, int64_t bytes) {
  if (!c->lag_on || !c->d_lag_arc || c->lag_ring == 0)
    return set_error(GP_ENOTRACK, "link delay is off for the current run (gp_link_delay, then gp_reset)");
  if (bytes != c->nnz_l) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(c->nnz_l));
  if (bytes) GP_TRY(copy_sync(c, host, c->d_lag_arc, (size_t)bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_link_delay(gp_ctx* c, int32_t on, int32_t dmax, uint64_t seed) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (dmax < 1 || dmax > LINK_DELAY_MAX) return set_error(GP_EINVAL, "link delay: dmax must lie in [1, 8]");
  c->lag_want = on != 0;
  c->lag_dmax_want = on ? dmax : 1;
  c->lag_seed_want = on ? seed : 0;
  return 0;
}

int gp_link_delay_info(gp_ctx* c, int32_t* on, int32_t* dmax, uint64_t* seed, int32_t* in_flight) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (on) *on = c->lag_on ? 1 : 0;
  if (dmax) *dmax = c->lag_dmax;
  if (seed) *seed = c->lag_seed;
  if (in_flight) *in_flight = lag_in_flight(c);
  return 0;
}

}  // extern "C"
