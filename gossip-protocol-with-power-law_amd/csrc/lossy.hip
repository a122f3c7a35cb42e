// lossy.hip -- the expansion E_r over links that drop gossip (DESIGN.md §2.2,
// §3.18): next[v] = OR over v's in-neighbours u with arc u -> v open in round r
// of frontier_r[u], & ~seen[v].  The pull of pull.hip reads whole Message-Lists,
// which is exact only while every line arrives (forward-once, §3.1); here a
// line on a closed arc is lost for good, so the receivers read the senders'
// *exact frontier rows* (Ctx::d_frx, kept because holds_frx() includes the loss
// request) through the per-arc draw of link_loss.h.  The receiver side is the
// pull's own: finish_row and commit_vertices, so every output a commit feeds
// (seen rows, frontier rows, first bytes, digest, popcounts, alive sets) is
// produced by the same code.
//
// k_expand_lossy: one-wave blocks over 64 consecutive receivers.  The lane
// phase does the per-vertex work with coalesced loads -- every owned vertex's
// sender accounting, the receiver's eligibility -- and the wave then walks the
// in-list of each eligible receiver 64 arcs per pass: a lane loads the column
// id and the sender's guard -- its bit of the activity bitmap k_mkbits built
// from fpop[cur] before the round (bit u = fpop[u] != 0; 2 MB at 2^24 against
// 64 MB of guard words) -- computes the draw only behind a set guard, the open
// live senders are compacted into LDS and their frontier rows gathered as 16-B
// pieces, RowsInFlight<W> wave-instructions in flight, OR-reduced over the row
// slots.  One shortcut survives loss and changes no output: the lane phase
// probes the guards of receivers of in-degree <= PRE_MAX_DEG itself, all loads
// in flight together, and drops those with no sending in-neighbour from the
// wave's serial loop (the sparse rounds).  Stopping a receiver once its OR
// covers cmask & ~seen is valid too, but frontier rows seldom cover a target:
// it saved 5 % of C4's rows at p = 0, none at p = 0.1, and is not built.
// At W <= 16 the receivers with short in-lists go several per wave step
// (lossy_groups).
// k_hub_lossy: receivers above hub_threshold, one wave per HubItem; the item's
// partial OR goes into the accumulator row with atomicOr on its nonzero words
// plus the receiver's tbits bit, and the push's tail (k_touch_list, k_apply /
// k_apply_lanes: push.hip launch_apply_touched_w) commits them and leaves the
// accumulator all-zero.
//
// Also the loss setting's half of the C-ABI (gp_link_loss, gp_link_loss_info)
// and what gp_reset does with it (loss_reset).
#include "gp_device.h"
#include "link_loss.h"
#include "lossy_scan.h"

namespace gp {

// Narrow rows (W <= 16): the receivers of in-degree <= GROUP_CHUNKS * LPR go
// RPI per wave step, one per row slot, as k_apply_lanes takes the push's
// receivers: a whole wave per receiver leaves most lanes of the gather and of
// the commit idle.  Slot g's LPR lanes walk their receiver's in-list LPR arcs
// per chunk (lane lw: the arc's column id, guard bit and draw), then every lane
// of the slot loads its 16-B piece of each open live sender's frontier row.
// The commit is k_apply_lanes' -- new = acc & ~seen, the rows, first bytes and
// digest per slot, reduced over the slot's lanes -- with the per-vertex words
// left in L.tot / L.dig for commit_vertices.  All control flow is
// wave-uniform (the chunk and sender loops have compile-time bounds, the work
// is predicated), so every lane is active in every shuffle.
constexpr int GROUP_CHUNKS = 4;
template <int W>
__device__ __forceinline__ void lossy_groups(const ExpandArgs& a, const LossArgs& la, WaveLds& L, u64 mg, int64_t base,
                                             uint32_t slot_of, WaveStats& st) {
  constexpr int LPR = Geo<W>::LPR;
  constexpr int RPI = Geo<W>::RPI;
  constexpr int WPL = Geo<W>::WPL;
  const int lane = threadIdx.x & 63;
  const int g = lane / LPR, lw = lane % LPR;
  u64 narcs = 0, nrows = 0, nbits = 0, nrecv = 0, nseen = 0;
  while (mg) {
    const int left = __popcll(mg);
    const bool on = g < left;   // slot g takes the (g + 1)-th receiver of the mask
    const int k = on ? select_bit(mg, g + 1) : 0;
    if (left <= RPI) mg = 0ull;
    else mg &= ~((2ull << select_bit(mg, RPI)) - 1ull);
    const int v = (int)(a.vbegin + base + k);
    const int64_t b = L.rp[k], e = on ? L.rp[k + 1] : b;
    const uint32_t sslot = (uint32_t)__shfl((int)slot_of, k);
    if (lw == 0) narcs += (u64)(e - b);
    u64x2 acc = {0, 0};
#pragma unroll
    for (int c = 0; c < GROUP_CHUNKS; ++c) {
      const int64_t j = b + c * LPR + lw;
      int32_t u = -1;
      if (j < e) {
        u = a.col[j];
        if (!(((a.abits[u >> 6] >> (u & 63)) & 1ull) &&
              arc_open(la.d.key, (uint32_t)(a.vbegin + u), (uint32_t)v, la.d.thresh)))
          u = -1;
      }
      if (u >= 0) ++nrows;
#pragma unroll
      for (int t = 0; t < LPR; ++t) {
        const int32_t ut = __shfl(u, g * LPR + t);
        if (ut >= 0) acc |= load_piece<W>(la.frx, ut, lw);
      }
    }
    const bool any = group_or<LPR>((acc.x | acc.y) != 0ull);
    u64x2 sv = {0, 0};
    if (any && sslot != SLOT_NONE) sv = load_piece<W>(a.slot[sslot], v, lw);
    const u64x2 nw = acc & ~sv;
    const uint32_t tot = group_sum<LPR>((uint32_t)(__popcll(nw.x) + __popcll(nw.y)));
    u64 t = 0;
    if (tot) {
      alive_add<W>(a, L, lw, nw);
      store_piece<W>(a.slot[a.wslot], v, lw, sv | nw);   // the whole row: the slot may hold an older one
      if (a.frx_next) store_piece<W>(a.frx_next, v, lw, nw);
      if (a.first) {
        uint8_t* row = a.first + (size_t)(base + k) * (W * 64);
        if (nw.x) set_first_bytes(row, lw * WPL, nw.x, (uint32_t)a.rr);
        if (WPL == 2 && nw.y) set_first_bytes(row, lw * WPL + 1, nw.y, (uint32_t)a.rr);
      }
      if (a.digest) {
        if (nw.x) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + lw * WPL), nw.x);
        if (WPL == 2 && nw.y) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + lw * WPL + 1), nw.y);
      }
    }
    t = group_xor<LPR>(t);
    if (on && lw == 0) {
      L.tot[k] = tot;
      L.dig[k] = t;
      nbits += tot;
      nrecv += tot ? 1 : 0;
      nseen += (any && sslot != SLOT_NONE) ? 1 : 0;
    }
  }
  nrows = wave_sum_u64(nrows);
  st.add(S_ARCS, wave_sum_u64(narcs));
  st.add(S_GATHERED, nrows);
  st.add(S_ROW_BYTES, nrows * (u64)(8 * W));
  st.add(S_NEW_BITS, wave_sum_u64(nbits));
  nrecv = wave_sum_u64(nrecv);
  st.add(S_RECEIVERS, nrecv);
  st.add(S_WRITTEN, nrecv);
  st.add(S_SEEN_READ, wave_sum_u64(nseen));
}

template <int W>
__global__ EXPAND_BOUNDS void k_expand_lossy(ExpandArgs a, LossArgs la) {
  constexpr int LPR = Geo<W>::LPR;
  __shared__ WaveLds s_w[EWAVES];
  const int lane = threadIdx.x & 63;
  const int wib = uniform(threadIdx.x >> 6);
  const int g = lane / LPR, lw = lane % LPR;
  WaveLds& L = s_w[wib];
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
    bool small = false;      // W <= 16: short in-list, taken by lossy_groups
    if (valid) {
      const int v = (int)(a.vbegin + li);
      const uint32_t fp = a.fpop[v];
      act = fp != 0u;
      // attempted sends: a line on a closed arc was still sent
      if (act) sends = (u64)fp * (u64)(uint32_t)max(a.deg_live[v], 0);
      const int64_t b = a.row_ptr[v], e = a.row_ptr[v + 1];
      L.rp[lane] = b;
      if (lane == 63 || li + 1 == a.nloc) L.rp[lane + 1] = e;
      const bool hub = e - b > a.hub_thr;   // split over waves by k_hub_lossy
      need = !(a.state[v] & ST_DOWN) && a.seenpop[li] < a.done_at[v] && !hub && e > b && !la.d.closed;
      if (need && e - b <= PRE_MAX_DEG) {   // no sending in-neighbour: nothing to scan
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
            for (int q = 0; q < PRE_IDS; ++q) w[q] = c[q] >= 0 ? a.abits[c[q] >> 6] : 0ull;
#pragma unroll
            for (int q = 0; q < PRE_IDS; ++q) any = any || (c[q] >= 0 && ((w[q] >> (c[q] & 63)) & 1ull));
          }
        }
        if (!any) {
          need = false;
          pre_arcs = (uint32_t)deg;
        }
      }
      small = need && e - b <= GROUP_CHUNKS * LPR;
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
    wave_sync_lds();
    u64 m = __ballot(need);
    if constexpr (W <= 16) {   // short in-lists RPI receivers per step, the rest below
      const u64 mg = __ballot(small);
      if (mg) {
        lossy_groups<W>(a, la, L, mg, base, slot_of, st);
        m &= ~mg;
      }
    }
    while (m) {
      const int k = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int64_t i = base + k;
      const int v = uniform((int)(a.vbegin + i));
      const uint32_t sv_slot = (uint32_t)__builtin_amdgcn_readlane((int)slot_of, k);
      u64x2 acc = {0, 0};
      lossy_scan<W>(a, la, v, L.rp[k], L.rp[k + 1], L, lane, g, lw, acc, st);
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
__global__ __launch_bounds__(64) void k_hub_lossy(ExpandArgs a, LossArgs la) {
  constexpr int LPR = Geo<W>::LPR;
  constexpr int WPL = Geo<W>::WPL;
  __shared__ WaveLds s_w[1];
  const int lane = threadIdx.x & 63;
  const int g = lane / LPR, lw = lane % LPR;
  WaveStats st;
  ws_zero<1>(st);
  const int64_t it = (int64_t)blockIdx.x;
  if (it < a.n_items) {
    const HubItem h = a.hub_items[it];
    const int64_t i = h.v - a.vbegin;
    if (!(a.state[h.v] & ST_DOWN) && a.seenpop[i] < a.done_at[h.v]) {
      u64x2 acc = {0, 0};
      lossy_scan<W>(a, la, h.v, h.beg, h.end, s_w[0], lane, g, lw, acc, st);
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

// the hub items' kernel alone (a repair round launches it behind its offers, repair.hip)
template <int W>
void launch_hub_lossy_w(Ctx* c, const ExpandArgs& a, const LossArgs& la) {
  if (c->n_hub_items <= 0) return;
  ExpandArgs h = a;
  h.n_items = c->n_hub_items;
  hipLaunchKernelGGL(k_hub_lossy<W>, dim3(grid_for(h.n_items, 1)), dim3(64), 0, c->stream, h, la);
}

template <int W>
void launch_expand_lossy_w(Ctx* c, const ExpandArgs& a) {
  LossArgs la;
  la.frx = c->d_frx[c->cur];
  la.d = loss_draw(c->loss_p, c->loss_seed, (uint32_t)c->round);
  hipStream_t s = c->stream;
  (void)hipEventRecord(c->ev[4], s);
  launch_hub_lossy_w<W>(c, a, la);   // first: their chains are the round's longest
  if (a.nloc > 0)
    hipLaunchKernelGGL(k_expand_lossy<W>, dim3(grid_for(a.nloc, (int64_t)EWAVES * 64)), dim3(EBLOCK), 0, s, a, la);
  if (c->n_hub_items > 0) launch_apply_touched_w<W>(c, a);
  (void)hipEventRecord(c->ev[5], s);
}
#define V(W) template void launch_expand_lossy_w<W>(Ctx*, const ExpandArgs&); \
             template void launch_hub_lossy_w<W>(Ctx*, const ExpandArgs&, const LossArgs&);
V(1) V(2) V(4) V(8) V(16) V(32) V(64)
#undef V

// gp_reset: the request becomes the setting in force -- or the reset is refused
int loss_reset(Ctx* c) {
  if (c->loss_want) {
    if (const RecordOps* rec = records_arc_walker(c))
      return set_error(GP_EINVAL, std::string("link loss is on and so is ") + rec->call +
                                      ": the record walks arcs and would count closed ones as deliveries");
    if (c->local || c->nranks > 1)
      return set_error(GP_EINVAL, "link loss is not supported in a vertex-partitioned context");
  }
  c->loss_on = c->loss_want;
  c->loss_p = c->loss_p_want;
  c->loss_seed = c->loss_seed_want;
  return 0;
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_link_loss(gp_ctx* c, int32_t on, double p, uint64_t seed) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (!(p >= 0.0 && p <= 1.0)) return set_error(GP_EINVAL, "link loss: p must lie in [0, 1]");
  c->loss_want = on != 0;
  c->loss_p_want = on ? p : 0.0;
  c->loss_seed_want = on ? seed : 0;
  return 0;
}

int gp_link_loss_info(gp_ctx* c, int32_t* on, double* p, uint64_t* seed) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (on) *on = c->loss_on ? 1 : 0;
  if (p) *p = c->loss_p;
  if (seed) *seed = c->loss_seed;
  return 0;
}

}  // extern "C"
