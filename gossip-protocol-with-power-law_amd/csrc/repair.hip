// repair.hip -- anti-entropy repair: in every round r
// with (r + 1) % period == 0 each up receiver v pulls the whole Message-List of
// one in-neighbour p_r(v), drawn from the receiver and the round
// (repair_draw.h), over the arc p -> v if the round's loss draw leaves it open:
//
//   offer_r[v] = seen_r[p_r(v)] & ~seen_r[v]
//   next_r[v]  = (the lossy expansion's OR of open senders' frontier rows | offer_r[v]) & ~seen[v]
//
// A repaired bit is a first receipt like any other: it enters frontier_{r+1}[v]
// and v forwards it once.  The other rounds of such a run are lossy.hip's,
// unchanged (with loss off their draw opens every arc).
//
// The hazard that shapes the kernels: the lossy expansion reads only senders'
// frontier rows, which no commit of the same round writes.  A partner need not
// be a sender; its Message-List may live in the slot buffer this round's commits
// write, S[(r + 1) & 1], and would be overwritten in place (and sp[p] flipped)
// under a reader.  So every Message-List row of another vertex is read by
// k_repair_offer, the round's first kernel, before anything commits:
//
// k_repair_offer: a wave per 64 consecutive receivers.  Lane phase, coalesced:
// state, in-list bounds, the partner draw, the partner's id and state, the loss
// draw of the arc.  Then the receivers with an open exchange go RPI per wave
// step, a row slot each: the 16-B pieces of slot[sp[p]][p] and slot[sp[v]][v],
// offer = P & ~V, written into v's accumulator row (all-zero between uses)
// where nonzero.  A receiver with an offer is marked: in tbits above
// hub_threshold, else in a bitmap of its own (rbits; the wave owns its word and
// writes it whole, so no stale mark survives a round).  exchanges and lines
// are wave-reduced into two device counters round_collect reads.  A receiver
// that holds every message of its component skips the row loads (its offer is
// empty); the exchange still counts.
// k_expand_repair: k_expand_lossy's lane phase, scan and commit -- a marked
// receiver is never dropped by the prefilter or for want of a sending
// in-neighbour; its gather ends with its accumulator row ORed in and zeroed;
// every output comes from finish_row / commit_vertices.  The narrow-row groups
// of lossy.hip are not built here: a receiver takes a wave step at every W.
// Hubs need no kernel: k_hub_lossy ORs into the same accumulator row and the
// push's tail (launch_apply_touched_w) commits and zeroes it.
//
// Also gp_repair / gp_repair_info / gp_read_repair, what gp_reset does with the
// request, the stopping rule's `quiet` and the per-round record (host side).
#include <algorithm>
#include <cstring>

#include "gp_device.h"
#include "link_loss.h"
#include "lossy_scan.h"
#include "repair_draw.h"

namespace gp {

struct RepairArgs {
  uint64_t key;             // repair_round_key(seed, r)
  LossDraw d;               // the round's loss draw (loss off: every arc open)
  u64* __restrict__ rbits;  // [n_alloc/64] receivers below hub_threshold with an offer
};

__device__ __forceinline__ const u64* slot_of_byte(const ExpandArgs& a, uint32_t s) { return s == 0u ? a.slot[0] : a.slot[1]; }

template <int W>
__global__ __launch_bounds__(BLOCK) void k_repair_offer(ExpandArgs a, RepairArgs ra) {
  constexpr int LPR = Geo<W>::LPR;
  constexpr int RPI = Geo<W>::RPI;
  constexpr u64 STEP = RPI == 64 ? ~0ull : (1ull << (RPI & 63)) - 1ull;
  __shared__ u64 s_mark[WAVES][2];   // [0]: receivers below hub_threshold, [1]: above
  const int lane = threadIdx.x & 63;
  const int wib = uniform(threadIdx.x >> 6);
  const int g = lane / LPR, lw = lane % LPR;
  const int64_t base = ((int64_t)blockIdx.x * WAVES + wib) * 64;
  if (base >= a.nloc) return;   // (wave-uniform; the kernel has no block barrier)
  const int64_t li = base + lane;
  int32_t p = 0;
  uint32_t sv = SLOT_NONE, sp = SLOT_NONE;
  bool x = false, rows = false, hub = false;
  if (li < a.nloc) {
    const int v = (int)(a.vbegin + li);
    const int64_t b = a.row_ptr[v], e = a.row_ptr[v + 1];
    if (!(a.state[v] & ST_DOWN) && e > b && !ra.d.closed) {
      p = a.col[b + (int64_t)repair_partner_index(ra.key, (uint64_t)v, (uint64_t)(e - b))];
      x = !(a.state[p] & ST_DOWN) && arc_open(ra.d.key, (uint32_t)(a.vbegin + p), (uint32_t)v, ra.d.thresh);
      if (x && p != v && a.seenpop[li] < a.done_at[v]) {   // (a self-loop offers nothing; nor does anyone to a done receiver)
        sp = a.sp[p];
        sv = a.sp[v];
        rows = sp <= 1u && (sv <= 1u || sv == SLOT_NONE);   // (a run with repair holds rows in S[0], S[1] only)
      }
      hub = e - b > a.hub_thr;
    }
  }
  if (lane < 2) s_mark[wib][lane] = 0ull;
  wave_sync_lds();
  const u64 nx = (u64)__popcll(__ballot(x));
  const u64 mrows = __ballot(rows);
  const u64 mhub = __ballot(hub);
  u64 nl = 0;
#pragma unroll 1
  for (int r0 = 0; r0 < 64; r0 += RPI) {
    if (!((mrows >> r0) & STEP)) continue;   // wave-uniform
    const int k = r0 + g;
    const bool on = (mrows >> k) & 1ull;
    const int32_t pk = __shfl(p, k);
    const uint32_t spk = (uint32_t)__shfl((int)sp, k), svk = (uint32_t)__shfl((int)sv, k);
    const int64_t vk = a.vbegin + base + k;
    u64x2 P = {0, 0}, V = {0, 0};
    if (on) {
      P = load_piece<W>(slot_of_byte(a, spk), pk, lw);
      if (svk != SLOT_NONE) V = load_piece<W>(slot_of_byte(a, svk), vk, lw);
    }
    const u64x2 offer = P & ~V;
    const bool nz = (offer.x | offer.y) != 0ull;
    if (nz) store_piece<W>(a.acc, vk, lw, offer);   // (the rest of the row is zero already)
    nl += (u64)(__popcll(offer.x) + __popcll(offer.y));
    if (group_or<LPR>(nz) && lw == 0) atomicOr(&s_mark[wib][(mhub >> k) & 1ull], 1ull << k);
  }
  wave_sync_lds();
  nl = wave_sum_u64(nl);
  if (lane == 0) {
    const int64_t w = (a.vbegin + base) >> 6;
    ra.rbits[w] = s_mark[wib][0];
    if (s_mark[wib][1]) atomicOr(&a.tbits[w], s_mark[wib][1]);
    if (nx) atomicAdd(&a.stats[S_REPAIR_X], nx);
    if (nl) atomicAdd(&a.stats[S_REPAIR_LINES], nl);
  }
}

template <int W>
__global__ EXPAND_BOUNDS void k_expand_repair(ExpandArgs a, LossArgs la, const u64* __restrict__ rbits) {
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
    const u64 marks = rbits[(a.vbegin + base) >> 6];   // receivers of this wave whose accumulator row holds an offer
    const bool marked = valid && ((marks >> lane) & 1ull);
    bool need = false, scan = false, act = false;
    u64 sends = 0;
    uint32_t slot_of = SLOT_NONE;
    uint32_t pre_arcs = 0;   // arcs the lane phase probed for the receivers it dropped
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
      scan = !(a.state[v] & ST_DOWN) && a.seenpop[li] < a.done_at[v] && !hub && e > b && !la.d.closed;
      if (scan && e - b <= PRE_MAX_DEG) {   // no sending in-neighbour: nothing to scan
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
          scan = false;
          pre_arcs = (uint32_t)deg;
        }
      }
      need = scan || marked;   // (a marked receiver commits its offer whatever the gossip brings)
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
    const u64 mscan = __ballot(scan), mmark = __ballot(marked);
    while (m) {
      const int k = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int64_t i = base + k;
      const int v = uniform((int)(a.vbegin + i));
      const uint32_t sv_slot = (uint32_t)__builtin_amdgcn_readlane((int)slot_of, k);
      u64x2 acc = {0, 0};
      if ((mscan >> k) & 1ull) lossy_scan<W>(a, la, v, L.rp[k], L.rp[k + 1], L, lane, g, lw, acc, st);
      reduce_slots<W>(acc);
      if (((mmark >> k) & 1ull) && g == 0) {   // the offer, and the row back to all-zero
        acc |= load_piece<W>(a.acc, v, lw);
        store_piece<W>(a.acc, v, lw, u64x2{0, 0});
      }
      finish_row<W, true, false>(a, v, i, acc, lane, g, lw, st, L, false, sv_slot, k);
    }
    alive_flush<W>(a, L.alive, lane);
    commit_vertices(a, L, li, need, st);   // (fpop_next of every other vertex was zeroed before the launch)
  }
  flush_stats<EWAVES>(st, a.partial);
}

template <int W>
void launch_expand_repair_w(Ctx* c, const ExpandArgs& a) {
  LossArgs la;
  la.frx = c->d_frx[c->cur];
  la.d = loss_draw(c->loss_on ? c->loss_p : 0.0, c->loss_on ? c->loss_seed : 0, (uint32_t)c->round);
  RepairArgs ra;
  ra.key = repair_round_key(c->repair_seed, (uint32_t)c->round);
  ra.d = la.d;
  ra.rbits = c->d_rbits;
  hipStream_t s = c->stream;
  (void)hipEventRecord(c->ev[4], s);
  if (a.nloc > 0)   // first: before any commit of the round can overwrite a partner's row
    hipLaunchKernelGGL(k_repair_offer<W>, dim3(grid_for(a.nloc, (int64_t)WAVES * 64)), dim3(BLOCK), 0, s, a, ra);
  launch_hub_lossy_w<W>(c, a, la);
  if (a.nloc > 0)
    hipLaunchKernelGGL(k_expand_repair<W>, dim3(grid_for(a.nloc, (int64_t)EWAVES * 64)), dim3(EBLOCK), 0, s, a, la,
                       (const u64*)c->d_rbits);
  if (c->n_hub_items > 0) launch_apply_touched_w<W>(c, a);
  (void)hipEventRecord(c->ev[5], s);
}
#define V(W) template void launch_expand_repair_w<W>(Ctx*, const ExpandArgs&);
V(1) V(2) V(4) V(8) V(16) V(32) V(64)
#undef V

bool repair_now(const Ctx* c) { return c->repair_on && repair_round(c->round, c->repair_period); }

// gp_reset, before anything changes: the request can become the setting in force
int repair_check_reset(const Ctx* c) {
  if (!c->repair_want) return 0;
  if (c->lag_want)
    return set_error(GP_EINVAL, "repair is on and so is gp_link_delay: a partner's Message-List over a delayed link is "
                                "not modelled");
  if (const RecordOps* rec = records_arc_walker(c))
    return set_error(GP_EINVAL, std::string("repair is on and so is ") + rec->call +
                                    ": the record walks arcs and would miss the receipts an exchange carried");
  if (c->local || c->nranks > 1)
    return set_error(GP_EINVAL, "repair is not supported in a vertex-partitioned context");
  if (c->jnranks > 0)
    return set_error(GP_EINVAL, "repair is not supported in a message-shard job (gp_shard_*): the job record takes a "
                                "round's receivers to have heard that round's senders");
  return 0;
}

// with the run state in place
int repair_reset(Ctx* c) {
  c->repair_on = false;   // (until the bitmap stands)
  c->repair_period = 1;
  c->repair_seed = 0;
  c->repair_quiet = 0;
  c->repair_rec_valid = true;
  c->repair_rec.clear();
  if (!c->repair_want) {
    repair_free(c);
    return 0;
  }
  const int64_t nw = (c->n_alloc + 63) / 64;
  if (c->rbits_words != nw || !c->d_rbits) {
    c->rbits_words = 0;
    GP_TRY(dalloc(&c->d_rbits, (size_t)std::max<int64_t>(nw, 1)));
    c->rbits_words = nw;
  }
  GP_HIP(hipMemsetAsync(c->d_rbits, 0, (size_t)std::max<int64_t>(nw, 1) * 8, c->stream));
  c->repair_on = true;
  c->repair_period = c->repair_period_want;
  c->repair_seed = c->repair_seed_want;
  return 0;
}

void repair_free(Ctx* c) {
  dfree(&c->d_rbits);
  c->rbits_words = 0;
}

// a transport joined after the reset: caught at the top of the round, as lag_check_round catches it
int repair_check_round(const Ctx* c) {
  if (!c->repair_on) return 0;
  if (c->jnranks > 0)
    return set_error(GP_ESTATE, "repair is in force and a message-shard job (gp_shard_*) was joined since the reset: "
                                "not supported together, gp_reset refuses it by name");
  if (!c->d_rbits || c->rbits_words < (c->n_alloc + 63) / 64)
    return set_error(GP_ESTATE, "repair is in force but its mark bitmap is gone: gp_reset first");
  return 0;
}

void repair_collect(Ctx* c, const u64* h, u64 new_bits, int32_t r) {
  if (!c->repair_on) return;
  c->repair_quiet = (new_bits == 0 && r >= c->last_inject_round) ? c->repair_quiet + 1 : 0;
  if (c->repair_rec_valid) {
    c->repair_rec.push_back(h[S_REPAIR_X]);
    c->repair_rec.push_back(h[S_REPAIR_LINES]);
  }
}

void repair_restored(Ctx* c, int32_t round) {
  c->repair_quiet = 0;
  c->repair_rec.clear();
  c->repair_rec_valid = round == 0;
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_repair(gp_ctx* c, int32_t on, int32_t period, uint64_t seed) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (period < 1 || period > REPAIR_PERIOD_MAX) return set_error(GP_EINVAL, "repair: period must lie in [1, 64]");
  c->repair_want = on != 0;
  c->repair_period_want = on ? period : 1;
  c->repair_seed_want = on ? seed : 0;
  return 0;
}

int gp_repair_info(gp_ctx* c, int32_t* on, int32_t* period, uint64_t* seed, int32_t* quiet) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (on) *on = c->repair_on ? 1 : 0;
  if (period) *period = c->repair_period;
  if (seed) *seed = c->repair_seed;
  if (quiet) *quiet = c->repair_on ? c->repair_quiet : 0;
  return 0;
}

int gp_read_repair(gp_ctx* c, uint64_t* out, int32_t cap, int32_t* rounds) {
  if (!c || !rounds || cap < 0 || (cap > 0 && !out)) return set_error(GP_EINVAL, "bad argument");
  if (!c->repair_on) return set_error(GP_ENOTRACK, "repair is off for the current run (gp_repair, then gp_reset)");
  if (!c->repair_rec_valid)
    return set_error(GP_ESTATE, "the run was restored past round 0: the repair record is not kept (gp_reset)");
  const int32_t R = (int32_t)(c->repair_rec.size() / 2);
  *rounds = R;
  const int32_t k = std::min(R, cap);
  if (k > 0) std::memcpy(out, c->repair_rec.data(), (size_t)k * 2 * sizeof(uint64_t));
  return 0;
}

}  // extern "C"
