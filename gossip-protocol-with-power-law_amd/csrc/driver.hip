// driver.hip -- host driver of one gossip round on MI355X (gfx950) and the
// run / output half of the C-ABI (include/gossip_capi.h; setup.hip has the
// configuration half).
//
// One gossip round r over all peers at once:
//   L_r  liveness: crash draws, heartbeat-miss counters, 3-miss detection,
//        dead-node reports, seed removal      (Peer.py:298-393, Seed.py:358-406;
//        liveness.hip)
//   I_r  injection of messages generated in round r     (Peer.py:395-400; k_inject)
//   E_r  expansion: next[v] = OR_{u in In(v)} frontier[u] & ~seen[v]; seen |= next
//        (forward-once with the Message-List slots; the send loop is
//        Peer.py:402-404, the receive side Peer.py:175-216).  round_plan.h
//        picks the direction and scan mode (launch_expand gathers its facts
//        and enqueues the plan); pull.hip / push.hip / hub.hip run it
//   X_r  (multi-GPU) counters' all-reduce, or the vertex partition's boundary
//        exchange over RCCL (partition.hip)
//
// Data layout in HBM: Message-List slots S[0], S[1]
// (u64[n_alloc][W], W words = 64*W messages per vertex), per-vertex fpop /
// seenpop / done_at / state, the in-CSR (row_ptr i64, col and gather-order
// gcol i32).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gp_device.h"
#include "xplan.h"

namespace gp {

static thread_local std::string g_err;
int set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int copy_sync(Ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (bytes == 0) return 0;
  GP_HIP(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
  GP_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

// partial layout [slot][NPART]: block k sums slot k with one coalesced sweep
__global__ void k_stats_reduce(u64* __restrict__ partial, u64* __restrict__ stats) {
  __shared__ u64 acc[BLOCK];
  const int k = blockIdx.x;
  u64 t = 0;
  for (int p = threadIdx.x; p < NPART; p += BLOCK) {
    t += partial[(size_t)k * NPART + p];
    partial[(size_t)k * NPART + p] = 0;
  }
  acc[threadIdx.x] = t;
  __syncthreads();
  for (int w = BLOCK / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) acc[threadIdx.x] += acc[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[k] += acc[0];
}

// frontier activity bitmap: bit v = (fpop[v] != 0), one word per 64 vertices.
// With dbits (single context, early-exit round without liveness) also the done
// bitmap: bit v = v holds every message of its component (seenpop == done_at,
// components with messages only), as of the end of the last round.
// With liveness (sated: the state bytes) the done bitmap is bit v = v is up and
// sated: it holds every alive message of its component, and
// the alive sets only shrink once no injection is left.
// With deg_live (receiver-list rounds, DESIGN.md §3.5: the pull's waves visit
// only the listed receivers) also every sender's accounting: sends =
// fpop * deg_live and the active count, into the partial stat slots.
__global__ __launch_bounds__(BLOCK) void k_mkbits(const uint32_t* __restrict__ fpop, u64* __restrict__ abits,
                                                  int64_t n, const uint32_t* __restrict__ seenpop,
                                                  const uint32_t* __restrict__ done_at, u64* __restrict__ dbits,
                                                  const uint8_t* __restrict__ sated,
                                                  const int32_t* __restrict__ deg_live, u64* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  u64 sends = 0, active = 0;
  for (int64_t v0 = (int64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63); v0 < n; v0 += stride) {
    const int64_t v = v0 + lane;
    const uint32_t fp = v < n ? fpop[v] : 0u;
    const u64 m = __ballot(fp != 0u);
    if (deg_live && fp) {
      sends += (u64)fp * (u64)(uint32_t)max(deg_live[v], 0);
      ++active;
    }
    if (lane == 0) abits[v0 >> 6] = m;
    if (dbits) {
      bool d = false;
      if (v < n) {
        if (sated) {   // (a complete up vertex holds every alive message too: pulls never mark it)
          const uint8_t sv = sated[v];
          const uint32_t t = done_at[v];
          d = !(sv & ST_DOWN) && ((sv & ST_SATED) || (t != 0u && seenpop[v] == t));
        } else {
          const uint32_t t = done_at[v];
          d = t != 0u && seenpop[v] == t;
        }
      }
      const u64 dm = __ballot(d);
      if (lane == 0) dbits[v0 >> 6] = dm;
    }
  }
  if (deg_live) {
    sends = wave_sum_u64(sends);
    active = wave_sum_u64(active);
    if (lane == 0) {
      const size_t p = blockIdx.x % NPART;
      if (sends) atomicAdd(&partial[(size_t)S_SENDS * NPART + p], sends);
      if (active) atomicAdd(&partial[(size_t)S_ACTIVE * NPART + p], active);
    }
  }
}

// summary level of the activity bitmap: bit j of sbits[k] = (abits[64k + j] != 0)
__global__ __launch_bounds__(BLOCK) void k_mksum(const u64* __restrict__ abits, u64* __restrict__ sbits,
                                                 int64_t nwords) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int64_t w = k * 64 + lane;
  const u64 m = __ballot(w < nwords && abits[w] != 0ull);
  if (lane == 0 && k * 64 < nwords) sbits[k] = m;
}

// Lost messages (origin down at the inject round, S_LOST) never enter any
// Message-List: drop them from the component targets of this run, so that the
// early-exit and done-skip tests of E_r still fire for the component's
// vertices.  One thread per (group, word) of this round's injection span; the
// state test is k_inject's own (no kernel between them changes state).
__global__ void k_lost_clear(const int32_t* __restrict__ origin, const u64* __restrict__ bits,
                             const uint32_t* __restrict__ cnt, const uint8_t* __restrict__ state,
                             const int32_t* __restrict__ midx, u64* __restrict__ cmask,
                             uint32_t* __restrict__ lostcnt, int64_t off, int64_t groups, int32_t words) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= groups * words) return;
  const int64_t gi = off + t / words;
  const int32_t w = (int32_t)(t % words);
  const int32_t o = origin[gi];
  if (!(state[o] & ST_DOWN)) return;
  const int32_t k = midx[o];
  atomicAnd(cmask + (size_t)k * words + w, ~bits[gi * words + w]);
  if (w == 0) atomicAdd(lostcnt + k, cnt[gi]);
}
__global__ void k_done_fix(const int32_t* __restrict__ midx, const uint32_t* __restrict__ lostcnt,
                           uint32_t* __restrict__ done_at, int64_t n) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
    const int32_t k = midx[v];
    if (k >= 0) {
      const uint32_t l = lostcnt[k];
      if (l) done_at[v] -= l;
    }
  }
}

// ---------------------------------------------------------------------------
// injection (I_r): one wave per (round, origin) group.  The origin's seen row
// is copied into slot r & 1 with the new messages (so that it is read as a
// sender this round, see ExpandArgs) and its frontier count grows.  Slots and
// popcounts are replicated on every rank, so every rank applies every group;
// the owner of the origin also updates seenpop, first-receipt and counters.
struct InjectArgs {
  const int32_t* __restrict__ origin;
  const u64* __restrict__ bits;
  const uint32_t* __restrict__ cnt;
  u64* slot[2];
  int32_t rslot;                       // r & 1
  uint8_t* __restrict__ sp;
  uint8_t* __restrict__ ws;
  uint32_t* __restrict__ fpop;
  u64* __restrict__ frx;               // exact frontier rows (track_msg_forwards, partitioned)
  int64_t frx_rows;                    // ... of vertices [0, frx_rows)
  u64* __restrict__ cmk;               // dense bitmap of slot r & 1 (record rounds, or null)
  u64* __restrict__ alive;             // [W] alive messages of round r (or null)
  uint32_t* __restrict__ seenpop;
  uint8_t* __restrict__ first;
  u64* __restrict__ digest;
  const uint8_t* __restrict__ state;
  uint8_t* __restrict__ lm;            // written line masks of this round's senders (or null)
  u64* __restrict__ partial;
  int64_t off, groups;
  int64_t vbegin, vend;                // owned local ids [vbegin, vend); beyond: ghosts / extras
  int32_t words;
  int32_t wbase;                       // global word index of local word 0 (message shards)
  int32_t r;
};

__global__ __launch_bounds__(BLOCK) void k_inject(InjectArgs a) {
  const int lane = threadIdx.x & 63;
  const int wib = uniform(threadIdx.x >> 6);
  WaveStats st;
  ws_zero(st);
  const int64_t k = (int64_t)blockIdx.x * WAVES + wib;
  if (k < a.groups && a.origin[a.off + k] >= 0) {   // (partitioned: every origin is local, never < 0)
    const int64_t gi = a.off + k;
    const int o = a.origin[gi];
    const bool owned = o >= a.vbegin && o < a.vend;
    // partitioned contexts hold every origin; a ghost's row in
    // slot r & 1 is its frontier, valid while its fpop is nonzero
    const bool ghost = o >= a.vend;
    if (a.state[o] & ST_DOWN) {
      if (owned) st.add(S_LOST, a.cnt[gi]);
    } else {
      const uint32_t cur = a.sp[o];
      const uint32_t fp = a.fpop[o];
      const bool has_frx = a.frx && o < a.frx_rows;
      u64 b = 0, s = 0, f = 0;
      if (lane < a.words) {
        b = a.bits[gi * a.words + lane];
        if (ghost ? fp != 0u : cur != SLOT_NONE) s = a.slot[ghost ? a.rslot : cur][(size_t)o * a.words + lane];
        if (has_frx && fp) f = a.frx[(size_t)o * a.words + lane];
      }
      __builtin_amdgcn_wave_barrier();   // the old rows are read before they are rewritten
      if (lane < a.words) {
        a.slot[a.rslot][(size_t)o * a.words + lane] = s | b;
        if (has_frx) a.frx[(size_t)o * a.words + lane] = f | b;
      }
      if (a.cmk && lane == 0) set_dense(a.cmk, o);   // a sender this round: its record (if any) is stale
      if (a.lm) {   // written line masks (64 words): the origin's new row, a superset of its old one
        const u64 nzb = __ballot(lane < a.words && (s | b) != 0ull);
        uint32_t nib = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) nib |= ((nzb >> (16 * t)) & 0xFFFFull) ? (1u << t) : 0u;
        if (lane == 0 && nib) atomicOr(reinterpret_cast<uint32_t*>(a.lm) + (o >> 3), nib << ((o & 7) * 4));
      }
      if (a.alive && b) atomicOr(a.alive + lane, b);   // injected messages are forwarded this round
      const uint32_t nb = wave_sum_u32((uint32_t)__popcll(b));
      if (lane == 0) {
        a.fpop[o] = fp + nb;
        a.sp[o] = (uint8_t)a.rslot;
        a.ws[o] |= (uint8_t)(1u << a.rslot);
      }
      if (owned) {
        const int64_t i = o - a.vbegin;
        if (lane < a.words && a.first && b)
          set_first_bytes(a.first + (size_t)i * a.words * 64, lane, b, (uint32_t)a.r);
        if (a.digest) {
          u64 t = b ? digest_term((uint32_t)a.r, (uint32_t)(a.wbase + lane) | DIGEST_INJECT, b) : 0ull;
          t = wave_xor_u64(t);
          if (lane == 0) a.digest[i] ^= t;
        }
        if (lane == 0) a.seenpop[i] += nb;
        st.add(S_INJECTED, a.cnt[gi]);
      }
    }
  }
  flush_stats(st, a.partial);
}

// ---------------------------------------------------------------------------
// per-message bit sums: cnt[m] += bit_m(row(v)), wsum[m] += weight(v)*bit_m(row(v))
// over rows [0, count).  Lane l holds word l % W of vertex slot l / W; each lane
// keeps 64 register counters per output.
struct BitsumArgs {
  const u64* __restrict__ rows;       // [count][W]
  const uint32_t* __restrict__ guard; // optional: row valid iff guard[i] != 0
  const int32_t* __restrict__ weight; // [count]
  u64* __restrict__ cnt;              // [W*64] or null
  u64* __restrict__ wsum;             // [W*64] or null
  int64_t count;
};

template <int W, bool CNT, bool SUM>
__global__ __launch_bounds__(BLOCK) void k_bitsum(BitsumArgs a) {
  static_assert(W <= 64, "W <= 64");
  constexpr int VPS = 64 / W;   // vertices per wave step
  __shared__ uint32_t lc[CNT ? W * 64 : 1];
  __shared__ uint32_t lsum[SUM ? W * 64 : 1];
  for (int t = threadIdx.x; t < W * 64; t += BLOCK) {
    if (CNT) lc[t] = 0;
    if (SUM) lsum[t] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int w = lane % W, q = lane / W;
  uint32_t c[64], s[64];
#pragma unroll
  for (int b = 0; b < 64; ++b) {
    c[b] = 0;
    s[b] = 0;
  }
  const int64_t step = (int64_t)gridDim.x * WAVES * VPS;
  for (int64_t i = ((int64_t)blockIdx.x * WAVES + wib) * VPS + q; i < a.count; i += step) {
    u64 x = 0;
    if (!a.guard || a.guard[i] != 0) {
      x = a.rows[i * W + w];
    }
    const uint32_t wt = SUM ? (uint32_t)max(a.weight[i], 0) : 0u;
#pragma unroll
    for (int b = 0; b < 64; ++b) {
      const uint32_t bit = (uint32_t)(x >> b) & 1u;
      if (CNT) c[b] += bit;
      if (SUM) s[b] += bit * wt;
    }
  }
#pragma unroll
  for (int b = 0; b < 64; ++b) {
#pragma unroll
    for (int st = W; st < 64; st <<= 1) {
      if (CNT) c[b] += __shfl_xor(c[b], st);
      if (SUM) s[b] += __shfl_xor(s[b], st);
    }
  }
  if (q == 0) {
#pragma unroll
    for (int b = 0; b < 64; ++b) {
      if (CNT && c[b]) atomicAdd(&lc[w * 64 + b], c[b]);
      if (SUM && s[b]) atomicAdd(&lsum[w * 64 + b], s[b]);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < W * 64; t += BLOCK) {
    if (CNT && lc[t]) atomicAdd(&a.cnt[t], (u64)lc[t]);
    if (SUM && lsum[t]) atomicAdd(&a.wsum[t], (u64)lsum[t]);
  }
}

// The activity bitmap of fpop[cur] (and its summary level) ahead of
// launch_expand, which builds both again from the same counts before anything
// else reads them: the per-round traffic pass probes them at its hook (load.hip)
int launch_activity_bits(Ctx* c, bool summary) {
  hipLaunchKernelGGL(k_mkbits, dim3(std::max(1, std::min(grid_for(c->n_alloc, BLOCK), c->cu_count * 8 * GS))),
                     dim3(BLOCK), 0, c->stream, c->d_fpop[c->cur], c->d_abits, c->n_alloc, c->d_seenpop,
                     c->d_done_at, (u64*)nullptr, (const uint8_t*)nullptr, (const int32_t*)nullptr, c->d_stats + 64);
  if (summary) {
    const int64_t nwords = (c->n_alloc + 63) / 64;
    hipLaunchKernelGGL(k_mksum, dim3(grid_for((nwords + 63) / 64, WAVES)), dim3(BLOCK), 0, c->stream, c->d_abits,
                       c->d_sbits, nwords);
  }
  GP_HIP(hipGetLastError());
  return 0;
}

// the pull's argument block for this round's plan
static void fill_expand(Ctx* c, ExpandArgs& a) {
  const RoundPlan& p = c->plan;
  a.alive = alive_now(c) ? c->d_alive + (size_t)c->cur * c->words : nullptr;
  a.alive_next = alive_on(c) ? c->d_alive + (size_t)(c->cur ^ 1) * c->words : nullptr;
  a.row_ptr = c->d_row_ptr;
  a.col = c->d_col;
  a.rows = c->d_slot[c->cur];
  a.slot[0] = c->d_slot[0];
  a.slot[1] = c->d_slot[1];
  a.wslot = c->cur ^ 1;
  a.sp = c->d_sp;
  a.ws = c->d_ws;
  a.fpop = c->d_fpop[c->cur];
  a.abits = c->d_abits;
  a.sbits = p.sum ? c->d_sbits : nullptr;
  a.dbits = p.dnb ? c->d_dbits : nullptr;
  a.amask = c->d_amask;
  a.prehi = p.split ? c->d_prehi : nullptr;
  a.split_push = 0;
  a.acc_row = p.split ? c->acc_row : 0;
  a.lm = p.lines ? (c->carry.lm_written ? c->d_lmw[c->cur] : c->d_lm) : nullptr;
  a.lm_next = p.lm_write ? c->d_lmw[c->cur ^ 1] : nullptr;
  a.cmk = p.cml_read ? c->d_cmk[c->cur] : nullptr;
  a.cml = p.cml_read ? c->d_cml[c->cur] : nullptr;
  a.cmk_next = p.cml_write ? c->d_cmk[c->cur ^ 1] : nullptr;
  a.cml_next = p.cml_write ? c->d_cml[c->cur ^ 1] : nullptr;
  // (the push reads the senders' exact rows where some other output keeps them;
  // rows kept for gp_track_fresh, gp_track_fresh_curve or gp_track_link_fresh alone leave its source, and
  // so every work counter of the run, the untracked run's)
  const bool frx_src = c->cfg.track_msg_forwards != 0 || c->local || c->rec[R_CURVE].want;
  a.frx = c->d_frx[0] && frx_src ? c->d_frx[c->cur] : nullptr;
  a.frx_next = c->d_frx[0] ? c->d_frx[c->cur ^ 1] : nullptr;
  a.frx_rows = c->frx_rows;
  a.done_at = c->d_done_at;
  a.gcol = c->d_gcol;
  a.midx = c->d_midx;
  a.cmask = c->d_cmask;
  a.unfiltered = p.unfiltered ? 1 : 0;
  a.near_done = p.near_done ? 1 : 0;
  a.sate = p.sate ? 1 : 0;
  a.ldone = p.line_done ? c->d_ldone : nullptr;
  a.early_exit = p.early_exit ? 1 : 0;
  a.dprobe = p.dprobe ? 1 : 0;
  a.alias = p.alias ? 1 : 0;
  a.ulist = p.ulist_read ? c->d_ulist[c->carry.ul_cur] : nullptr;
  a.ulist_n = p.ulist_read ? c->carry.ulist_n : 0;
  a.ulist_next = p.ulist_emit ? c->d_ulist[c->carry.ul_cur ^ 1] : nullptr;
  a.fpop_next = c->d_fpop[c->cur ^ 1];
  a.seenpop = c->d_seenpop;
  a.first = c->cfg.track_first ? c->d_first : nullptr;
  a.digest = c->cfg.track_digest ? c->d_digest : nullptr;
  a.state = c->d_state;
  a.deg_live = c->d_deg_live;
  a.partial = c->d_stats + 64;   // partial slots live behind the stats block
  a.hub_items = c->d_hub_items;
  a.hubs = c->d_hubs;
  a.hub_item_ptr = c->d_hub_item_ptr;
  a.hub_partial = c->d_hub_partial;
  a.hub_pnz = c->d_hub_pnz;
  a.hub_done = c->d_hub_done;
  if (++c->hub_epoch == 0) c->hub_epoch = 1;   // (wraps after 2^32 launches: 0 is the never-set value)
  a.hub_epoch = c->hub_epoch;
  a.border = c->d_border;
  a.vbegin = 0;   // kernels address local ids: owned vertices are [0, nloc)
  a.nloc = c->nloc();
  a.m_total = c->m;
  a.wbase = c->cfg.msg_word_base;
  a.rr = c->round + 1;
  a.hub_thr = c->cfg.hub_threshold;
  a.orp = c->directed ? c->d_out_row_ptr : c->d_row_ptr;
  a.ocol = c->directed ? c->d_out_col : c->d_col;
  a.acc = c->d_acc;
  a.tbits = c->d_tbits;
  a.touched = c->d_touched;
  a.active = c->d_active;
  a.big = c->d_big;
  a.stats = c->d_stats;
}

// what plan_round reads, from the context
static RoundFacts round_facts(const Ctx* c) {
  RoundFacts f;
  f.n = c->n;
  f.n_alloc = c->n_alloc;
  f.nloc = c->nloc();
  f.nnz = c->nnz;
  f.m = c->m;
  f.words = c->words;
  f.round = c->round;
  f.cfg = c->cfg;
  f.prev_new_bits = c->prev_new_bits;
  f.prev_receivers = c->prev_receivers;
  f.prev_next_arcs = c->prev_next_arcs;
  f.held_bits = c->held_bits;
  f.inj_arcs = (size_t)c->round < c->inj_arcs.size() ? (u64)c->inj_arcs[(size_t)c->round] : 0ull;
  f.inj_groups = c->inj_groups_at(c->round);
  f.last_inject_round = c->last_inject_round;
  f.local = c->local;
  f.liveness_active = c->liveness_active;
  f.alive_on = alive_on(c);
  f.alive_now = alive_now(c);
  f.have_cml = c->d_cml[0] != nullptr;
  f.have_lm = c->d_lm != nullptr;
  f.have_lmw = c->d_lmw[0] != nullptr;
  f.have_ldone = c->d_ldone != nullptr;
  f.have_ld_cand = c->n_ld_cand > 0;
  // accumulator rows as rows of this round's slot buffer: same allocation, same stride
  const int64_t row = c->words > 0 ? (int64_t)(c->d_acc - c->d_slot[c->cur]) / c->words : 0;   // (d_rows: S[0] | S[1] | acc)
  f.acc_row = row > 0 && row + c->nloc() <= (int64_t)INT32_MAX ? row : 0;
  f.ld_env = c->ld_env;
  f.lp_env = c->lp_env;
  f.can_park = !c->carry.park_failed;
  f.carry = c->carry;
  // (delayed links read frontier rows through the same plan, delayed.hip; so does a run with repair, repair.hip)
  f.lossy = c->loss_on || c->lag_on || c->repair_on;
  return f;
}

// E_r: gather the facts, plan the round (round_plan.h), enqueue what the plan says
static int launch_expand(Ctx* c) {
  RoundFacts f = round_facts(c);
  RoundPlan p = plan_round(f);
  // the buffers a plan may rely on are allocated at first use; without one
  // the round is planned again (at most once for each)
  if (p.need_park_slot && !c->d_slot[2] && dalloc(&c->d_slot[2], (size_t)c->n_alloc * c->words) != 0) {
    (void)hipGetLastError();
    c->carry.park_failed = f.carry.park_failed = true;   // (out of memory: stay filtered)
    f.can_park = false;
    p = plan_round(f);
  }
  if (p.need_ulist && !c->d_ulist[0] &&
      (dalloc(&c->d_ulist[0], (size_t)c->n_alloc) != 0 || dalloc(&c->d_ulist[1], (size_t)c->n_alloc) != 0)) {
    dfree(&c->d_ulist[0]);   // (out of memory: no lists)
    dfree(&c->d_ulist[1]);
    (void)hipGetLastError();
    f.can_list = false;
    p = plan_round(f);
  }
  // (a lossy round reads every sender's exact frontier row: a state reallocated
  // since the reset with the request withdrawn holds none)
  if (p.pull.kernel == PULL_LOSSY && (!c->d_frx[0] || c->frx_rows < c->n_alloc))
    return set_error(GP_ESTATE, "link loss is in force but the frontier rows are gone: gp_reset first");
  c->plan = p;
  c->acc_row = p.split ? (int32_t)f.acc_row : 0;
  if (alive_on(c))   // F_{r+1} is built by this round's receivers
    GP_HIP(hipMemsetAsync(c->d_alive + (size_t)(c->cur ^ 1) * c->words, 0, (size_t)c->words * 8, c->stream));
  // a push's receivers and a list round's non-receivers start from fpop_next = 0;
  // so does a lossy round, whose hubs are committed by the push's receiver side
  if ((p.mode_push && c->nloc() > 0) || p.ulist_read || (p.pull.kernel == PULL_LOSSY && c->nloc() > 0))
    GP_HIP(hipMemsetAsync(c->d_fpop[c->cur ^ 1], 0, (size_t)c->nloc() * 4, c->stream));
  hipLaunchKernelGGL(k_mkbits, dim3(std::max(1, std::min(grid_for(c->n_alloc, BLOCK), c->cu_count * 8 * GS))),
                     dim3(BLOCK), 0, c->stream, c->d_fpop[c->cur], c->d_abits, c->n_alloc,
                     c->d_seenpop, c->d_done_at, p.dnb ? c->d_dbits : nullptr,
                     p.dnb && c->liveness_active ? (const uint8_t*)c->d_state : nullptr,
                     p.ulist_read ? (const int32_t*)c->d_deg_live : nullptr, c->d_stats + 64);
  if (c->carry.alias_active) {   // (after k_mkbits: a push round's senders are the activity bitmap's bits)
    if (p.mode_push) GP_TRY(unalias(c, true));
    else if (!p.dprobe) GP_TRY(unalias(c, false));   // (a pull that could gather a done sender's row)
  }
  if (p.sum) {
    const int64_t nwords = (c->n_alloc + 63) / 64;
    hipLaunchKernelGGL(k_mksum, dim3(grid_for((nwords + 63) / 64, WAVES)), dim3(BLOCK), 0, c->stream,
                       c->d_abits, c->d_sbits, nwords);
  }
  if (p.split) GP_TRY(build_prehi(c, c->cfg.split_deg));
  ExpandArgs a{};
  fill_expand(c, a);
  return launch_round_kernels(c, a);
}

template <int W>
static void launch_bitsum_w(Ctx* c, BitsumArgs a, bool cnt, bool sum) {
  const int grid = std::max(1, std::min(grid_for(a.count, (int64_t)WAVES * (64 / W)), c->cu_count * 2 * GS));
  if (cnt && sum)
    hipLaunchKernelGGL((k_bitsum<W, true, true>), dim3(grid), dim3(BLOCK), 0, c->stream, a);
  else if (cnt)
    hipLaunchKernelGGL((k_bitsum<W, true, false>), dim3(grid), dim3(BLOCK), 0, c->stream, a);
  else if (sum)
    hipLaunchKernelGGL((k_bitsum<W, false, true>), dim3(grid), dim3(BLOCK), 0, c->stream, a);
}

static int launch_bitsum(Ctx* c, BitsumArgs a, bool cnt, bool sum) {
  if (a.count <= 0) return 0;
  GP_TRY(with_words(c->words, [&](auto w) { launch_bitsum_w<w()>(c, a, cnt, sum); }));
  GP_HIP(hipGetLastError());
  return 0;
}

// the per-bit count of guarded rows, for curve.hip's yardstick (GP_CURVE_YARDSTICK)
int bitsum_count_rows(Ctx* c, const u64* rows, const uint32_t* guard, int64_t count, u64* cnt) {
  BitsumArgs b{};
  b.rows = rows;
  b.guard = guard;
  b.cnt = cnt;
  b.count = count;
  return launch_bitsum(c, b, true, false);
}

// phases L_r, I_r, E_r of one round on one context (no host sync)
static int round_launch(Ctx* c) {
  if (!state_ready(c) || c->words <= 0) return set_error(GP_ESTATE, "gp_set_messages + gp_reset first");
  if (c->round > 253) return set_error(GP_ESTATE, "round limit (254) reached");
  GP_TRY(lag_check_round(c));   // (delayed links: before anything of the round is enqueued)
  GP_TRY(repair_check_round(c));
  GP_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  u64* stats = c->d_stats;
  u64* partial = c->d_stats + 64;
  const int r = c->round;
  lag_rotate(c);   // (delayed links: d_frx[cur] / d_frx[cur ^ 1] are the ring's slots of rounds r and r + 1)
  GP_HIP(hipMemsetAsync(stats, 0, 64 * sizeof(u64), s));
  GP_HIP(hipEventRecord(c->ev[0], s));
  if (c->liveness_active) {
    c->msg_forwards_valid = c->msg_forwards_valid && (c->cfg.track_msg_forwards != 0);
    GP_TRY(launch_liveness(c));
  }

  auto it = c->inject.find(r);
  if (it != c->inject.end() && it->second.cnt > 0) {
    GP_TRY(unalias(c, false));   // (k_inject reads the origins' rows; no vertex completes before the last injection)
    InjectArgs ia{};
    ia.origin = c->d_inj_origin;
    ia.bits = c->d_inj_bits;
    ia.cnt = c->d_inj_cnt;
    ia.slot[0] = c->d_slot[0];
    ia.slot[1] = c->d_slot[1];
    ia.rslot = c->cur;
    ia.sp = c->d_sp;
    ia.ws = c->d_ws;
    ia.fpop = c->d_fpop[c->cur];
    ia.frx = c->d_frx[0] ? c->d_frx[c->cur] : nullptr;
    ia.frx_rows = c->frx_rows;
    ia.cmk = c->d_cmk[0] ? c->d_cmk[c->cur] : nullptr;
    ia.alive = alive_on(c) ? c->d_alive + (size_t)c->cur * c->words : nullptr;
    ia.seenpop = c->d_seenpop;
    ia.first = c->cfg.track_first ? c->d_first : nullptr;
    ia.digest = c->cfg.track_digest ? c->d_digest : nullptr;
    ia.state = c->d_state;
    ia.lm = c->carry.lm_written ? c->d_lmw[c->cur] : nullptr;
    ia.partial = partial;
    ia.off = it->second.off;
    ia.groups = it->second.cnt;
    ia.vbegin = 0;
    ia.vend = c->nloc();
    ia.words = c->words;
    ia.wbase = c->cfg.msg_word_base;
    ia.r = r;
    hipLaunchKernelGGL(k_inject, dim3(grid_for(ia.groups, WAVES)), dim3(BLOCK), 0, s, ia);
    GP_HIP(hipGetLastError());
    if (c->liveness_active && c->cmask_rows > 0) {   // origins may be down: drop lost messages
      GP_HIP(hipMemsetAsync(c->d_lostcnt, 0, (size_t)c->cmask_rows * 4, s));
      hipLaunchKernelGGL(k_lost_clear, dim3(grid_for(ia.groups * c->words, 256)), dim3(256), 0, s,
                         c->d_inj_origin, c->d_inj_bits, c->d_inj_cnt, c->d_state, c->d_midx, c->d_cmask,
                         c->d_lostcnt, ia.off, ia.groups, c->words);
      hipLaunchKernelGGL(k_done_fix, dim3(std::min(grid_for(c->n_alloc, 256), c->cu_count * 8)), dim3(256), 0, s,
                         c->d_midx, c->d_lostcnt,
                         c->d_done_at, c->n_alloc);
      GP_HIP(hipGetLastError());
      c->done_dirty = true;
    }
  }

  if (c->cfg.track_msg_forwards) {   // sends of round r per message (owned senders)
    BitsumArgs b{};
    b.rows = c->d_frx[c->cur];   // exact frontier rows of the owned senders
    b.guard = c->d_fpop[c->cur];
    b.weight = c->d_deg_live;
    b.cnt = nullptr;
    b.wsum = c->d_msg_fwd;
    b.count = c->nloc();
    GP_TRY(launch_bitsum(c, b, false, true));
  }
  GP_TRY(load_before_expand(c));   // (nothing is launched unless gp_track_load is on and the run counts per round)

  GP_HIP(hipEventRecord(c->ev[1], s));
  GP_TRY(launch_expand(c));
  hipLaunchKernelGGL(k_stats_reduce, dim3(NST), dim3(BLOCK), 0, s, partial, stats);
  GP_HIP(hipGetLastError());
  GP_HIP(hipEventRecord(c->ev[2], s));
  return records_count_round(c);   // (nothing is launched unless a record is on; all after expand_ms ends: round_ms carries them)
}

// X_r over RCCL.  One rank: the counters' all-reduce is the whole exchange.
// Vertex partition: the boundary exchange of partition.hip (this round's new
// bits of the owned vertices other ranks hold as ghosts, removal flags, alive
// sets) and the counters' all-reduce, so that every rank takes the same
// decisions next round.
static int round_exchange_rccl(Ctx* c) {
  if (!c->comm) {
    if (c->local) return set_error(GP_ESTATE, "a partitioned context exchanges over RCCL (gp_comm_init) "
                                              "or in gp_round_group");
    return 0;
  }
  if (c->local) return exchange_rccl(c);
  // the report cursor (slot S_REPORT_CURSOR) stays rank-local
  GP_RCCL(ncclAllReduce(c->d_stats, c->d_stats, S_REPORT_CURSOR, ncclUint64, ncclSum, c->comm, c->stream));
  return 0;
}

static int round_collect(Ctx* c, gp_round_stats* out) {
  hipStream_t s = c->stream;
  const int r = c->round;
  GP_HIP(hipEventRecord(c->ev[3], s));
  GP_HIP(hipMemcpyAsync(c->h_stats, c->d_stats, 64 * sizeof(u64), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  const u64* h = c->h_stats;
  if (h[S_XERR])   // (every rank of an RCCL partition sees the all-reduced count)
    return set_error(GP_ERCCL, "boundary exchange: " + std::to_string(h[S_XERR]) +
                                   " received entries do not match the exchange plan (round " + std::to_string(r) + ")");
  gp_round_stats own;
  {
    gp_round_stats* out = &own;   // (kept for the run: a shard job's combine reads it)
    std::memset(out, 0, sizeof(*out));
    out->round = r;
    out->injected = h[S_INJECTED];
    out->lost = h[S_LOST];
    out->new_bits = h[S_NEW_BITS];
    out->receivers = h[S_RECEIVERS];
    out->sends = h[S_SENDS];
    out->active = h[S_ACTIVE];
    out->crashed = h[S_CRASHED];
    out->reports = h[S_REPORTS];
    out->removals = h[S_REMOVALS];
    out->dup_reports = h[S_DUP];
    out->arcs_scanned = h[S_ARCS];
    out->rows_gathered = h[S_GATHERED];
    out->seen_rows_read = h[S_SEEN_READ];
    out->rows_written = h[S_WRITTEN];
    out->vertices_visited = h[S_VISITED];
    out->atomics = h[S_ATOMICS];
    out->next_arcs = h[S_NEXT_ARCS];
    out->row_bytes = h[S_ROW_BYTES];
    out->mode = c->plan.pull.kernel == PULL_LOSSY ? 2 : c->plan.mode_push ? 1 : 0;
    out->scan = c->plan.scan();
    out->kernel_ms = 0.0;
    if (!c->plan.mode_push && c->nloc() > 0) {
      float kms = 0.f;
      (void)hipEventElapsedTime(&kms, c->ev[4], c->ev[5]);
      out->kernel_ms = kms;
    }
    out->overflow = (int64_t)h[S_REPORT_CURSOR] > c->report_cap ? 1 : 0;
    out->xchg_rows = h[S_XROWS];
    out->xchg_bytes = h[S_XBYTES];
    out->done_nb = h[S_DNB];
    out->lm_rows = h[S_LM_ROWS];
    out->aliased = h[S_ALIASED];
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev[1], c->ev[2]);
    out->expand_ms = ms;
    (void)hipEventElapsedTime(&ms, c->ev[2], c->ev[3]);
    out->exchange_ms = ms;
    (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[3]);
    out->round_ms = ms;
  }
  if (out) *out = own;
  c->run_stats.push_back(own);
  c->last_reports = (int64_t)h[S_REPORT_CURSOR];
  c->prev_next_arcs = h[S_NEXT_ARCS];
  c->prev_new_bits = h[S_NEW_BITS];
  c->prev_receivers = h[S_RECEIVERS];
  c->held_bits += h[S_INJECTED] + h[S_NEW_BITS];
  c->lag_hist = (c->lag_hist << 1) | (h[S_ACTIVE] ? 1u : 0u);   // (delayed links: lag_in_flight)
  repair_collect(c, h, h[S_NEW_BITS], r);
  {   // what this round hands to the next one
    const RoundPlan& p = c->plan;
    RoundCarry& k = c->carry;
    k.cml_written = p.cml_write;
    k.lm_written = p.lm_write;
    if (h[S_ALIASED]) k.alias_active = true;
    k.ulist_valid = p.ulist_emit;   // (a round that appends no list ends the last one)
    if (p.ulist_emit) {
      k.ulist_n = (int64_t)h[S_ULIST];
      k.ul_cur ^= 1;
    }
    if (p.sate && k.sate_since < 0) k.sate_since = r;
  }
  c->cur ^= 1;
  c->round = r + 1;
  return 0;
}

// dst[i] -= src[i], i < n
__global__ void k_sub_u64(u64* __restrict__ dst, const u64* __restrict__ src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] -= src[i];
}

// Forwards taken from the Message-Lists (no liveness, no track_msg_forwards)
// count every holder of a message as a sender of it.  That is the run's sends
// once it is quiescent; a run that stopped while its last round still made new
// bits -- at the round limit, or because the caller stopped -- holds receivers
// that have not sent yet.  pending: such receivers exist; unknown: and the
// context keeps no frontier rows to take their share off again
bool fwd_pending(const Ctx* c) {
  return !c->liveness_active && !c->cfg.track_msg_forwards && c->round > 0 && c->prev_new_bits > 0;
}
bool forwards_unknown(const Ctx* c) {
  return fwd_pending(c) && !(c->d_frx[0] && c->frx_rows >= c->nloc());
}

}  // namespace gp

using namespace gp;

// ===========================================================================
// C-ABI
extern "C" {

int gp_abi_version(void) { return GP_ABI_VERSION; }
const char* gp_last_error(void) { return g_err.c_str(); }

int gp_device_count(int* n_out) {
  if (!n_out) return set_error(GP_EINVAL, "null n_out");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *n_out = n;
  return 0;
}

}  // extern "C"

extern "C" {

int gp_round(gp_ctx* c, gp_round_stats* out) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (c->local && !c->comm)
    return set_error(GP_ESTATE, "a partitioned context exchanges over RCCL (gp_comm_init) or in gp_round_group");
  // (message-shard job, shard.hip: the history check and its growth come
  // first, so that no error of theirs can leave a round half applied)
  GP_TRY(lag_check_round(c));   // (delayed links are refused in a shard job: before its history moves)
  GP_TRY(repair_check_round(c));   // (and so is repair)
  if (c->jnranks > 0) GP_TRY(shard_prepare_round(c));
  GP_TRY(round_launch(c));
  GP_TRY(round_exchange_rccl(c));
  if (c->jnranks > 0) GP_TRY(shard_record_round(c));
  return round_collect(c, out);
}

int gp_round_group(gp_ctx** ctxs, int32_t nctx, gp_round_stats* out) {
  if (!ctxs || nctx < 1) return set_error(GP_EINVAL, "bad context list");
  for (int32_t k = 0; k < nctx; ++k) {
    Ctx* c = ctxs[k];
    if (!c) return set_error(GP_EINVAL, "null ctx in group");
    if (c->comm) return set_error(GP_EINVAL, "group rounds exchange without RCCL");
    if (c->nranks != nctx || c->rank != k) return set_error(GP_EINVAL, "ctxs[k] must own partition k of nctx");
    if (c->round != ctxs[0]->round || c->n != ctxs[0]->n || c->words != ctxs[0]->words)
      return set_error(GP_EINVAL, "contexts out of step");
  }
  for (int32_t k = 0; k < nctx; ++k) GP_TRY(round_launch(ctxs[k]));
  // X_r: the boundary exchange through device-to-device copies -- the same
  // pack / unpack as over RCCL (partition.hip)
  if (nctx > 1) {
    std::vector<Ctx*> cs(ctxs, ctxs + nctx);
    GP_TRY(exchange_group(cs.data(), nctx));
  }
  gp_round_stats sum;
  std::vector<u64> own_held((size_t)nctx, 0);
  std::memset(&sum, 0, sizeof(sum));
  for (int32_t k = 0; k < nctx; ++k) {
    gp_round_stats st;
    GP_TRY(round_collect(ctxs[k], &st));
    own_held[(size_t)k] = st.injected + st.new_bits;
    sum.round = st.round;
    sum.overflow |= st.overflow;
    sum.injected += st.injected; sum.lost += st.lost; sum.new_bits += st.new_bits;
    sum.receivers += st.receivers; sum.sends += st.sends; sum.active += st.active;
    sum.crashed += st.crashed; sum.reports += st.reports; sum.removals += st.removals;
    sum.dup_reports += st.dup_reports; sum.arcs_scanned += st.arcs_scanned;
    sum.rows_gathered += st.rows_gathered; sum.seen_rows_read += st.seen_rows_read;
    sum.rows_written += st.rows_written; sum.vertices_visited += st.vertices_visited;
    sum.atomics += st.atomics; sum.next_arcs += st.next_arcs; sum.mode = st.mode;
    sum.row_bytes += st.row_bytes; sum.scan = st.scan;
    sum.xchg_rows += st.xchg_rows; sum.xchg_bytes += st.xchg_bytes; sum.done_nb += st.done_nb;
    sum.lm_rows += st.lm_rows;
    sum.expand_ms = std::max(sum.expand_ms, st.expand_ms);
    sum.exchange_ms = std::max(sum.exchange_ms, st.exchange_ms);
    sum.round_ms = std::max(sum.round_ms, st.round_ms);
    sum.kernel_ms = std::max(sum.kernel_ms, st.kernel_ms);
  }
  for (int32_t k = 0; k < nctx; ++k) {   // every context takes the same decisions next round
    ctxs[k]->prev_next_arcs = sum.next_arcs;
    ctxs[k]->prev_new_bits = sum.new_bits;
    ctxs[k]->prev_receivers = sum.receivers;
    // round_collect added the context's own share; every context holds the sum
    ctxs[k]->held_bits += sum.injected + sum.new_bits - own_held[(size_t)k];
  }
  if (out) *out = sum;
  return 0;
}

int gp_run(gp_ctx* c, int32_t max_rounds, gp_round_stats* per_round, int32_t* rounds_out) {
  if (!c || max_rounds < 1) return set_error(GP_EINVAL, "bad argument");
  int32_t done = 0;
  for (int32_t k = 0; k < max_rounds; ++k) {
    gp_round_stats st;
    GP_TRY(gp_round(c, &st));
    if (per_round) per_round[k] = st;
    ++done;
    // (delayed links: and nothing in flight -- no sender in the last dmax - 1 rounds)
    // (repair: and the last `period` rounds were all silent -- at period 1 the same rule)
    if (st.new_bits == 0 && st.round >= c->last_inject_round && lag_in_flight(c) == 0 &&
        (!c->repair_on || c->repair_quiet >= c->repair_period))
      break;
  }
  if (rounds_out) *rounds_out = done;
  return 0;
}

// finalize through the component targets (bitcount.hip); GP_FINALIZE_ROWS=1 in
// the environment counts every row instead (the tests compare the two)
static bool finalize_by_rows() {
  const char* e = getenv("GP_FINALIZE_ROWS");
  return e && e[0] == '1';
}
int gp_finalize_messages(gp_ctx* c) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (!state_ready(c)) return set_error(GP_ESTATE, "no run state");
  GP_HIP(hipSetDevice(c->device));
  const size_t M = (size_t)c->words * 64;
  hipStream_t s = c->stream;
  u64* cov = c->d_msg_cov;
  u64* fwd_local = c->d_msg_fwd;
  u64* gcov = c->d_msg_cov + 2 * M;
  u64* gfwd = c->d_msg_cov + 3 * M;
  const bool fwd_from_seen = !c->liveness_active && !c->cfg.track_msg_forwards;
  // seen row i = slot[sp[i]][i], owned local ids [0, nloc): bit-sliced counts
  // (bitcount.hip), forwards weighted by the static degree (= deg_live without liveness)
  if (c->done_at_valid && !finalize_by_rows()) GP_TRY(finalize_by_components(c, fwd_from_seen, cov, fwd_local));
  else GP_TRY(bitcount_messages(c, fwd_from_seen, cov, fwd_local));
  // the last round's receivers have not sent their new bits: the next round's
  // frontier x deg_live (what its track_msg_forwards pass would add) comes off
  // again (gfwd is free until the copy below; GP_FORWARDS refuses the read
  // where no frontier rows exist: forwards_unknown)
  if (fwd_pending(c) && !forwards_unknown(c) && c->nloc() > 0) {
    GP_HIP(hipMemsetAsync(gfwd, 0, M * 8, s));
    BitsumArgs b{};
    b.rows = c->d_frx[c->cur];
    b.guard = c->d_fpop[c->cur];
    b.weight = c->d_deg_live;
    b.wsum = gfwd;
    b.count = c->nloc();
    GP_TRY(launch_bitsum(c, b, false, true));
    hipLaunchKernelGGL(k_sub_u64, dim3(grid_for((int64_t)M, 256)), dim3(256), 0, s, fwd_local, gfwd, (int64_t)M);
    GP_HIP(hipGetLastError());
  }
  if (c->comm) {
    GP_RCCL(ncclGroupStart());
    GP_RCCL(ncclAllReduce(cov, gcov, M, ncclUint64, ncclSum, c->comm, s));
    GP_RCCL(ncclAllReduce(fwd_local, gfwd, M, ncclUint64, ncclSum, c->comm, s));
    GP_RCCL(ncclGroupEnd());
  } else {
    GP_HIP(hipMemcpyAsync(gcov, cov, M * 8, hipMemcpyDeviceToDevice, s));
    GP_HIP(hipMemcpyAsync(gfwd, fwd_local, M * 8, hipMemcpyDeviceToDevice, s));
  }
  GP_HIP(hipStreamSynchronize(s));
  c->fin_round = c->round;
  return 0;
}

int gp_read(gp_ctx* c, int32_t what, void* host, int64_t bytes) {
  if (!c || !host) return set_error(GP_EINVAL, "null argument");
  GP_HIP(hipSetDevice(c->device));
  GP_HIP(hipStreamSynchronize(c->stream));
  // partitioned contexts read their owned slice of the per-vertex arrays
  // (local ids [0, nloc) = global [vbegin, vend)) and their local CSR
  const int64_t W = c->words, nl = c->nloc(), M = c->m, n = c->local ? c->nloc() : c->n;
  auto need = [&](int64_t b) -> int {
    if (bytes != b) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(b));
    return 0;
  };
  const bool run = state_ready(c);
  switch (what) {
    case GP_SEEN:
      if (!run) return set_error(GP_ESTATE, "no run state");
      GP_TRY(need(nl * W * 8));
      GP_TRY(unalias(c, false));   // (aliased Message-Lists become rows of S[cur])
      if (bytes) {   // owned rows of every slot, picked per vertex by its slot byte
        // blocks of rows: host scratch stays at 2 blocks whatever n (a 2^26 x
        // 4096 read would otherwise hold two more 32 GiB copies)
        const int64_t blk = std::max<int64_t>(1, (int64_t(64) << 20) / (W * 8));
        std::vector<uint64_t> s1((size_t)(std::min(nl, blk) * W)), s2(c->d_slot[2] ? s1.size() : 0);
        std::vector<uint8_t> sp((size_t)nl);
        GP_TRY(copy_sync(c, sp.data(), c->d_sp, (size_t)nl, hipMemcpyDeviceToHost));
        uint64_t* h = static_cast<uint64_t*>(host);
        for (int64_t v0 = 0; v0 < nl; v0 += blk) {
          const int64_t k = std::min(blk, nl - v0);
          const size_t kb = (size_t)(k * W * 8);
          GP_TRY(copy_sync(c, h + v0 * W, c->d_slot[0] + v0 * W, kb, hipMemcpyDeviceToHost));
          GP_TRY(copy_sync(c, s1.data(), c->d_slot[1] + v0 * W, kb, hipMemcpyDeviceToHost));
          if (c->d_slot[2]) GP_TRY(copy_sync(c, s2.data(), c->d_slot[2] + v0 * W, kb, hipMemcpyDeviceToHost));
          for (int64_t v = v0; v < v0 + k; ++v) {
            const uint8_t p = sp[(size_t)v];
            const int64_t o = (v - v0) * W;
            if (p == SLOT_NONE) std::memset(h + v * W, 0, (size_t)W * 8);
            else if (p == 1) std::memcpy(h + v * W, s1.data() + o, (size_t)W * 8);
            else if (p == SLOT_PARKED && !s2.empty()) std::memcpy(h + v * W, s2.data() + o, (size_t)W * 8);
          }
        }
      }
      return 0;
    case GP_FIRST:
      if (!run) return set_error(GP_ESTATE, "no run state");
      if (!c->d_first || !c->cfg.track_first) return set_error(GP_ENOTRACK, "track_first is off");
      GP_TRY(need(nl * M));
      if (bytes)
        GP_HIP(hipMemcpy2D(host, (size_t)M, c->d_first, (size_t)W * 64, (size_t)M, (size_t)nl,
                           hipMemcpyDeviceToHost));
      return 0;
    case GP_DIGEST:
      if (!run) return set_error(GP_ESTATE, "no run state");
      if (!c->cfg.track_digest) return set_error(GP_ENOTRACK, "track_digest is off");
      GP_TRY(need(nl * 8));
      if (bytes) GP_TRY(copy_sync(c, host, c->d_digest, (size_t)bytes, hipMemcpyDeviceToHost));
      return 0;
    case GP_COVERAGE:
    case GP_FORWARDS: {
      if (!run) return set_error(GP_ESTATE, "no run state");
      if (what == GP_FORWARDS && !c->msg_forwards_valid && c->liveness_active)
        return set_error(GP_ENOTRACK, "churn run without track_msg_forwards");
      if (what == GP_FORWARDS && forwards_unknown(c))
        return set_error(GP_ENOTRACK, "the run stopped before quiescence and keeps no frontier rows: its last "
                                      "receivers' sends are not known (track_msg_forwards)");
      GP_TRY(need(M * 8));
      const size_t MM = (size_t)W * 64;
      const u64* src = c->d_msg_cov + (what == GP_COVERAGE ? 2 * MM : 3 * MM);
      GP_TRY(copy_sync(c, host, src, (size_t)bytes, hipMemcpyDeviceToHost));
      return 0;
    }
    case GP_STATE:
    case GP_MISS:
      if (!run) return set_error(GP_ESTATE, "no run state");
      GP_TRY(need(n));
      GP_TRY(copy_sync(c, host, what == GP_STATE ? c->d_state : c->d_miss, (size_t)n, hipMemcpyDeviceToHost));
      if (what == GP_STATE)   // (the removal flag and the sated mark are engine bookkeeping)
        for (int64_t v = 0; v < n; ++v) static_cast<uint8_t*>(host)[v] &= (uint8_t)~(ST_RMNEW | ST_SATED);
      return 0;
    case GP_DEG_LIVE:
      if (!run) return set_error(GP_ESTATE, "no run state");
      GP_TRY(need(n * 4));
      GP_TRY(copy_sync(c, host, c->d_deg_live, (size_t)bytes, hipMemcpyDeviceToHost));
      return 0;
    case GP_ROW_PTR:   // partitioned: the local CSR over all local slots
      if (c->n <= 0) return set_error(GP_ESTATE, "no graph");
      GP_TRY(need((c->n_alloc + 1) * 8));
      GP_TRY(copy_sync(c, host, c->d_row_ptr, (size_t)bytes, hipMemcpyDeviceToHost));
      return 0;
    case GP_COL:
      if (c->n <= 0) return set_error(GP_ESTATE, "no graph");
      GP_TRY(need(c->nnz_l * 4));
      if (bytes) GP_TRY(copy_sync(c, host, c->d_col, (size_t)bytes, hipMemcpyDeviceToHost));
      return 0;
    case GP_L2G:   // global id of every local slot
      if (c->n <= 0) return set_error(GP_ESTATE, "no graph");
      GP_TRY(need(c->n_alloc * 4));
      if (c->local) {
        GP_TRY(copy_sync(c, host, c->d_l2g, (size_t)bytes, hipMemcpyDeviceToHost));
      } else {
        for (int64_t v = 0; v < c->n; ++v) static_cast<int32_t*>(host)[v] = (int32_t)v;
      }
      return 0;
    case GP_JOB_DIGEST:
    case GP_JOB_COVERAGE:
    case GP_JOB_FORWARDS: {   // the job record of gp_shard_combine (shard.hip)
      if (!c->j_ready) return set_error(GP_ESTATE, "gp_shard_combine first");
      if (what == GP_JOB_DIGEST) {
        if (!c->j_dig_valid) return set_error(GP_ENOTRACK, "track_digest is off");
        GP_TRY(need(c->n * 8));
        GP_TRY(copy_sync(c, host, c->d_jdig, (size_t)bytes, hipMemcpyDeviceToHost));
        return 0;
      }
      if (what == GP_JOB_FORWARDS && !c->j_fwd_valid)
        return set_error(GP_ENOTRACK, "churn run without track_msg_forwards (on some rank)");
      GP_TRY(need((int64_t)c->jm * 8));
      GP_TRY(copy_sync(c, host, c->d_jcf + (what == GP_JOB_COVERAGE ? 0 : (size_t)c->jm), (size_t)bytes,
                       hipMemcpyDeviceToHost));
      return 0;
    }
    case GP_FPOP:
      if (!run) return set_error(GP_ESTATE, "no run state");
      GP_TRY(need(n * 4));
      GP_TRY(copy_sync(c, host, c->d_fpop[c->cur], (size_t)bytes, hipMemcpyDeviceToHost));
      return 0;
    case GP_FRONTIER: {
      if (!run) return set_error(GP_ESTATE, "no run state");
      // exact frontier rows exist only with track_msg_forwards: the pull reads
      // whole Message-Lists
      if (!c->cfg.track_msg_forwards) return set_error(GP_ENOTRACK, "frontier rows are kept only with track_msg_forwards");
      GP_TRY(need(n * W * 8));
      std::vector<uint32_t> fp((size_t)n);
      GP_TRY(copy_sync(c, fp.data(), c->d_fpop[c->cur], (size_t)n * 4, hipMemcpyDeviceToHost));
      GP_TRY(copy_sync(c, host, c->d_frx[c->cur], (size_t)bytes, hipMemcpyDeviceToHost));
      uint64_t* h = static_cast<uint64_t*>(host);
      for (int64_t v = 0; v < n; ++v)
        if (!fp[v]) std::memset(h + v * W, 0, (size_t)W * 8);
      return 0;
    }
    case GP_LOAD_SENT:
    case GP_LOAD_RECV:   // per-peer traffic record (load.hip)
      return load_read(c, what, host, bytes);
    case GP_FRESH_SENT:
    case GP_FRESH_RECV:   // per-peer fresh deliveries (fresh.hip)
      return fresh_read(c, what, host, bytes);
    case GP_LINK_FRESH:   // per-link fresh deliveries (link.hip)
      return link_read(c, host, bytes);
    case GP_DELAY_SUM:
    case GP_DELAY_MAX:   // per-peer receipt delays (delay.hip)
      return delay_read(c, what, host, bytes);
    case GP_DELAY_DIST:   // per-peer delay distributions (delay_dist.hip)
      return delay_dist_read(c, host, bytes);
    case GP_SOLE_SENT:
    case GP_SOLE_RECV:   // delivery multiplicity (mult.hip)
      return mult_read(c, what, host, bytes);
    case GP_WATCH_FIRST:
    case GP_WATCH_ARRIVAL:
    case GP_WATCH_PTR:   // watched peers (watch.hip)
      return watch_read(c, what, host, bytes);
    case GP_ARC_DELAY:   // delayed links (delayed.hip)
      return lag_read(c, host, bytes);
    case GP_SEENPOP:
      if (!run) return set_error(GP_ESTATE, "no run state");
      GP_TRY(need(nl * 4));
      if (bytes) GP_TRY(copy_sync(c, host, c->d_seenpop, (size_t)bytes, hipMemcpyDeviceToHost));
      return 0;
    default:
      return set_error(GP_EINVAL, "unknown gp_what");
  }
}

int gp_reports(gp_ctx* c, gp_report* buf, int64_t cap, int64_t* n_out) {
  if (!c || !n_out || (cap > 0 && !buf)) return set_error(GP_EINVAL, "null argument");
  GP_HIP(hipSetDevice(c->device));
  const int64_t total = c->last_reports;
  *n_out = total;
  const int64_t k = std::min(std::min(total, cap), c->report_cap);
  if (k > 0) GP_TRY(copy_sync(c, buf, c->d_reports, (size_t)k * sizeof(gp_report), hipMemcpyDeviceToHost));
  return 0;
}

int gp_synchronize(gp_ctx* c) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  GP_HIP(hipSetDevice(c->device));
  GP_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int gp_info(gp_ctx* c, int64_t* n, int64_t* nnz, int32_t* m, int32_t* words) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (n) *n = c->n;
  if (nnz) *nnz = c->nnz;
  if (m) *m = c->m;
  if (words) *words = c->words;
  return 0;
}

int gp_local_info(gp_ctx* c, int64_t* nloc, int64_t* nghost, int64_t* nextra, int64_t* nnz_local,
                  int64_t* n_boundary) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (nloc) *nloc = c->nloc();
  if (nghost) *nghost = c->nghost;
  if (nextra) *nextra = c->nextra;
  if (nnz_local) *nnz_local = c->nnz_l;
  if (n_boundary) *n_boundary = c->n_bnd;
  return 0;
}

}  // extern "C"
