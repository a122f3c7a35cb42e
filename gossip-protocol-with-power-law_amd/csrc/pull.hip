// pull.hip -- the pull expansion E_r of DESIGN.md §3.2-3.4: next[v] = OR over
// v's in-neighbours u of frontier[u] & ~seen[v] (the send loop of Peer.py:402-404,
// the receive side of Peer.py:175-216), with forward-once and Message-List
// dedup.  k_expand (a wave per 64 receivers, one receiver at a time, W >= 32;
// its receivers several per wave step: pull_groups.h) and the launch of a
// whole expansion round as round_plan.h planned it (k_expand's variants,
// k_expand_flat of pull_flat.hip, k_expand_rec of pull_rec.hip) with the
// helper passes of pull_aux.hip.
#include "pull_groups.h"
#include "round_plan.h"

namespace gp {

// main pull kernel: a wave owns 64 consecutive vertices.  The per-vertex
// checks (sender accounting, down / done / hub / no in-arcs) run lane-parallel
// with coalesced loads; the wave then scans, one receiver at a time, only the
// vertices that can still receive something.  Kept lean on registers (7 waves
// per SIMD): the dense rounds are bound by the rows in flight.
// (occupancy is the compiler's choice: an 8-waves hint spilled and was slower
// for the alive variants, and for W < 64, r04_ab_waves.txt)
template <int W, int MODE>
__global__ EXPAND_BOUNDS __attribute__((amdgpu_waves_per_eu(1))) void k_expand(ExpandArgs a) {
  constexpr int LPR = Geo<W>::LPR;
  __shared__ LDS_OF(MODE) s_w[EWAVES];
  const int lane = threadIdx.x & 63;
  const int wib = uniform(threadIdx.x >> 6);
  const int g = lane / LPR, lw = lane % LPR;
  auto& L = s_w[wib];
  constexpr bool ALIVE = (MODE & SCAN_ALIVE) != 0;
  constexpr bool DPROBE = (MODE & SCAN_DPROBE) != 0;
  constexpr bool LIST = (MODE & SCAN_LIST) != 0;
  constexpr bool QUADS = (MODE & SCAN_QUADS) != 0;
  // the serial loop's row gather packs the live lines (gather_rows_pack): a
  // variant of its own, launched only in gated rounds (round_plan.h's choice)
  constexpr bool PACK = (MODE & SCAN_PACK) != 0;
  static_assert(!PACK || (W == 64 && !ALIVE && !DPROBE && !LIST && !QUADS), "the packed gather: the plain W = 64 pull");
  constexpr int SCAN = MODE & ~(SCAN_ALIVE | SCAN_DPROBE | SCAN_LIST | SCAN_QUADS | SCAN_PACK);
  // the variants that can append this round's survivors to the next list
  // (profiles/r06_ab_lists_c5.txt)
  constexpr bool EMIT = W == 64 && (SCAN == SCAN_FILTERED || SCAN == SCAN_UNFILTERED);
  // the variants done-neighbour rounds without liveness launch: their complete
  // receivers may alias (a.alias) and their scans probe the done bitmap
  // (a.dprobe); the other variants compile neither
  constexpr bool ALIASABLE = W == 64 && !ALIVE && (SCAN == SCAN_FILTERED || SCAN == SCAN_UNFILTERED);
  // the variants whose receivers of in-degree <= 32 go two at a time
  // (gather_pairs): the unfiltered near-done pulls without liveness
  // (SCAN_QUADS; C4 round 4 6.93-7.02 -> 6.61-6.65 ms, 80 VGPRs; in the alive
  // one C5 rounds 4-5 gained nothing: their receivers scan to the end,
  // profiles/r06_ab_gather_pairs.txt)
  constexpr bool GPAIRS = W == 64 && QUADS && !ALIVE && SCAN == SCAN_UNFILTERED && !LIST;
  // ... and at W = 32 / 16 four / eight at a time (gather_groups; not at W = 8:
  // 16 receivers per step took 96 VGPRs and were slower, profiles/r06_ab_w8.txt)
  constexpr bool GGROUPS = (W == 32 || W == 16) && QUADS && !ALIVE && SCAN == SCAN_UNFILTERED && !LIST;
  // the variants that take the complete lines of a top in-neighbour from
  // their receivers' targets (a.ldone): the unfiltered
  // early-exit pulls without liveness or list (C4 rounds 3 and 4, and the
  // done-probe variant behind them, which keeps its 70 VGPRs); the other
  // variants compile none of it
  constexpr bool LDONE = W == 64 && !ALIVE && !LIST && SCAN == SCAN_UNFILTERED;
  // the serial loop's and the commit's cross-lane reductions in registers
  // (lane_ops.h; GP_LANE_OPS).  Every variant: the line-mask one (C4 round 2),
  // which reduces once per receiver, ran 0.1 ms slower with them and the run
  // as fast with it left on LDS shuffles as without (profiles/r21_ab_lane_ops.txt)
  constexpr bool LO = true;
  WaveStats st;
  ws_zero<EWAVES>(st);
  // the wave's block of 64 vertices: the blocks with a long non-hub in-list are
  // launched first (a.border, block_order.h: one wave-uniform load), so their
  // chains do not start when the rest of the grid has drained; list rounds keep
  // the list's order.  Nothing depends on the order: every receiver is
  // committed by exactly one wave, the counters are sums, the next list is
  // appended in atomic order
  int64_t blk = (int64_t)blockIdx.x * EWAVES + wib;
  if constexpr (!LIST) {
    if (a.border && blk * 64 < a.nloc) blk = uniform(a.border[blk]);
  }
  const int64_t base = blk * 64;
  if (base < (LIST ? a.ulist_n : a.nloc)) {
    const int64_t li = base + lane;
    // lane's vertex (local index): base + lane, or the list's entry (list
    // rounds: every sender's accounting is k_mkbits', every non-receiver's
    // fpop_next was zeroed before the launch)
    const bool valid = LIST ? li < a.ulist_n : li < a.nloc;
    const int64_t vi = LIST ? (valid ? (int64_t)a.ulist[li] : 0) : li;
    bool need = false, act = false, dnb = false;
    // degree-split rounds: receivers the push half touched (bit k = vertex
    // base + k; one context: local = global ids).  A touched receiver's
    // accumulator row is one more entry of its staged list: row a.acc_row + v
    // of this round's slot buffer is row v of a.acc (same stride, host-checked
    // offset), so the gathers need no second base pointer.  k_acc_clear zeroes
    // the rows and the bitmap after the pull (no store here to the rows the
    // gathers read)
    u64 tw = 0;
    if constexpr ((MODE & 3) == SCAN_PRE) {
      if (a.prehi) tw = a.tbits[base >> 6];
    }
    u64 sends = 0;
    uint32_t slot_of = SLOT_NONE;
    uint32_t pre_arcs = 0;   // SCAN_PRE: arcs the lane phase scanned
    bool small = false;      // GPAIRS: in-degree <= 32
    if (valid) {
      const int v = (int)(a.vbegin + vi);
      if constexpr (!LIST) {
        const uint32_t fp = a.fpop[v];
        act = fp != 0u;
        if (act) sends = (u64)fp * (u64)(uint32_t)max(a.deg_live[v], 0);
      }
      const int64_t b = a.row_ptr[v], e = a.row_ptr[v + 1];
      L.rp[lane] = b;
      if constexpr (LIST) {
        L.re[lane] = e;
        L.vid[lane] = v;
      } else {
        if (lane == 63 || li + 1 == a.nloc) L.rp[lane + 1] = e;
      }
      const bool hub = e - b > a.hub_thr;   // split over waves by the hub kernels
      need = !(a.state[v] & (ST_DOWN | ST_SATED)) && a.seenpop[vi] < a.done_at[v] && !hub && e > b;
      if constexpr (GPAIRS) small = e - b <= 32;
      if constexpr (GGROUPS) small = e - b <= Geo<W>::LPR;
      if constexpr ((MODE & 3) == SCAN_MASKED) need = need && mask_any(a.amask, b, e);
      if constexpr ((MODE & 3) == SCAN_PRE) {
        // sparse filtered rounds: every lane probes the in-list of its own
        // vertex (up to PRE_MAX_DEG arcs, all loads in flight together), so the
        // wave's serial loop skips vertices with no active in-neighbour and
        // starts the others at their rows
        uint32_t np = 0xFFu;
        const bool tch = (tw >> lane) & 1ull;
        const int64_t se = a.prehi ? b + a.prehi[v] : e;   // end of the arcs this vertex scans
        L.len[lane] = (uint32_t)(se - b);
        if (need && se - b <= PRE_MAX_DEG) {
          const int deg = (int)(se - b);
          uint32_t cnt = 0;
#pragma unroll
          for (int h = 0; h < PRE_MAX_DEG / PRE_IDS; ++h) {
            if (h * PRE_IDS < deg) {
              int32_t c[PRE_IDS];
              u64 w[PRE_IDS];
#pragma unroll
              for (int q = 0; q < PRE_IDS; ++q) c[q] = h * PRE_IDS + q < deg ? a.gcol[b + h * PRE_IDS + q] : -1;
              if (a.sbits) {   // summary level first: L2-resident, most probes end there
                u64 sw[PRE_IDS];
#pragma unroll
                for (int q = 0; q < PRE_IDS; ++q) sw[q] = c[q] >= 0 ? a.sbits[c[q] >> 12] : 0ull;
#pragma unroll
                for (int q = 0; q < PRE_IDS; ++q)
                  w[q] = ((sw[q] >> ((c[q] >> 6) & 63)) & 1ull) ? a.abits[c[q] >> 6] : 0ull;
              } else
#pragma unroll
              for (int q = 0; q < PRE_IDS; ++q) w[q] = c[q] >= 0 ? a.abits[c[q] >> 6] : 0ull;
#pragma unroll
              for (int q = 0; q < PRE_IDS; ++q) {
                if (c[q] >= 0 && ((w[q] >> (c[q] & 63)) & 1ull)) {
                  if (cnt < (uint32_t)PRE_IDS) L.pre[lane][cnt] = c[q];
                  ++cnt;
                }
              }
            }
          }
          if (cnt + (tch ? 1u : 0u) <= (uint32_t)PRE_IDS) {
            if (tch) L.pre[lane][cnt++] = a.acc_row + v;   // the accumulator row: one more entry
            np = cnt;
            pre_arcs = (uint32_t)deg;
          }
          if (cnt == 0) need = false;
        }
        L.np[lane] = (uint8_t)np;
      }
      if (!need && !hub) a.fpop_next[v] = 0;
      slot_of = a.sp[v];
      if (a.early_exit && need) L.mi[lane] = a.midx[v];
      // (with alive sets -- liveness -- only the SCAN_ALIVE variants: the done
      // target is then cmask & F_r & ~seen, which the others cannot form)
      if (a.dbits && need && (ALIVE || !a.alive)) dnb = done_nb(a, b, e);
      if constexpr (LDONE) {
        // complete lines of the first two in-neighbours, carried above the
        // slot byte (a done in-neighbour already gives all four)
        if (a.ldone && need && (!QUADS || small)) {   // (quads variant: gather_pairs' receivers only)
          const uint32_t ld = line_done_nb(a, b, e);
          if (!dnb) slot_of |= ld << LD_SHIFT;
        }
      }
    }
    if constexpr ((MODE & 3) == SCAN_PRE) st.add(S_ARCS, (u64)wsum_u32<LO>(pre_arcs));
    st.add(S_SENDS, wsum_u64<LO>(sends));
    st.add(S_ACTIVE, (u64)__popcll(__ballot(act)));
    st.add(S_VISITED, (u64)__popcll(__ballot(need)));
    L.tot[lane] = 0u;
    L.dig[lane] = 0ull;
    alive_zero<W>(a, L.alive, lane);
    wave_sync_lds();
    const bool ee = a.early_exit != 0;
    u64 m = __ballot(need);
    const u64 mdn = __ballot(dnb);   // receivers with a done in-neighbour (a.dbits rounds)
    st.add(S_DNB, (u64)__popcll(mdn));
    if constexpr ((MODE & 3) == SCAN_PRE && GP_WAVE_PRE_MAX > PRE_MAX_DEG) {
      // receivers with PRE_MAX_DEG < deg <= GP_WAVE_PRE_MAX: the wave probes
      // their in-lists WAVE_PRE_N at a time (one coalesced pass each, all
      // loads in flight together) instead of one receiver's chain after the
      // other in the serial loop; those with at most PRE_IDS active
      // neighbours join the prefiltered receivers, those with none drop out
      u64 mw = __ballot(need && L.np[lane] == 0xFFu && L.len[lane] <= GP_WAVE_PRE_MAX);
      u64 zero = 0;   // no active in-neighbour: nothing to scan (commit writes fpop_next = 0)
      uint32_t arcs = 0;
      while (mw) {
        int kq[WAVE_PRE_N];
        int32_t c[WAVE_PRE_N];
#pragma unroll
        for (int q = 0; q < WAVE_PRE_N; ++q) {
          kq[q] = -1;
          if (mw) {
            kq[q] = __ffsll((long long)mw) - 1;
            mw &= mw - 1;
          }
          c[q] = -1;
          if (kq[q] >= 0) {
            const int64_t b = L.rp[kq[q]];
            if (lane < (int)L.len[kq[q]]) c[q] = a.gcol[b + lane];
          }
        }
        u64 w[WAVE_PRE_N];
        if (a.sbits) {
          u64 sw[WAVE_PRE_N];
#pragma unroll
          for (int q = 0; q < WAVE_PRE_N; ++q) sw[q] = c[q] >= 0 ? a.sbits[c[q] >> 12] : 0ull;
#pragma unroll
          for (int q = 0; q < WAVE_PRE_N; ++q)
            w[q] = ((sw[q] >> ((c[q] >> 6) & 63)) & 1ull) ? a.abits[c[q] >> 6] : 0ull;
        } else
#pragma unroll
        for (int q = 0; q < WAVE_PRE_N; ++q) w[q] = c[q] >= 0 ? a.abits[c[q] >> 6] : 0ull;
#pragma unroll
        for (int q = 0; q < WAVE_PRE_N; ++q) {
          if (kq[q] < 0) continue;
          const bool act = c[q] >= 0 && ((w[q] >> (c[q] & 63)) & 1ull);
          const u64 am = __ballot(act);
          const int tq = (int)((tw >> kq[q]) & 1ull);   // degree-split: + the accumulator row
          const int cnt = __popcll(am) + tq;
          if (cnt <= PRE_IDS) {   // (more: the serial loop scans it, and counts its arcs)
            if (act) L.pre[kq[q]][lane_rank(am)] = c[q];
            if (lane == 0) {
              if (tq) L.pre[kq[q]][cnt - 1] = a.acc_row + (int32_t)(base + kq[q]);
              L.np[kq[q]] = (uint8_t)cnt;
            }
            if (cnt == 0) zero |= 1ull << kq[q];
            arcs += L.len[kq[q]];
          }
        }
      }
      st.add(S_ARCS, (u64)arcs);
      wave_sync_lds();
      m &= ~zero;
    }
    if constexpr ((MODE & SCAN_CML) != 0) L.racc[lane] = 0ull;   // record rounds: first receiver's accumulator
    if constexpr (W == 64 && (MODE & 3) == SCAN_PRE) {
      if (!ee) {   // prefiltered receivers two at a time, the rest below
        const u64 mp = m & __ballot(need && L.np[lane] != 0xFFu);
        // (four at a time without records, profiles/r06_ab_pre_quads.txt)
        if constexpr (!LDS_OF(MODE)::kCml) pre_quads(a, L, mp, base, slot_of, st);
        else pre_pairs<W>(a, L, mp, base, slot_of, st);
        m &= ~mp;
      }
    } else if constexpr ((W == 32 || W == 16 || W == 8) && (MODE & 3) == SCAN_PRE) {
      if (!ee) {   // four (eight) at a time (pre_groups)
        const u64 mp = m & __ballot(need && L.np[lane] != 0xFFu);
        pre_groups<W>(a, L, mp, base, slot_of, st);
        m &= ~mp;
      }
    }
    u64 sat = 0;   // receivers of this wave found sated (alive rounds)
    if constexpr (W == 64) {
      if (mdn) {   // done in-neighbours: two receivers at a time, the rest below
        const u64 md = m & mdn;
        // (quads in the alive variants too: C5 round 5 11.95 -> 11.78 ms, but
        // round 3, the same kernel, 73.8 -> 78.7 ms, profiles/r06_ab_quads_c5.txt)
        // (in the alive SCAN_QUADS variant, which only the half-held rounds
        // launch, they pay: C5 round 5 12.2 -> 11.8 ms, r06_ab_gather_pairs.txt)
        if constexpr (DPROBE || QUADS) dnb_quads<ALIASABLE, ALIVE>(a, L, md, base, slot_of, st);
        else dnb_pairs<W, ALIVE, ALIASABLE>(a, L, md, base, slot_of, st);
        if constexpr (ALIVE) {   // they now hold every alive message of their component: sated too
          if (a.sate) sat |= md;
        }
        m &= ~md;
      }
    } else if constexpr (W == 32 || W == 16 || W == 8) {
      if (mdn) {   // done in-neighbours, four (eight) at a time (dnb_groups)
        const u64 md = m & mdn;
        dnb_groups<W, ALIVE>(a, L, md, base, slot_of, st);
        if constexpr (ALIVE) {
          if (a.sate) sat |= md;
        }
        m &= ~md;
      }
    }
    if constexpr (GPAIRS) {   // low in-degree receivers two at a time, the rest below
      const u64 mg = m & __ballot(small);
      if (mg) {
        sat |= gather_pairs<ALIVE, ALIASABLE>(a, L, mg, base, slot_of, st);
        m &= ~mg;
      }
    }
    if constexpr (GGROUPS) {   // W = 32: low in-degree receivers four at a time
      const u64 mg = m & __ballot(small);
      if (mg) {
        gather_groups<W>(a, L, mg, base, slot_of, st);
        m &= ~mg;
      }
    }
    while (m) {
      const int k = __ffsll((long long)m) - 1;
      m &= m - 1;
      int64_t i = base + k;
      int v = uniform((int)(a.vbegin + i));
      const int64_t vb = L.rp[k];   // staged by the lane phase
      int64_t ve;
      if constexpr (LIST) {
        v = uniform(L.vid[k]);
        i = v - a.vbegin;
        ve = L.re[k];
      } else {
        ve = L.rp[k + 1];
      }
      const uint32_t sv_raw = (uint32_t)__builtin_amdgcn_readlane((int)slot_of, k);
      const uint32_t sv_slot = LDONE ? sv_raw & LD_SLOT_MASK : sv_raw;
      u64x2 acc = {0, 0}, want = {0, 0};
      // early-exit rounds: the first pass's column ids are loaded beside the
      // target's seen / component rows, one round trip instead of two
      int32_t col0 = INT32_MIN;
      if constexpr ((MODE & 3) != SCAN_MASKED && (MODE & SCAN_LINES) == 0 && (MODE & SCAN_CML) == 0) {
        if (ee && !((mdn >> k) & 1ull) && lane < (int)min((int64_t)64, ve - vb)) col0 = a.gcol[vb + lane];
      }
      // line-mask rounds (no early exit): the seen row comes up front too, beside
      // the first column ids, parked in LDS for the commit (one round trip less)
      constexpr bool SEEN_EARLY = W == 64 && (MODE & SCAN_LINES) != 0;
      if constexpr (SEEN_EARLY) {
        if (lane < (int)min((int64_t)64, ve - vb)) col0 = a.gcol[vb + lane];
        const u64x2 sv = load_seen<W>(a, v, sv_slot, lw);
        if (g == 0) {
          L.seen[2 * lw] = sv.x;
          L.seen[2 * lw + 1] = sv.y;
        }
        if (sv_slot != SLOT_NONE) st.add(S_SEEN_READ, 1);
      }
      bool covered = false;   // LDONE: the complete lines cover the whole target, nothing to scan
      if (ee) {
        if (sv_slot != SLOT_NONE) st.add(S_SEEN_READ, 1);
        want = early_exit_target<W, LDS_OF(MODE), ALIVE>(a, v, L, g, lw, sv_slot, L.mi[k]);
        // (not in the quads variant: its receivers of in-degree <= 32 take the
        // rule in gather_pairs, and here it cost 4 VGPRs and the seventh wave)
        if constexpr (LDONE && !QUADS) {
          // lines a top in-neighbour held whole: the receiver ends the round
          // with all of cmask there whatever the others hold, so those words
          // are gathered from nobody (gather_rows_n's `live` never loads them).
          // The lanes come from a scalar mask: testing the lane's own line bit
          // took 2 VGPRs and this variant's eighth wave
          const uint32_t ld = sv_raw >> LD_SHIFT;
          if (ld) {
            if (__builtin_amdgcn_inverse_ballot_w64(line_lanes(ld))) acc = want;
            const u64x2 rem = want & ~acc;
            covered = !__any((rem.x | rem.y) != 0ull);
          }
        }
      }
      // (with alive sets a receiver may hold every alive message of its
      // component already: then there is nothing to scan)
      if (ALIVE && ee && a.alive && !__any((want.x | want.y) != 0ull)) {
        if (a.sate) sat |= 1ull << k;
      } else if (((mdn >> k) & 1ull) || covered) {
        // a done in-neighbour: its Message-List is the whole target (covered:
        // complete lines give the same, acc holds it already) -- nothing to scan
        acc = want;
      } else if constexpr ((MODE & 3) == SCAN_PRE) {
        const uint32_t np = L.np[k];
        if (np != 0xFFu) {
          gather_rows<W>(a, L.pre[k], (int)np, g, lw, acc, st, ee, want);   // full rows
        } else {
          gather_scan<W, SCAN, false>(a, vb, vb + L.len[k], L, lane, g, lw, acc, st, ee, want, col0);
          if ((tw >> k) & 1ull) {   // degree-split: the accumulator row (not staged: a scanned receiver)
            if (g == 0) acc |= load_piece<W>(a.acc, v, lw);
            st.add(S_GATHERED, 1);
            st.add(S_ROW_BYTES, (u64)(8 * W));
          }
        }
      } else {
        gather_scan<W, SCAN | (PACK ? SCAN_PACK : 0), DPROBE>(a, vb, ve, L, lane, g, lw, acc, st, ee, want, col0);
      }
      reduce_slots<W, LO>(acc);
      if constexpr (ALIVE) {   // the round's gather covered every alive message v lacked: sated
        if (a.sate && ee && a.alive) {
          const u64x2 rem = want & ~acc;
          if (!__any((rem.x | rem.y) != 0ull)) sat |= 1ull << k;
        }
      }
      if constexpr (W == 64 && (MODE & SCAN_CML) != 0) {
        if (a.cmk) {   // the gathered records (gather_scan ORs them into L.racc)
          wave_sync_lds();
          acc.x |= L.racc[2 * lw];
          acc.y |= L.racc[2 * lw + 1];
          wave_sync_lds();
          L.racc[lane] = 0ull;   // for the next receiver (read by every lane above first)
          wave_sync_lds();
        }
      }
      // alias rounds: a receiver whose gather covered its whole target now
      // holds its component's row (no liveness: want = cm & ~seen)
      bool full = false;
      if (ALIASABLE && a.alias && ee) {
        const u64x2 rem = want & ~acc;
        full = !__any((rem.x | rem.y) != 0ull);
      }
      finish_row<W, true, (MODE & SCAN_CML) != 0, LO>(a, v, i, acc, lane, g, lw, st, L, ee || SEEN_EARLY, sv_slot, k,
                                                      full);
    }
    alive_flush<W>(a, L.alive, lane);
    commit_vertices<LO>(a, L, vi, need, st);
    if constexpr (ALIVE) {
      if (sat && ((sat >> lane) & 1ull)) a.state[a.vbegin + vi] |= ST_SATED;
    }
    // the next round's list: receivers still neither done
    // nor sated -- the set only shrinks (seenpop grows, done_at and the down /
    // sated marks only move one way), so it holds every later receiver
    if constexpr (EMIT) {
      if (a.ulist_next) {
        const bool surv = need && !((sat >> lane) & 1ull) &&
                          a.seenpop[vi] < a.done_at[a.vbegin + vi];   // (commit_vertices' sum: this lane's own write)
        const u64 sm = __ballot(surv);
        if (sm) {
          uint32_t p0 = 0;
          if (lane == 0) p0 = (uint32_t)atomicAdd(a.stats + S_ULIST, (u64)__popcll(sm));
          if constexpr (LO && lane::ON) p0 = (uint32_t)uniform((int)p0);   // (lane 0's: every lane is active)
          else p0 = (uint32_t)__shfl((int)p0, 0);
          if (surv) a.ulist_next[p0 + lane_rank(sm)] = (int32_t)vi;
        }
      }
    }
  }
  flush_stats<EWAVES>(st, a.partial);
}

// One launch per row of round_plan.h's EXPAND_VARIANTS table.  false: no such
// variant is built for W (plan_round asks the table first, so this is a
// mistake in one of the two: the round reports it instead of silently losing
// its pull)
template <int W>
static bool launch_k_expand(Ctx* c, const ExpandArgs& a, int64_t receivers, int mode) {
  const dim3 grid(grid_for(receivers, (int64_t)EWAVES * 64));
  switch (mode) {
#define V(MODE, MINW)                                                                         \
  case (MODE):                                                                                \
    if constexpr (W >= (MINW)) {                                                              \
      hipLaunchKernelGGL((k_expand<W, (MODE)>), grid, dim3(EBLOCK), 0, c->stream, a);         \
      return true;                                                                            \
    }                                                                                         \
    break;
    EXPAND_VARIANTS(V)
#undef V
    default: break;
  }
  return false;
}

// One pull round on the engine stream, with the hub chunks on the context's
// side stream beside the main pull kernel.  What orders what:
//  - k_hub_partial reads only state from before the round (S[cur], sp,
//    seenpop, state and done_at of hubs, the activity / line / done masks) and
//    what the passes before the fork prepare: k_park, k_fixup_rows, k_arcmask,
//    the degree-split push half, k_mklm.  It writes only hub_partial, hub_pnz,
//    hub_done and atomically added stat partials.  The main pull kernel writes
//    none of what it reads: commit_vertices writes `need` lanes only, and a hub
//    is never `need`.  So the chunks wait for the fork alone, and are launched
//    first: their chains are as long as the main kernel's longest.
//  - k_hub_final reads the partials and ORs the hub's nibble into the lm_next
//    byte the main kernel's commit wrote: it follows the join and the main
//    kernel, on the engine stream.
//  - everything after the round (stats reduce, exchange, readers, checkpoint,
//    the next round) is enqueued on the engine stream behind the join; the next
//    round's fork is recorded there after this round's k_hub_final, so the
//    partial buffers are not overwritten while it reads them.
// kernel_ms (ev[4] .. ev[5]) stays on the engine stream around all of it.
enum { PULL_OK = 0, PULL_NOT_BUILT = 1, PULL_ORDER_FAILED = 2 };
template <int W>
static int launch_expand_w(Ctx* c, ExpandArgs a) {
  if (c->plan.mode_push) {
    launch_push_w<W>(c, a);
    return PULL_OK;
  }
  if (c->plan.pull.kernel == PULL_LOSSY) {   // lossy links: a family of its own, none of the pull's passes (lossy.hip)
    if (c->lag_on) launch_expand_delayed_w<W>(c, a);   // delayed links, dmax = 1 included (delayed.hip)
    else if (repair_now(c)) launch_expand_repair_w<W>(c, a);   // a repair round (repair.hip)
    else launch_expand_lossy_w<W>(c, a);
    return PULL_OK;
  }
  if (a.unfiltered && c->liveness_active) launch_park_w<W>(c);
  if (a.unfiltered) launch_fixup_rows_w<W>(c);
  // (k_line_done reads the rows as they are now: after the last round's k_hub_final, before the fork)
  if (a.ldone) launch_line_done(c);
  const PullChoice& p = c->plan.pull;   // (round_plan.h: the kernel, its MODE, its pre-passes)
  if (p.masked) launch_arcmask(c);
  // kernel_ms (ev[4] .. ev[5]) brackets every kernel of the round's pull: the
  // degree-split push half and accumulator clear too (their accumulator
  // updates are in the bench's algorithmic bytes, `atomics`)
  (void)hipEventRecord(c->ev[4], c->stream);
  if (a.prehi) launch_split_push_w<W>(c, a);   // degree-split round, push half: senders of in-degree < split_deg
  // line masks of the senders' rows (inside the pull's events and bytes)
  if (p.lines && !p.lm_from_commits) launch_mklm(c, a);   // (the last round's commits did not write them)
  const bool hubs = c->n_hub_items > 0;
  bool order_ok = true;
  if (hubs) {   // fork: the chunks first, their chains are the round's longest
    order_ok = hipEventRecord(c->ev_fork, c->stream) == hipSuccess &&
               hipStreamWaitEvent(c->side, c->ev_fork, 0) == hipSuccess;
    if (order_ok) {
      launch_hub_partial_w<W>(c, a, a.unfiltered != 0, (p.mode & SCAN_LINES) != 0, c->side);
      order_ok = hipEventRecord(c->ev_join, c->side) == hipSuccess;
    }
  }
  int rc = PULL_OK;
  switch (p.kernel) {
    case PULL_FLAT:
      if constexpr (W <= 32) launch_expand_flat_w<W>(c, a);
      else rc = PULL_NOT_BUILT;
      break;
    case PULL_LIST: if (!launch_k_expand<W>(c, a, a.ulist_n, p.mode)) rc = PULL_NOT_BUILT; break;
    case PULL_RECEIVER: if (!launch_k_expand<W>(c, a, a.nloc, p.mode)) rc = PULL_NOT_BUILT; break;
    case PULL_RECORD: launch_expand_rec(c, a); break;
    case PULL_LOSSY:   // (launched above)
    case PULL_NONE: break;
  }
  if (hubs) {   // join, then the hubs' rows
    order_ok = order_ok && hipStreamWaitEvent(c->stream, c->ev_join, 0) == hipSuccess;
    // kernel_ms brackets the pull kernel and the hub passes: the round's
    // counters (row bytes, arcs scanned, rows written) include the hubs' share
    if (order_ok) launch_hub_final_w<W>(c, a);
  }
  if (a.prehi) launch_acc_clear_w<W>(c);   // degree-split round: the accumulator back to all-zero
  (void)hipEventRecord(c->ev[5], c->stream);
  return order_ok ? rc : PULL_ORDER_FAILED;
}

int launch_round_kernels(Ctx* c, const ExpandArgs& a) {
  int rc = PULL_OK;
  GP_TRY(with_words(c->words, [&](auto w) { rc = launch_expand_w<w()>(c, a); }));
  GP_HIP(hipGetLastError());
  if (rc == PULL_ORDER_FAILED) return set_error(GP_EHIP, "the hub chunks could not be ordered against the round's pull kernel");
  if (rc == PULL_NOT_BUILT) return set_error(GP_EINVAL, "the round chose a pull kernel that is not built for this row width");
  return 0;
}

}  // namespace gp
