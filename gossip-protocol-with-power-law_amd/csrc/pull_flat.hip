// pull_flat.hip -- k_expand_flat, the edge-parallel pull of narrow rows
// (DESIGN.md §3.2), and its launcher.
#include "gp_device.h"

namespace gp {

// edge-parallel pull for narrow rows (W <= 32: message shards, C2/C3 widths).
// The per-receiver loop of k_expand pays several dependent memory round trips
// per receiver, which narrow rows cannot amortise.  Here a wave streams the
// in-arcs of all its (non-hub) receivers as one flat sequence: QA chunks of 64
// arcs have their column ids and activity probes in flight together, the
// active rows are gathered RPI per wave-instruction whatever receiver they
// belong to, and OR-ed into per-receiver accumulators in LDS (ds_or_b64).  The
// receiver side then runs lane-parallel, one receiver per lane.  No early exit
// (narrow rows are cheap next to the arc scan).
constexpr int FLAT_CAP = 512;   // arc positions per owner window
// row wave-instructions in flight per lane (VGPRs vs occupancy).  Measured on
// the message shards (same box A/B): W = 8 (64-B rows, 16 per instruction)
// 15.6 -> 15.2 ms with 3 against 2 for a 512-message shard (round 3 of the
// build), and 5 against 3 at HEAD of round 5 (72 against 76 VGPRs; 4 takes 90):
// ranks 7 / 0 of the N = 8 job 12.12 -> 11.83 / 10.47 -> 10.16 ms
// (profiles/r05_ab_flat_w8.txt; forcing 8 waves per SIMD at 64 VGPRs was
// slower, 12.0-12.2 ms); W = 16 28.3 -> 24.4 ms with 4 and 22.9 ms with 6 for
// a 1024-message shard (8: 25.6).  W < 8: 3 (5 costs W = 1 16 VGPRs)
#ifndef GP_FLAT_RIF_NARROW
#define GP_FLAT_RIF_NARROW 5
#endif
#ifndef GP_FLAT_RIF_WIDE
#define GP_FLAT_RIF_WIDE 6
#endif
template <int W>
struct FlatRIF { static constexpr int value = W >= 16 ? GP_FLAT_RIF_WIDE : W == 8 ? GP_FLAT_RIF_NARROW : 3; };
// receivers per wave: 64, or 32 at W = 32 so that the LDS accumulators (8 KB
// per wave) leave room for 4 blocks per CU
template <int W>
struct FlatNR { static constexpr int value = W >= 32 ? 32 : 64; };
template <int W>
struct FlatLds {
  static constexpr int NR = FlatNR<W>::value;
  u64 acc[NR][W];               // OR accumulators of the wave's NR receivers
  // the passes' staging and the receiver side's words share their bytes (the
  // receiver side starts after the last pass): W = 8 takes 4,928 B + 176 B
  // of counters, so LDS no longer caps its waves (VGPRs do: 7 per SIMD)
  union {
    struct {
      int32_t idx[64];          // active neighbours of one chunk
      int8_t vtx[64];           // their receiver (lane) in the wave
      int8_t own[FLAT_CAP];     // receiver lane owning each arc position of the window
    };
    struct {
      uint16_t tot[NR];         // receiver side: new bits of receiver k (<= 64 W)
      u64 dig[NR];              // its digest terms
      int8_t rd[NR];            // between passes: still missing messages; receiver side: its seen row was read
      u64 alive[W];             // receiver side: OR of the new rows this wave wrote (alive_next)
    };
  };
};

// one flat pass: the arcs [start, start + sdeg) of every lane's receiver, as
// one sequence (owner windows of FLAT_CAP positions), OR-ed into F.acc.
// Returns the rows gathered.
template <int W, int MODE>
__device__ __forceinline__ u64 flat_pass(const ExpandArgs& a, FlatLds<W>& F, int lane, int g, int lw,
                                         uint32_t sdeg, int64_t start, WaveStats& st) {
  constexpr int RPI = Geo<W>::RPI;
  constexpr int WPL = Geo<W>::WPL;
  constexpr int QA = 4;
  constexpr int RIF = FlatRIF<W>::value;
  const uint32_t excl = wave_excl_scan_u32(sdeg, lane);
  const uint32_t incl = excl + sdeg;
  const uint32_t T = (uint32_t)__shfl((int)incl, 63);
  const uint32_t vb_lo = (uint32_t)start, vb_hi = (uint32_t)((u64)start >> 32);
  st.add(S_ARCS, T);
  u64 gathered = 0;
  for (uint32_t g0 = 0; g0 < T; g0 += FLAT_CAP) {
    const uint32_t wn = min((uint32_t)FLAT_CAP, T - g0);
    // owner table of positions [g0, g0 + wn): start markers, then a forward
    // fill seeded with the receiver that straddles g0
    {
      u64* own8 = reinterpret_cast<u64*>(F.own);
      own8[lane] = 0xFFFFFFFFFFFFFFFFull;
      wave_sync_lds();
      if (sdeg && excl >= g0 && excl < g0 + wn) F.own[excl - g0] = (int8_t)lane;
      const u64 before = __ballot(sdeg && excl < g0);
      const int carry_in = before ? 63 - __clzll((long long)before) : -1;
      wave_sync_lds();
      const u64 w8 = own8[lane];
      int run = -1;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int o = (int8_t)((w8 >> (8 * q)) & 0xFF);
        if (o >= 0) run = o;
      }
      int carry = run;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(carry, o);
        if (lane >= o) carry = max(carry, y);
      }
      int cur = __shfl_up(carry, 1);
      if (lane == 0) cur = carry_in;
      cur = max(cur, carry_in);
      u64 out = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int o = (int8_t)((w8 >> (8 * q)) & 0xFF);
        if (o >= 0) cur = o;
        out |= (u64)(uint8_t)(int8_t)cur << (8 * q);
      }
      own8[lane] = out;
      wave_sync_lds();
    }
    for (uint32_t c0 = 0; c0 < wn; c0 += 64 * QA) {
      int32_t col[QA];
      int8_t who[QA];
#pragma unroll
      for (int q = 0; q < QA; ++q) {
        const uint32_t p = c0 + (uint32_t)(q * 64 + lane);
        const int j = p < wn ? (int)F.own[p] : 0;
        // shuffles with the whole wave active (bpermute reads every lane)
        const int64_t b = (int64_t)(((u64)(uint32_t)__shfl((int)vb_hi, j) << 32) |
                                    (u64)(uint32_t)__shfl((int)vb_lo, j));
        const uint32_t s = (uint32_t)__shfl((int)excl, j);
        who[q] = (int8_t)j;
        col[q] = -1;
        if (p < wn) col[q] = a.gcol[b + (g0 + p - s)];
      }
      u64 raw[QA];   // activity words, all in flight before the first use
#pragma unroll
      for (int q = 0; q < QA; ++q) {
        raw[q] = ~0ull;
        if constexpr (MODE != SCAN_UNFILTERED)
          if (col[q] >= 0) raw[q] = a.abits[col[q] >> 6];
      }
      if constexpr (MODE != SCAN_UNFILTERED)
        if (a.sbits) {
          u64 sw[QA];
#pragma unroll
          for (int q = 0; q < QA; ++q) sw[q] = col[q] >= 0 ? a.sbits[col[q] >> 12] : 0ull;
#pragma unroll
          for (int q = 0; q < QA; ++q)
            raw[q] = ((sw[q] >> ((col[q] >> 6) & 63)) & 1ull) ? a.abits[col[q] >> 6] : 0ull;
        }
#pragma unroll
      for (int q = 0; q < QA; ++q) {
        const int32_t u = (col[q] >= 0 && ((raw[q] >> (col[q] & 63)) & 1ull)) ? col[q] : -1;
        const u64 am = __ballot(u >= 0);
        const int cnt = __popcll(am);
        if (cnt == 0) continue;
        if (u >= 0) {
          const int r = lane_rank(am);
          F.idx[r] = u;
          F.vtx[r] = who[q];
        }
        wave_sync_lds();
        gathered += (u64)cnt;
        for (int k0 = 0; k0 < cnt; k0 += RIF * RPI) {
          u64x2 r[RIF];
#pragma unroll
          for (int t = 0; t < RIF; ++t) {
            const int k = k0 + g + t * RPI;
            r[t] = u64x2{0, 0};
            if (k < cnt) r[t] = load_piece<W>(a.rows, F.idx[k], lw);
          }
#pragma unroll
          for (int t = 0; t < RIF; ++t) {
            const int k = k0 + g + t * RPI;
            if (k < cnt) {
              u64* dst = &F.acc[F.vtx[k]][lw * WPL];
              if (r[t].x) atomicOr(dst, r[t].x);
              if constexpr (WPL == 2) {
                if (r[t].y) atomicOr(dst + 1, r[t].y);
              }
            }
          }
        }
        wave_sync_lds();
      }
    }
  }
  return gathered;
}

// early-exit rounds: the first GP_FLAT_EE_PREFIX arcs of every
// receiver (its biggest neighbours: gather order) go in a first pass; only
// receivers still missing messages of their component after it scan further
// (a second prefix pass of 8 arcs measured no better, §3.7).
#ifndef GP_FLAT_EE_PREFIX
#define GP_FLAT_EE_PREFIX 2
#endif

template <int W, int MODE, bool EE>
__global__ __launch_bounds__(EBLOCK) void k_expand_flat(ExpandArgs a) {
  constexpr int LPR = Geo<W>::LPR;
  constexpr int RPI = Geo<W>::RPI;
  constexpr int WPL = Geo<W>::WPL;
  __shared__ FlatLds<W> s_f[EWAVES];
  const int lane = threadIdx.x & 63;
  const int wib = uniform(threadIdx.x >> 6);
  const int g = lane / LPR, lw = lane % LPR;
  FlatLds<W>& F = s_f[wib];
  constexpr int NR = FlatNR<W>::value;
  WaveStats st;
  ws_zero<EWAVES>(st);
  const int64_t base = ((int64_t)blockIdx.x * EWAVES + wib) * NR;
  if (base < a.nloc) {
    // per-lane state is reloaded (coalesced) where it is needed rather than
    // kept live across the passes: VGPRs are what bound this kernel's waves
    const int64_t li = base + lane;
    const bool mine = lane < NR && li < a.nloc;   // lane = receiver
    const int v = mine ? (int)(a.vbegin + li) : 0;
    u64 needm;
    {
      bool need = false, act = false;
      u64 sends = 0;
      if (mine) {
        const uint32_t fp = a.fpop[v];
        act = fp != 0u;
        if (act) sends = (u64)fp * (u64)(uint32_t)max(a.deg_live[v], 0);
        const int64_t b = a.row_ptr[v], e = a.row_ptr[v + 1];
        const bool hub = e - b > a.hub_thr;   // split over waves by the hub kernels
        need = !(a.state[v] & (ST_DOWN | ST_SATED)) && a.seenpop[li] < a.done_at[v] && !hub && e > b;
        if (!need && !hub) a.fpop_next[v] = 0;
      }
      st.add(S_SENDS, wave_sum_u64(sends));
      st.add(S_ACTIVE, (u64)__popcll(__ballot(act)));
      needm = __ballot(need);
      st.add(S_VISITED, (u64)__popcll(needm));
    }
    const bool need = (needm >> lane) & 1ull;
    // degree-split rounds: the receivers the push half touched (bit r =
    // receiver base + r; NR = 32 waves take their half of the 64-vertex word)
    u64 tw = 0;
    if (a.prehi) {
      tw = a.tbits[base >> 6] >> (base & 63);
      if constexpr (NR < 64) tw &= (1ull << NR) - 1ull;
    }
    // (a wave with no receiver to scan is done: late rounds leave most waves
    // with none, and the passes and the receiver side cost latency even empty)
    if (needm != 0ull) {
    if (lane < NR) {
#pragma unroll
      for (int w = 0; w < W; ++w) F.acc[lane][w] = 0ull;
    }
    // one pass, or (early-exit rounds) a prefix pass and a pass over the rest
    // of the in-lists of the receivers still missing messages
    constexpr uint32_t K1 = GP_FLAT_EE_PREFIX, K2 = 0;
    constexpr bool ee = EE && K1 > 0;   // compile-time: the lean kernel keeps its VGPRs
    constexpr int npass = !ee ? 1 : 2;
    u64 gathered = 0;
    u64 todo = needm;   // receivers of this pass
#pragma nounroll
    for (int pass = 0; pass < npass; ++pass) {
      // this pass covers in-list positions [lo, hi)
      const uint32_t lo = pass == 0 ? 0u : pass == 1 ? K1 : K2;
      const uint32_t hi = pass + 1 == npass ? 0xFFFFFFFFu : pass == 0 ? K1 : K2;
      uint32_t sdeg = 0;
      int64_t start = 0;
      if ((todo >> lane) & 1ull) {
        const int64_t b = a.row_ptr[v], e = a.row_ptr[v + 1];
        // (degree-split rounds, no early exit: the prefix of bigger senders)
        const uint32_t deg = a.prehi ? (uint32_t)a.prehi[v] : (uint32_t)(e - b);
        sdeg = deg > lo ? min(deg, hi) - lo : 0u;
        start = b + lo;
      }
      gathered += flat_pass<W, MODE>(a, F, lane, g, lw, sdeg, start, st);
      if (pass + 1 == npass) break;
      // which receivers with arcs left still miss messages of their component?
      bool longer = false;
      uint32_t slot_of = SLOT_NONE;
      int32_t mrow = -1;
      if ((todo >> lane) & 1ull) {
        longer = a.row_ptr[v + 1] - a.row_ptr[v] > (int64_t)hi;
        if (longer) {
          slot_of = a.sp[v];
          mrow = a.midx[v];
        }
      }
      const u64 longm = __ballot(longer);
      wave_sync_lds();
#pragma nounroll
      for (int r0 = 0; r0 < NR; r0 += RPI) {
        const int r = r0 + g;
        const uint32_t rslot = (uint32_t)__shfl((int)slot_of, r);
        const int rv = __shfl(v, r);
        const int32_t rm = __shfl(mrow, r);
        bool miss = false;
        if ((longm >> r) & 1ull) {
          u64x2 accp;
          accp.x = F.acc[r][lw * WPL];
          accp.y = 0;
          if constexpr (WPL == 2) accp.y = F.acc[r][lw * WPL + 1];
          const u64x2 sv = rslot != SLOT_NONE ? load_piece<W>(a.slot[rslot], rv, lw) : u64x2{0, 0};
          u64x2 cm = load_piece<W>(a.cmask, rm, lw);
          if (a.alive) cm &= load_piece<W>(a.alive, 0, lw);
          const u64x2 m = cm & ~(sv | accp);
          miss = (m.x | m.y) != 0ull;
        }
        miss = group_or<LPR>(miss);
        if (lw == 0) F.rd[r] = (int8_t)miss;
      }
      wave_sync_lds();
      todo = __ballot(((longm >> lane) & 1ull) && F.rd[lane]);
    }
    const u64 tn = (u64)__popcll(tw & needm);   // accumulator rows read by the receiver side
    st.add(S_GATHERED, gathered + tn);
    st.add(S_ROW_BYTES, (gathered + tn) * (u64)(8 * W));
    // receiver side: RPI receivers per wave-instruction, LPR lanes x 16 B per
    // row (coalesced, like the gather); a receiver with nothing new reads and
    // writes nothing.  Per-receiver words go to F.tot / F.dig, then one
    // coalesced commit with one receiver per lane.
    wave_sync_lds();
    alive_zero<W>(a, F.alive, lane);   // (shares its bytes with the passes' staging)
    wave_sync_lds();
    const uint32_t slot_of = need ? a.sp[v] : SLOT_NONE;
    for (int r0 = 0; r0 < NR; r0 += RPI) {
      const int r = r0 + g;
      const uint32_t rslot = (uint32_t)__shfl((int)slot_of, r);
      const int rv = __shfl(v, r);
      const bool rn = (needm >> r) & 1ull;
      u64x2 accp = {0, 0};
      if (rn) {
        accp.x = F.acc[r][lw * WPL];
        if constexpr (WPL == 2) accp.y = F.acc[r][lw * WPL + 1];
        if ((tw >> r) & 1ull) accp |= load_piece<W>(a.acc, rv, lw);   // degree-split: the pushed rows
      }
      const bool any = group_or<LPR>((accp.x | accp.y) != 0ull);
      u64x2 sv = {0, 0};
      if (any && rslot != SLOT_NONE) sv = load_piece<W>(a.slot[rslot], rv, lw);
      const u64x2 nw = accp & ~sv;
      const uint32_t tot = group_sum<LPR>((uint32_t)(__popcll(nw.x) + __popcll(nw.y)));
      u64 t = 0;
      if (tot) {
        alive_add<W>(a, F, lw, nw);
        store_piece<W>(a.slot[a.wslot], rv, lw, sv | nw);
        if (a.frx_next) store_piece<W>(a.frx_next, rv, lw, nw);
        if (a.first) {
          uint8_t* row = a.first + (size_t)(base + r) * (W * 64);
          if (nw.x) set_first_bytes(row, lw * WPL, nw.x, (uint32_t)a.rr);
          if (WPL == 2 && nw.y) set_first_bytes(row, lw * WPL + 1, nw.y, (uint32_t)a.rr);
        }
        if (a.digest) {
          if (nw.x) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + lw * WPL), nw.x);
          if (WPL == 2 && nw.y) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + lw * WPL + 1), nw.y);
        }
      }
      t = group_xor<LPR>(t);
      if (lw == 0) {
        F.tot[r] = tot;
        F.dig[r] = t;
        F.rd[r] = (int8_t)(any && rslot != SLOT_NONE);
      }
    }
    wave_sync_lds();
    u64 nbits = 0, nrecv = 0, nwritten = 0, narcs = 0, nseen = 0;
    if (need) {
      const uint32_t tot = F.tot[lane];
      nseen = (u64)F.rd[lane];
      a.fpop_next[v] = tot;
      if (tot) {
        a.seenpop[li] += tot;
        a.sp[v] = (uint8_t)a.wslot;
        a.ws[v] |= (uint8_t)(1u << a.wslot);
        if (a.digest) a.digest[li] ^= F.dig[lane];
        nbits = tot;
        nrecv = 1;
        nwritten = 1;
        narcs = (u64)(uint32_t)max(a.deg_live[v], 0);
      }
    }
    st.add(S_NEW_BITS, wave_sum_u64(nbits));
    st.add(S_RECEIVERS, wave_sum_u64(nrecv));
    st.add(S_WRITTEN, wave_sum_u64(nwritten));
    st.add(S_NEXT_ARCS, wave_sum_u64(narcs));
    st.add(S_SEEN_READ, wave_sum_u64(nseen));
    alive_flush<W>(a, F.alive, lane);
    }   // needm
  }
  flush_stats<EWAVES>(st, a.partial);
}

template <int W>
void launch_expand_flat_w(Ctx* c, const ExpandArgs& a) {
  const dim3 grid(grid_for(a.nloc, (int64_t)EWAVES * FlatNR<W>::value));
  const bool ee = a.early_exit != 0 && GP_FLAT_EE_PREFIX > 0;
  if (a.unfiltered) {
    if (ee) hipLaunchKernelGGL((k_expand_flat<W, SCAN_UNFILTERED, true>), grid, dim3(EBLOCK), 0, c->stream, a);
    else hipLaunchKernelGGL((k_expand_flat<W, SCAN_UNFILTERED, false>), grid, dim3(EBLOCK), 0, c->stream, a);
  } else {
    if (ee) hipLaunchKernelGGL((k_expand_flat<W, SCAN_FILTERED, true>), grid, dim3(EBLOCK), 0, c->stream, a);
    else hipLaunchKernelGGL((k_expand_flat<W, SCAN_FILTERED, false>), grid, dim3(EBLOCK), 0, c->stream, a);
  }
}

// (W <= 32: wider rows never take this kernel)
template void launch_expand_flat_w<1>(Ctx*, const ExpandArgs&);
template void launch_expand_flat_w<2>(Ctx*, const ExpandArgs&);
template void launch_expand_flat_w<4>(Ctx*, const ExpandArgs&);
template void launch_expand_flat_w<8>(Ctx*, const ExpandArgs&);
template void launch_expand_flat_w<16>(Ctx*, const ExpandArgs&);
template void launch_expand_flat_w<32>(Ctx*, const ExpandArgs&);

}  // namespace gp
