// pull_groups.h -- the per-receiver pull's receivers several per wave step
// (pairs: a half-wave per 64-word row; quads: a quarter-wave; groups: a 16- /
// 8- / 4-lane group per W = 32 / 16 / 8 row).  Device helpers of k_expand
// (pull.hip); the record pull's receiver side (pull_rec.hip) commits through
// pair_seen / pair_finish.
#pragma once
#include "gp_device.h"

namespace gp {

// Receivers two at a time, one per half-wave (W = 64).  A half-wave loads a
// whole 64-word row per instruction, so each receiver keeps its rows in flight
// on its own and the dependent chain (column ids -> probes -> rows -> commit)
// is walked for two receivers at once: the latency-bound rounds' lever, since
// 64 VGPRs already give the 8 waves per SIMD the hardware holds.  Same
// commits as finish_row (deferred per-vertex words in L.tot / L.dig / L.cd).
// rows in flight per half-wave in pre_pairs: 2 (70 VGPRs, 7 waves per SIMD)
// against 4 (78, 6 waves): C4 round 1 3.97 -> 3.78 ms same-box
#ifndef GP_PAIR_RIF
#define GP_PAIR_RIF 2
#endif

// receiver side of a pair: half h holds receiver ks (on: the half has one;
// kB < 0: half 1 idle) with its gathered OR acc and its seen row sv
// (alias: both receivers complete their component -- done in-neighbours in an
// a.alias round -- and commit SLOT_CMASK instead of a row, finish_row)
// (LO: the half-wave reductions in registers, lane_ops.h -- k_expand's calls;
// the record pull's keep the LDS shuffles)
template <int W, bool LO = false, class LDS>
__device__ __forceinline__ void pair_finish(const ExpandArgs& a, LDS& L, int h, int lw, bool on, int ks, int kB,
                                            int64_t i, int v, u64x2 acc, u64x2 sv, WaveStats& st,
                                            bool alias = false) {
  const u64x2 nw = acc & ~sv;
  uint32_t tot = (uint32_t)(__popcll(nw.x) + __popcll(nw.y));
  if constexpr (LO && lane::ON) {
    tot = lane::group_sum_u32<32>(tot);
  } else {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) tot += (uint32_t)__shfl_xor((int)tot, o);
  }
  u64 t = 0;
  bool dense = true;   // record of the new Message-List (record-writing rounds)
  if constexpr (LDS::kCml) {
    if (a.cml_next) {
      const u64x2 row = sv | nw;
      const u64 bx = __ballot(row.x != 0ull), by = __ballot(row.y != 0ull);
      const u64 msk = spread32((bx >> (32 * h)) & 0xFFFFFFFFull) | (spread32((by >> (32 * h)) & 0xFFFFFFFFull) << 1);
      dense = __popcll(msk) > CML_MAXW;
      if (!dense && on && tot) {
        u64* rec = a.cml_next + (size_t)v * CML_WORDS;
        const int p = 1 + __popcll(msk & ((1ull << (2 * lw)) - 1ull));
        if (row.x) rec[p] = row.x;
        if (row.y) rec[p + (row.x ? 1 : 0)] = row.y;
        if (lw == 0) rec[0] = msk;
      }
    }
  }
  if (on && tot) {
    alive_add<W>(a, L, lw, nw);
    if (!alias) store_piece<W>(a.slot[a.wslot], v, lw, sv | nw);
    if (a.frx_next) store_piece<W>(a.frx_next, v, lw, nw);
    if (a.first) {
      uint8_t* row = a.first + (size_t)i * (W * 64);
      if (nw.x) set_first_bytes(row, 2 * lw, nw.x, (uint32_t)a.rr);
      if (nw.y) set_first_bytes(row, 2 * lw + 1, nw.y, (uint32_t)a.rr);
    }
    if (a.digest) {
      if (nw.x) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + 2 * lw), nw.x);
      if (nw.y) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + 2 * lw + 1), nw.y);
    }
  }
  if constexpr (LO && lane::ON) {
    t = lane::group_xor_u64<32>(t);
  } else {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) t ^= __shfl_xor(t, o);
  }
  uint32_t lmn = 0;   // lines of the new bits holding a nonzero word (lm_next; finish_row)
  if (a.lm_next) lmn = lines_of((uint32_t)(__ballot(on && (nw.x | nw.y) != 0ull) >> (32 * h)));
  if (lw == 0 && on && tot) {
    L.tot[ks] = tot;
    L.lmn[ks] = (uint8_t)lmn | (alias ? LMN_ALIAS : (uint8_t)0);
    L.dig[ks] = t;
    if constexpr (LDS::kCml) L.cd[ks] = dense ? 1 : 0;
  }
  const uint32_t tA = (uint32_t)__builtin_amdgcn_readlane((int)tot, 0);
  const uint32_t tB = kB >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)tot, 32) : 0u;
  st.add(S_NEW_BITS, (u64)tA + (u64)tB);
  st.add(S_RECEIVERS, (u64)((tA ? 1 : 0) + (tB ? 1 : 0)));
  // (alias is per half: gather_pairs' receivers complete or not each on its own)
  const bool aA = __builtin_amdgcn_readlane((int)alias, 0) != 0, aB = __builtin_amdgcn_readlane((int)alias, 32) != 0;
  st.add(S_ALIASED, (u64)((tA && aA ? 1 : 0) + (tB && aB ? 1 : 0)));
  st.add(S_WRITTEN, (u64)((tA && !aA ? 1 : 0) + (tB && !aB ? 1 : 0)));
}

// the seen row of a pair's receivers, loaded after a gather without early
// exit (only by a half that gathered something), and its S_SEEN_READ count
template <int W>
__device__ __forceinline__ u64x2 pair_seen(const ExpandArgs& a, int h, int lw, bool on, int kB, int v,
                                           uint32_t sv_slot, u64x2 acc, WaveStats& st) {
  const u64 bz = __ballot(on && (acc.x | acc.y) != 0ull);
  const bool any_h = ((bz >> (32 * h)) & 0xFFFFFFFFull) != 0ull;
  u64x2 sv = {0, 0};
  if (any_h && sv_slot != SLOT_NONE) sv = load_piece<W>(a.slot[sv_slot], v, lw);
  const uint32_t sA = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, 0);
  const uint32_t sB = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, 32);
  st.add(S_SEEN_READ, (u64)(((bz & 0xFFFFFFFFull) && sA != SLOT_NONE) ? 1 : 0) +
                          (u64)(((bz >> 32) && kB >= 0 && sB != SLOT_NONE) ? 1 : 0));
  return sv;
}

// SCAN_PRE rounds without early exit (round 1 of a C4 run: 7.9 M receivers,
// about 2 active in-neighbours each, already found by the lane phase)
template <int W, class LDS>
__device__ __forceinline__ void pre_pairs(const ExpandArgs& a, LDS& L, u64 mp, int64_t base, uint32_t slot_of,
                                          WaveStats& st) {
  static_assert(W == 64, "half-wave rows");
  const int lane = threadIdx.x & 63, h = lane >> 5, lw = lane & 31;
  while (mp) {
    const int kA = __ffsll((long long)mp) - 1;
    mp &= mp - 1;
    int kB = -1;
    if (mp) {
      kB = __ffsll((long long)mp) - 1;
      mp &= mp - 1;
    }
    const bool on = h == 0 || kB >= 0;
    const int ks = (h && kB >= 0) ? kB : kA;
    const uint32_t npA = L.np[kA], npB = kB >= 0 ? (uint32_t)L.np[kB] : 0u;
    const uint32_t np = on ? (h ? npB : npA) : 0u;
    const int64_t i = base + ks;
    const int v = (int)(a.vbegin + i);
    const uint32_t sv_slot = (uint32_t)__shfl((int)slot_of, ks);
    u64x2 acc = {0, 0};
    const uint32_t nmax = max(npA, npB);
    for (uint32_t q0 = 0; q0 < nmax; q0 += GP_PAIR_RIF) {
      u64x2 r[GP_PAIR_RIF];
#pragma unroll
      for (int q = 0; q < GP_PAIR_RIF; ++q) {
        r[q] = u64x2{0, 0};
        if (q0 + q < np) r[q] = load_piece<W>(a.rows, L.pre[ks][q0 + q], lw);
      }
#pragma unroll
      for (int q = 0; q < GP_PAIR_RIF; ++q) acc |= r[q];
    }
    st.add(S_GATHERED, (u64)(npA + npB));
    st.add(S_ROW_BYTES, (u64)(npA + npB) * (u64)(8 * W));
    const u64x2 sv = pair_seen<W>(a, h, lw, on, kB, v, sv_slot, acc, st);
    pair_finish<W, true>(a, L, h, lw, on, ks, kB, i, v, acc, sv, st);
  }
}

// The same four at a time (pre_quads; W = 64 without records): a
// quarter-wave per receiver holds a whole 512-B row at 32 B per lane (words
// 4ql .. 4ql + 3), and the receiver's seen row is loaded beside its staged
// rows, one round trip per step instead of two (a receiver whose rows are all
// zero has its seen row read for nothing: round 1's staged senders all send)
// rows in flight per quarter-wave (2: 80 VGPRs, a wave per SIMD less, no faster: profiles/r06_ab_pre_quads.txt)
constexpr int PRE_QUADS_RIF = 1;
template <int NG>
__device__ __forceinline__ int take_group(u64& mq, int (&kq)[NG], int gq);
template <class LDS>
__device__ __forceinline__ void pre_quads(const ExpandArgs& a, LDS& L, u64 mq, int64_t base, uint32_t slot_of,
                                          WaveStats& st) {
  const int lane = threadIdx.x & 63, qd = lane >> 4, ql = lane & 15;
  while (mq) {
    int kq[4];
    const int ks = take_group<4>(mq, kq, qd);
    const bool on = ks >= 0;
    const int64_t i = base + (on ? ks : 0);
    const int v = (int)(a.vbegin + i);
    const uint32_t sv_slot = (uint32_t)__shfl((int)slot_of, on ? ks : 0);
    const int np = on ? (int)L.np[ks] : 0;
    int nmax = 0;
    uint32_t rows = 0, nsr = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int nq = __builtin_amdgcn_readlane(np, 16 * q);
      const uint32_t sq = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, 16 * q);
      nmax = max(nmax, nq);
      rows += (uint32_t)nq;
      nsr += (kq[q] >= 0 && sq != SLOT_NONE) ? 1u : 0u;
    }
    u64x2 s0 = {0, 0}, s1 = {0, 0}, c0 = {0, 0}, c1 = {0, 0};
    if (on && sv_slot != SLOT_NONE) {
      const u64* r = a.slot[sv_slot] + (size_t)v * 64 + 4 * ql;
      s0 = *reinterpret_cast<const u64x2*>(r);
      s1 = *reinterpret_cast<const u64x2*>(r + 2);
    }
    for (int q0 = 0; q0 < nmax; q0 += PRE_QUADS_RIF) {
      if (q0 < np) {   // (one branch per batch; past the last row a lane reloads it: same line, in flight)
        u64x2 r0[PRE_QUADS_RIF], r1[PRE_QUADS_RIF];
#pragma unroll
        for (int q = 0; q < PRE_QUADS_RIF; ++q) {
          const u64* p = a.rows + (size_t)L.pre[ks][min(q0 + q, np - 1)] * 64 + 4 * ql;
          r0[q] = *reinterpret_cast<const u64x2*>(p);
          r1[q] = *reinterpret_cast<const u64x2*>(p + 2);
        }
#pragma unroll
        for (int q = 0; q < PRE_QUADS_RIF; ++q) {
          c0 |= r0[q];
          c1 |= r1[q];
        }
      }
    }
    st.add(S_GATHERED, (u64)rows);
    st.add(S_ROW_BYTES, (u64)rows * 512ull);
    st.add(S_SEEN_READ, nsr);
    const u64x2 n0 = c0 & ~s0, n1 = c1 & ~s1;
    uint32_t tot = (uint32_t)(__popcll(n0.x) + __popcll(n0.y) + __popcll(n1.x) + __popcll(n1.y));
    if constexpr (lane::ON) {   // (every lane active: the loop is wave-uniform)
      tot = lane::group_sum_u32<16>(tot);
    } else {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) tot += (uint32_t)__shfl_xor((int)tot, o);
    }
    u64 t = 0;
    if (on && tot) {
      u64* out = a.slot[a.wslot] + (size_t)v * 64 + 4 * ql;
      *reinterpret_cast<u64x2*>(out) = s0 | n0;
      *reinterpret_cast<u64x2*>(out + 2) = s1 | n1;
      if (a.frx_next) {
        u64* f = a.frx_next + (size_t)v * 64 + 4 * ql;
        *reinterpret_cast<u64x2*>(f) = n0;
        *reinterpret_cast<u64x2*>(f + 2) = n1;
      }
      const u64 nw[4] = {n0.x, n0.y, n1.x, n1.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!nw[j]) continue;
        if (a.alive_next) atomicOr(&L.alive[4 * ql + j], nw[j]);   // (alive_add's words)
        if (a.first) set_first_bytes(a.first + (size_t)i * (64 * 64), 4 * ql + j, nw[j], (uint32_t)a.rr);
        if (a.digest) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + 4 * ql + j), nw[j]);
      }
    }
    if constexpr (lane::ON) {
      t = lane::group_xor_u64<16>(t);
    } else {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) t ^= __shfl_xor(t, o);
    }
    uint32_t lmn = 0;   // lines of the new bits holding a nonzero word (lm_next; pair_finish)
    if (a.lm_next) {
      const uint32_t bq = (uint32_t)((__ballot(on && ((n0.x | n0.y | n1.x | n1.y) != 0ull)) >> (16 * qd)) & 0xFFFFull);
#pragma unroll
      for (int l = 0; l < 4; ++l) lmn |= ((bq >> (4 * l)) & 0xFu) ? (1u << l) : 0u;
    }
    if (ql == 0 && on && tot) {
      L.tot[ks] = tot;
      L.lmn[ks] = (uint8_t)lmn;
      L.dig[ks] = t;
    }
    uint32_t nb = 0, nr = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t tq = (uint32_t)__builtin_amdgcn_readlane((int)tot, 16 * q);
      nb += kq[q] >= 0 ? tq : 0u;
      nr += (kq[q] >= 0 && tq) ? 1u : 0u;
    }
    st.add(S_NEW_BITS, nb);
    st.add(S_RECEIVERS, nr);
    st.add(S_WRITTEN, nr);
  }
}

// Done in-neighbours (a.dbits rounds: early exit, no liveness,
// one context).  Without liveness a receiver's new bits are OR_u seen(u) &
// ~seen(v) over all its in-neighbours (ExpandArgs), and every Message-List is
// a subset of the component's messages cmask, so one in-neighbour that held
// all of them at the end of the last round makes the result exactly cmask &
// ~seen(v): the receiver takes the early-exit target and gathers no row.
// Probed for the first DNB_K arcs of the gather order (the biggest
// neighbours, the first to complete), all loads in flight together (1 or 4
// arcs measured no better).  (Not in
// the flat kernel: its 2-arc prefix pass already reads those rows, and the
// extra probe round trip made the 512-message shard's rounds slower.)
constexpr int DNB_K = 2;
__device__ __forceinline__ bool done_nb(const ExpandArgs& a, int64_t b, int64_t e) {
  int32_t c[DNB_K];
#pragma unroll
  for (int q = 0; q < DNB_K; ++q) c[q] = b + q < e ? a.gcol[b + q] : -1;
  u64 w[DNB_K];
#pragma unroll
  for (int q = 0; q < DNB_K; ++q) w[q] = c[q] >= 0 ? a.dbits[c[q] >> 6] : 0ull;
  bool d = false;
#pragma unroll
  for (int q = 0; q < DNB_K; ++q) d = d || (c[q] >= 0 && ((w[q] >> (c[q] & 63)) & 1ull));
  return d;
}

// Complete lines of a top in-neighbour (a.ldone rounds: early
// exit, no liveness, one context, W = 64).  done_nb's argument per 128-B line:
// if in-neighbour u held every message of the component on line l at the
// start of the round, the OR over v's in-neighbours covers cmask there, every
// Message-List is a subset of cmask, so v's new bits on line l are exactly
// cmask_l & ~seen_l -- and line l of no row need be fetched, u's included.
// k_line_done (pull_aux.hip) wrote the byte of every big vertex before the
// round; probed like done_nb, for the same DNB_K arcs, all loads in flight.
// The mask rides above the slot byte in the lane's slot_of.
constexpr int LD_SHIFT = 8;
constexpr uint32_t LD_SLOT_MASK = (1u << LD_SHIFT) - 1u;
// the lanes of a wave whose 16-B pieces lie on the lines of mask l (W = 64: a
// half-wave per row, 8 lanes per line); l wave-uniform: scalar code
__device__ __forceinline__ u64 line_lanes(uint32_t l) {
  u64 m = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) m |= ((l >> t) & 1u) ? 0x000000FF000000FFull << (8 * t) : 0ull;
  return m;
}
__device__ __forceinline__ uint32_t line_done_nb(const ExpandArgs& a, int64_t b, int64_t e) {
  int32_t c[DNB_K];
#pragma unroll
  for (int q = 0; q < DNB_K; ++q) c[q] = b + q < e ? a.gcol[b + q] : -1;
  uint32_t l = 0;
#pragma unroll
  for (int q = 0; q < DNB_K; ++q) l |= c[q] >= 0 ? (uint32_t)a.ldone[c[q]] : 0u;
  return l & 0xFu;
}

// Receivers with a done in-neighbour two at a time, one per half-wave (W =
// 64): nothing to gather, so each pair is one round trip (its seen rows and
// the component rows, the latter L2-resident) and the commit
template <int W, bool ALIVE, bool ALIAS, class LDS>
__device__ __forceinline__ void dnb_pairs(const ExpandArgs& a, LDS& L, u64 mp, int64_t base, uint32_t slot_of,
                                          WaveStats& st) {
  static_assert(W == 64, "half-wave rows");
  const int lane = threadIdx.x & 63, h = lane >> 5, lw = lane & 31;
  while (mp) {
    const int kA = __ffsll((long long)mp) - 1;
    mp &= mp - 1;
    int kB = -1;
    if (mp) {
      kB = __ffsll((long long)mp) - 1;
      mp &= mp - 1;
    }
    const bool on = h == 0 || kB >= 0;
    const int ks = (h && kB >= 0) ? kB : kA;
    int64_t i = base + ks;
    int v = (int)(a.vbegin + i);
    if constexpr (LDS::kList) {   // (list rounds: lane k's vertex)
      v = L.vid[ks];
      i = v - a.vbegin;
    }
    const uint32_t sv_slot = (uint32_t)__shfl((int)slot_of, ks);
    u64x2 sv = {0, 0}, cm = {0, 0};
    if (on) {
      if (sv_slot != SLOT_NONE) sv = load_piece<W>(a.slot[sv_slot], v, lw);
      cm = load_piece<W>(a.cmask, L.mi[ks], lw);
      if (ALIVE && a.alive) cm &= load_piece<W>(a.alive, 0, lw);   // liveness: the sated neighbour's alive set
    }
    const uint32_t sA = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, 0);
    const uint32_t sB = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, 32);
    st.add(S_SEEN_READ, (u64)((sA != SLOT_NONE ? 1 : 0) + (kB >= 0 && sB != SLOT_NONE ? 1 : 0)));
    pair_finish<W, true>(a, L, h, lw, on, ks, kB, i, v, cm, sv, st, ALIAS && a.alias != 0);
  }
}

// The same four at a time, one per quarter-wave (W = 64, the done-probe
// variants, i.e. the late rounds: C4 round 5's 7.5 M receivers are all done-
// neighbour ones): a quarter-wave holds a whole row at 32 B per lane (words
// 4ql .. 4ql + 3), so four receivers' seen and component rows are in flight
// per round trip instead of two.  No liveness (no alive sets, no records).
template <bool ALIAS, bool ALIVE, class LDS>
__device__ __forceinline__ void dnb_quads(const ExpandArgs& a, LDS& L, u64 mq, int64_t base, uint32_t slot_of,
                                          WaveStats& st) {
  const int lane = threadIdx.x & 63, qd = lane >> 4, ql = lane & 15;
  const bool alias = ALIAS && a.alias != 0;
  while (mq) {
    int kq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      kq[q] = -1;
      if (mq) {
        kq[q] = __ffsll((long long)mq) - 1;
        mq &= mq - 1;
      }
    }
    const int ks = qd == 0 ? kq[0] : qd == 1 ? kq[1] : qd == 2 ? kq[2] : kq[3];
    const bool on = ks >= 0;
    int64_t i = base + (on ? ks : 0);
    int v = (int)(a.vbegin + i);
    if constexpr (LDS::kList) {
      v = on ? L.vid[ks] : 0;
      i = v - a.vbegin;
    }
    const uint32_t sv_slot = (uint32_t)__shfl((int)slot_of, on ? ks : 0);
    u64x2 s0 = {0, 0}, s1 = {0, 0}, c0 = {0, 0}, c1 = {0, 0};
    if (on) {
      if (sv_slot != SLOT_NONE) {
        const u64* r = a.slot[sv_slot] + (size_t)v * 64 + 4 * ql;
        s0 = *reinterpret_cast<const u64x2*>(r);
        s1 = *reinterpret_cast<const u64x2*>(r + 2);
      }
      const u64* cr = a.cmask + (size_t)L.mi[ks] * 64 + 4 * ql;
      c0 = *reinterpret_cast<const u64x2*>(cr);
      c1 = *reinterpret_cast<const u64x2*>(cr + 2);
      if (ALIVE && a.alive) {   // liveness: the sated neighbour's alive set
        c0 &= *reinterpret_cast<const u64x2*>(a.alive + 4 * ql);
        c1 &= *reinterpret_cast<const u64x2*>(a.alive + 4 * ql + 2);
      }
    }
    const u64x2 n0 = c0 & ~s0, n1 = c1 & ~s1;
    uint32_t tot = (uint32_t)(__popcll(n0.x) + __popcll(n0.y) + __popcll(n1.x) + __popcll(n1.y));
    if constexpr (lane::ON) {   // (every lane active: the loop is wave-uniform)
      tot = lane::group_sum_u32<16>(tot);
    } else {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) tot += (uint32_t)__shfl_xor((int)tot, o);
    }
    u64 t = 0;
    if (on && tot) {
      u64* out = a.slot[a.wslot] + (size_t)v * 64 + 4 * ql;
      if (!alias) {
        *reinterpret_cast<u64x2*>(out) = s0 | n0;
        *reinterpret_cast<u64x2*>(out + 2) = s1 | n1;
      }
      if (a.frx_next) {
        u64* f = a.frx_next + (size_t)v * 64 + 4 * ql;
        *reinterpret_cast<u64x2*>(f) = n0;
        *reinterpret_cast<u64x2*>(f + 2) = n1;
      }
      const u64 nw[4] = {n0.x, n0.y, n1.x, n1.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!nw[j]) continue;
        if (ALIVE && a.alive_next) atomicOr(&L.alive[4 * ql + j], nw[j]);   // (alive_add's words)
        if (a.first) set_first_bytes(a.first + (size_t)i * (64 * 64), 4 * ql + j, nw[j], (uint32_t)a.rr);
        if (a.digest) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + 4 * ql + j), nw[j]);
      }
    }
    if constexpr (lane::ON) {
      t = lane::group_xor_u64<16>(t);
    } else {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) t ^= __shfl_xor(t, o);
    }
    if (ql == 0 && on && tot) {
      L.tot[ks] = tot;
      L.lmn[ks] = alias ? LMN_ALIAS : (uint8_t)0;   // (no line masks are written in early-exit rounds)
      L.dig[ks] = t;
    }
    uint32_t nb = 0, nr = 0, nsr = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t tq = (uint32_t)__builtin_amdgcn_readlane((int)tot, 16 * q);
      const uint32_t sq = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, 16 * q);
      nb += kq[q] >= 0 ? tq : 0u;
      nr += (kq[q] >= 0 && tq) ? 1u : 0u;
      nsr += (kq[q] >= 0 && sq != SLOT_NONE) ? 1u : 0u;
    }
    st.add(S_NEW_BITS, nb);
    st.add(S_RECEIVERS, nr);
    st.add(alias ? S_ALIASED : S_WRITTEN, nr);
    st.add(S_SEEN_READ, nsr);
  }
}

// W = 32 rows (two-rank message shards): receivers four per wave step, one
// per 16-lane group (a 256-B row at 16 B per lane, the load_piece layout of
// group g = lane / 16), where the serial loop took them one at a time -- the
// done-neighbour receivers (dnb_groups: the N = 2 job's slow rank ran 7.5 M
// of them in round 5 at 3.1 ms) and the prefiltered ones of sparse rounds
// (pre_groups).  group_finish commits like finish_row (deferred per-vertex
// words, L.tot / L.dig).  (A/B against the serial loop: profiles/r06_ab_w32_groups.txt)
template <int W>
struct Groups {
  static constexpr int LG = Geo<W>::LPR;   // lanes per row
  static constexpr int NG = 64 / LG;       // receivers per step
  static_assert(Geo<W>::WPL == 2 && NG >= 2 && NG <= 16, "16-B pieces, two to sixteen rows per wave");
};

// the next NG receivers of mq (kq[q] = -1: none); returns group gq's
template <int NG>
__device__ __forceinline__ int take_group(u64& mq, int (&kq)[NG], int gq) {
  int ks = -1;
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    kq[q] = -1;
    if (mq) {
      kq[q] = __ffsll((long long)mq) - 1;
      mq &= mq - 1;
    }
    if (q == gq) ks = kq[q];
  }
  return ks;
}

template <int W, class LDS>
__device__ __forceinline__ void group_finish(const ExpandArgs& a, LDS& L, int lw, bool on, int ks,
                                             const int (&kq)[Groups<W>::NG], int64_t i, int v, u64x2 acc,
                                             u64x2 sv, WaveStats& st) {
  constexpr int LG = Groups<W>::LG, NG = Groups<W>::NG;
  const u64x2 nw = acc & ~sv;
  uint32_t tot = (uint32_t)(__popcll(nw.x) + __popcll(nw.y));
  if constexpr (lane::ON) {
    tot = lane::group_sum_u32<LG>(tot);
  } else {
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) tot += (uint32_t)__shfl_xor((int)tot, o);
  }
  u64 t = 0;
  if (on && tot) {
    alive_add<W>(a, L, lw, nw);
    store_piece<W>(a.slot[a.wslot], v, lw, sv | nw);
    if (a.frx_next) store_piece<W>(a.frx_next, v, lw, nw);
    if (a.first) {
      uint8_t* row = a.first + (size_t)i * (W * 64);
      if (nw.x) set_first_bytes(row, 2 * lw, nw.x, (uint32_t)a.rr);
      if (nw.y) set_first_bytes(row, 2 * lw + 1, nw.y, (uint32_t)a.rr);
    }
    if (a.digest) {
      if (nw.x) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + 2 * lw), nw.x);
      if (nw.y) t ^= digest_term((uint32_t)a.rr, (uint32_t)(a.wbase + 2 * lw + 1), nw.y);
    }
  }
  if constexpr (lane::ON) {
    t = lane::group_xor_u64<LG>(t);
  } else {
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) t ^= __shfl_xor(t, o);
  }
  if (lw == 0 && on && tot) {
    L.tot[ks] = tot;
    L.lmn[ks] = 0;   // (line masks: W = 64 only)
    L.dig[ks] = t;
  }
  uint32_t nb = 0, nr = 0;
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    const uint32_t tq = (uint32_t)__builtin_amdgcn_readlane((int)tot, LG * q);
    nb += kq[q] >= 0 ? tq : 0u;
    nr += (kq[q] >= 0 && tq) ? 1u : 0u;
  }
  st.add(S_NEW_BITS, nb);
  st.add(S_RECEIVERS, nr);
  st.add(S_WRITTEN, nr);
}

// groups whose receiver's seen row was read (S_SEEN_READ): on[q] && slot[q] != SLOT_NONE
template <int W>
__device__ __forceinline__ uint32_t group_seen_reads(const int (&kq)[Groups<W>::NG], uint32_t sv_slot, u64 read) {
  constexpr int LG = Groups<W>::LG, NG = Groups<W>::NG;
  uint32_t n = 0;
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    const uint32_t sq = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, LG * q);
    n += (kq[q] >= 0 && sq != SLOT_NONE && ((read >> (LG * q)) & 1ull)) ? 1u : 0u;
  }
  return n;
}

template <int W, bool ALIVE, class LDS>
__device__ __forceinline__ void dnb_groups(const ExpandArgs& a, LDS& L, u64 mq, int64_t base, uint32_t slot_of,
                                           WaveStats& st) {
  constexpr int LG = Groups<W>::LG, NG = Groups<W>::NG;
  const int lane = threadIdx.x & 63, gq = lane / LG, lw = lane % LG;
  while (mq) {
    int kq[NG];
    const int ks = take_group<NG>(mq, kq, gq);
    const bool on = ks >= 0;
    int64_t i = base + (on ? ks : 0);
    int v = (int)(a.vbegin + i);
    if constexpr (LDS::kList) {
      v = on ? L.vid[ks] : 0;
      i = v - a.vbegin;
    }
    const uint32_t sv_slot = (uint32_t)__shfl((int)slot_of, on ? ks : 0);
    u64x2 sv = {0, 0}, cm = {0, 0};
    if (on) {
      if (sv_slot != SLOT_NONE) sv = load_piece<W>(a.slot[sv_slot], v, lw);
      cm = load_piece<W>(a.cmask, L.mi[ks], lw);
      if (ALIVE && a.alive) cm &= load_piece<W>(a.alive, 0, lw);   // liveness: the sated neighbour's alive set
    }
    st.add(S_SEEN_READ, group_seen_reads<W>(kq, sv_slot, ~0ull));
    group_finish<W>(a, L, lw, on, ks, kq, i, v, cm & ~sv, sv, st);
  }
}

// SCAN_PRE rounds without early exit: the receivers whose active
// in-neighbours the lane phase staged (L.pre, at most PRE_IDS), four at a time
template <int W, class LDS>
__device__ __forceinline__ void pre_groups(const ExpandArgs& a, LDS& L, u64 mp, int64_t base, uint32_t slot_of,
                                           WaveStats& st) {
  constexpr int LG = Groups<W>::LG, NG = Groups<W>::NG;
  const int lane = threadIdx.x & 63, gq = lane / LG, lw = lane % LG;
  while (mp) {
    int kq[NG];
    const int ks = take_group<NG>(mp, kq, gq);
    const bool on = ks >= 0;
    const int64_t i = base + (on ? ks : 0);
    const int v = (int)(a.vbegin + i);
    const uint32_t sv_slot = (uint32_t)__shfl((int)slot_of, on ? ks : 0);
    const int np = on ? (int)L.np[ks] : 0;
    int nmax = 0;
    uint32_t rows = 0;
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      const int nq = __builtin_amdgcn_readlane(np, LG * q);
      nmax = max(nmax, nq);
      rows += (uint32_t)nq;
    }
    u64x2 acc = {0, 0};
    for (int q0 = 0; q0 < nmax; q0 += GP_PAIR_RIF) {
      if (q0 < np) {   // (one branch per batch; past the last row a lane reloads it: same line, in flight)
        u64x2 r[GP_PAIR_RIF];
#pragma unroll
        for (int q = 0; q < GP_PAIR_RIF; ++q) r[q] = load_piece<W>(a.rows, L.pre[ks][min(q0 + q, np - 1)], lw);
#pragma unroll
        for (int q = 0; q < GP_PAIR_RIF; ++q) acc |= r[q];
      }
    }
    st.add(S_GATHERED, (u64)rows);
    st.add(S_ROW_BYTES, (u64)rows * (u64)(8 * W));
    // the seen row only where the gather found something (pair_seen)
    const u64 bz = __ballot(on && (acc.x | acc.y) != 0ull);
    u64 gz = 0;   // bit LG * q: group q gathered a nonzero word
#pragma unroll
    for (int q = 0; q < NG; ++q)
      if ((bz >> (LG * q)) & ((1ull << LG) - 1ull)) gz |= 1ull << (LG * q);
    u64x2 sv = {0, 0};
    if (((gz >> (LG * gq)) & 1ull) && sv_slot != SLOT_NONE) sv = load_piece<W>(a.slot[sv_slot], v, lw);
    st.add(S_SEEN_READ, group_seen_reads<W>(kq, sv_slot, gz));
    group_finish<W>(a, L, lw, on, ks, kq, i, v, acc, sv, st);
  }
}

// rows in flight per receiver of gather_pairs (W = 64: 2, 72 VGPRs, 7 waves
// per SIMD; 3 took 76 and 6 waves: C4 round 4 6.70-6.74 -> 6.44-6.48 ms with
// 2) and of gather_groups (W = 32: 3; 2 was slower, profiles/r06_ab_grif.txt)
#ifndef GP_GPAIR_RIF
#define GP_GPAIR_RIF 2
#endif
#ifndef GP_GGROUP_RIF
#define GP_GGROUP_RIF 3
#endif

// W = 32 near-done unfiltered pulls: receivers of in-degree <= 16 four per
// wave step, one per 16-lane group (gather_pairs' scheme at a 256-B row per
// group-instruction): column ids, seen and component rows in one round trip,
// then GP_GGROUP_RIF rows per group in flight until the target is covered.
template <int W, class LDS>
__device__ __forceinline__ void gather_groups(const ExpandArgs& a, LDS& L, u64 mp, int64_t base, uint32_t slot_of,
                                              WaveStats& st) {
  constexpr int LG = Groups<W>::LG, NG = Groups<W>::NG;
  const int lane = threadIdx.x & 63, gq = lane / LG, lw = lane % LG;
  const bool ee = a.early_exit != 0;
  while (mp) {
    int kq[NG];
    const int ks = take_group<NG>(mp, kq, gq);
    const bool on = ks >= 0;
    const int64_t i = base + (on ? ks : 0);
    const int v = (int)(a.vbegin + i);
    const int64_t vb = L.rp[on ? ks : 0];
    const int deg = on ? (int)(L.rp[ks + 1] - vb) : 0;   // <= LG (the caller's mask)
    const uint32_t sv_slot = (uint32_t)__shfl((int)slot_of, on ? ks : 0);
    if (lw < deg) L.idx[LG * gq + lw] = a.gcol[vb + lw];
    u64x2 sv = {0, 0}, want = {0, 0};
    if (on) {
      if (sv_slot != SLOT_NONE) sv = load_piece<W>(a.slot[sv_slot], v, lw);
      if (ee) want = load_piece<W>(a.cmask, L.mi[ks], lw) & ~sv;
    }
    wave_sync_lds();
    int dq[NG], dmax = 0, arcs = 0;
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      dq[q] = __builtin_amdgcn_readlane(deg, LG * q);
      dmax = max(dmax, dq[q]);
      arcs += dq[q];
    }
    st.add(S_ARCS, (u64)arcs);
    st.add(S_SEEN_READ, group_seen_reads<W>(kq, sv_slot, ~0ull));
    bool live = on && (!ee || (want.x | want.y) != 0ull);
    u64x2 acc = {0, 0};
    u64 rows = 0, pieces = 0;
    for (int k0 = 0; k0 < dmax; k0 += GP_GGROUP_RIF) {
      const u64 lb = __ballot(live);
      if (lb == 0ull) break;
      if (live && k0 < deg) {   // (one branch per batch, gather_pairs)
        u64x2 r[GP_GGROUP_RIF];
#pragma unroll
        for (int q = 0; q < GP_GGROUP_RIF; ++q) r[q] = load_piece<W>(a.rows, L.idx[LG * gq + min(k0 + q, deg - 1)], lw);
#pragma unroll
        for (int q = 0; q < GP_GGROUP_RIF; ++q) acc |= r[q];
      }
#pragma unroll
      for (int q = 0; q < GP_GGROUP_RIF; ++q) pieces += line_pieces<W>(__ballot(live && k0 + q < deg));
#pragma unroll
      for (int q = 0; q < NG; ++q)
        if ((lb >> (LG * q)) & ((1ull << LG) - 1ull)) rows += (u64)min(GP_GGROUP_RIF, max(dq[q] - k0, 0));
      if (ee) {
        const u64x2 miss = want & ~acc;
        live = live && (miss.x | miss.y) != 0ull;
      }
    }
    st.add(S_GATHERED, rows);
    st.add(S_ROW_BYTES, pieces * 16ull);
    wave_sync_lds();   // (the next step's column ids overwrite L.idx)
    group_finish<W>(a, L, lw, on, ks, kq, i, v, acc, sv, st);
  }
}

// Receivers of in-degree <= 32 two at a time, one per half-wave (W = 64, the
// unfiltered SCAN_QUADS variants: near-done pulls, C4 round 4 / C5 rounds
// 4-5, where a receiver lacks a few words and gathers ~8 rows).  A half loads
// its receiver's column ids (one per lane), seen row and component row in one
// round trip, then gathers GP_GPAIR_RIF rows at a time (a whole 512-B row per
// half-wave instruction) until they cover its target (per-lane word skip as in
// gather_rows_n).  The serial loop walks target -> rows -> rows one receiver
// after the other; here two receivers' chains share each round trip.  Same
// rows, commits and sated marks as the serial loop (returned: the sated
// receivers, alive rounds).
template <bool ALIVE, bool ALIAS, class LDS>
__device__ __forceinline__ u64 gather_pairs(const ExpandArgs& a, LDS& L, u64 mp, int64_t base, uint32_t slot_of,
                                            WaveStats& st) {
  constexpr int W = 64;
  const int lane = threadIdx.x & 63, h = lane >> 5, lw = lane & 31;
  const bool ee = a.early_exit != 0;
  u64 sat = 0;
  while (mp) {
    const int kA = __ffsll((long long)mp) - 1;
    mp &= mp - 1;
    int kB = -1;
    if (mp) {
      kB = __ffsll((long long)mp) - 1;
      mp &= mp - 1;
    }
    const bool on = h == 0 || kB >= 0;
    const int ks = (h && kB >= 0) ? kB : kA;
    const int v = (int)(a.vbegin + base + ks);
    const int64_t vb = L.rp[ks];
    const int deg = on ? (int)(L.rp[ks + 1] - vb) : 0;   // <= 32 (the caller's mask)
    // the receiver's slot, with the complete lines of its top in-neighbours
    // above it (line_done_nb; none: 0)
    const uint32_t sv_raw = (uint32_t)__shfl((int)slot_of, ks);
    const uint32_t sv_slot = sv_raw & LD_SLOT_MASK;
    u64x2 want = {0, 0};
    if (lw < deg) L.idx[32 * h + lw] = a.gcol[vb + lw];   // (this pair's column ids: half h at 32h)
    wave_sync_lds();
    {
      u64x2 sv = {0, 0};
      if (on) {
        if (sv_slot != SLOT_NONE) sv = load_piece<W>(a.slot[sv_slot], v, lw);
        if (ee) {
          u64x2 cm = load_piece<W>(a.cmask, L.mi[ks], lw);
          if (ALIVE && a.alive) cm &= load_piece<W>(a.alive, 0, lw);
          want = cm & ~sv;
        }
      }
      L.seen[64 * h + 2 * lw] = sv.x;   // (parked for the commit: registers for the rows in flight)
      L.seen[64 * h + 2 * lw + 1] = sv.y;
    }
    const int dA = __builtin_amdgcn_readlane(deg, 0), dB = __builtin_amdgcn_readlane(deg, 32);
    const uint32_t sA = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, 0);
    const uint32_t sB = (uint32_t)__builtin_amdgcn_readlane((int)sv_slot, 32);
    st.add(S_ARCS, (u64)(dA + dB));
    st.add(S_SEEN_READ, (u64)((sA != SLOT_NONE ? 1 : 0) + (kB >= 0 && sB != SLOT_NONE ? 1 : 0)));
    u64x2 acc = {0, 0};
    // (a complete line of a top in-neighbour: its words are the target, gathered from nobody)
    if (on && ee && ((sv_raw >> LD_SHIFT >> (lw >> 3)) & 1u)) acc = want;
    const u64x2 lack = want & ~acc;
    bool live = on && (!ee || (lack.x | lack.y) != 0ull);   // this lane's words still miss messages
    u64 rows = 0, pieces = 0;
    for (int k0 = 0; k0 < max(dA, dB); k0 += GP_GPAIR_RIF) {
      const u64 lb = __ballot(live);
      if (lb == 0ull) break;
      // one branch for the batch: a lane past its receiver's last arc loads
      // that last row again (same line, already requested: no HBM bytes),
      // which keeps the RIF loads unconditional inside it
      if (live && k0 < deg) {
        u64x2 r[GP_GPAIR_RIF];
#pragma unroll
        for (int q = 0; q < GP_GPAIR_RIF; ++q) r[q] = load_piece<W>(a.rows, L.idx[32 * h + min(k0 + q, deg - 1)], lw);
#pragma unroll
        for (int q = 0; q < GP_GPAIR_RIF; ++q) acc |= r[q];
      }
#pragma unroll
      for (int q = 0; q < GP_GPAIR_RIF; ++q) pieces += line_pieces<W>(__ballot(live && k0 + q < deg));
      if (lb & 0xFFFFFFFFull) rows += (u64)min(GP_GPAIR_RIF, max(dA - k0, 0));
      if (lb >> 32) rows += (u64)min(GP_GPAIR_RIF, max(dB - k0, 0));
      if (ee) {
        const u64x2 miss = want & ~acc;
        live = live && (miss.x | miss.y) != 0ull;
      }
    }
    st.add(S_GATHERED, rows);
    st.add(S_ROW_BYTES, pieces * 16ull);
    // a half whose rows covered its whole target: the receiver completes its
    // component (alias rounds: it commits SLOT_CMASK) or, under liveness,
    // holds every alive message it lacked (sated)
    const u64x2 rem = want & ~acc;
    const u64 rb = __ballot(on && (rem.x | rem.y) != 0ull);
    const bool full = ((rb >> (32 * h)) & 0xFFFFFFFFull) == 0ull;
    if constexpr (ALIVE) {
      if (a.sate && ee && a.alive) {
        if (!(rb & 0xFFFFFFFFull)) sat |= 1ull << kA;
        if (kB >= 0 && !(rb >> 32)) sat |= 1ull << kB;
      }
    }
    wave_sync_lds();   // (the next pair's column ids overwrite L.idx)
    const u64x2 sv = {L.seen[64 * h + 2 * lw], L.seen[64 * h + 2 * lw + 1]};
    pair_finish<W, true>(a, L, h, lw, on, ks, kB, base + ks, v, acc, sv, st, ALIAS && a.alias != 0 && ee && full);
  }
  return sat;
}

}  // namespace gp
