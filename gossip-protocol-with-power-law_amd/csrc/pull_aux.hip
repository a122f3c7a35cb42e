// pull_aux.hip -- the helper passes around a pull round: line masks of the
// senders (k_mklm), the per-arc activity mask (k_arcmask), aliased
// Message-Lists back to rows (k_unalias), stale rows of an unfiltered round
// (k_fixup_rows), parking of crashed vertices' rows (k_park), the big vertices'
// complete lines (k_line_done); their launchers.
#include "gp_device.h"

namespace gp {

// line masks of this round's senders (SCAN_LINES, W = 64): lm[v] = the 128-B
// lines of v's row in `rows` that hold a nonzero word, 0 for non-senders.  A
// wave takes 64 vertices; their senders' rows are read two per
// wave-instruction (a half-wave per row, 8 lanes per line), 4 instructions in
// flight; the 64 bytes are stored at once
__global__ __launch_bounds__(BLOCK) void k_mklm(const uint32_t* __restrict__ fpop, const u64* __restrict__ rows,
                                                int64_t n, uint8_t* __restrict__ lm, u64* __restrict__ partial) {
  const int lane = threadIdx.x & 63, h = lane >> 5, lw = lane & 31;
  __shared__ uint8_t s_lm[WAVES][64];
  uint8_t* out = s_lm[threadIdx.x >> 6];
  WaveStats st;
  ws_zero(st);
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t v0 = (int64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63); v0 < n; v0 += stride) {
    const int64_t v = v0 + lane;
    u64 m = __ballot(v < n && fpop[v] != 0u);
    st.add(S_LM_ROWS, (u64)__popcll(m));
    out[lane] = 0;
    wave_sync_lds();
    while (m) {
      int k[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {   // 4 pairs: rows k[2p] (half 0), k[2p + 1] (half 1)
        k[q] = -1;
        if (m) {
          k[q] = __ffsll((long long)m) - 1;
          m &= m - 1;
        }
      }
      u64x2 r[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int kk = h ? k[2 * p + 1] : k[2 * p];
        r[p] = kk >= 0 ? load_piece<64>(rows, (int)(v0 + kk), lw) : u64x2{0, 0};
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const u64 b = __ballot((r[p].x | r[p].y) != 0ull);
        const int kk = h ? k[2 * p + 1] : k[2 * p];
        if (lw == 0 && kk >= 0) {
          const uint32_t hb = (uint32_t)(b >> (32 * h));
          uint8_t l = 0;
#pragma unroll
          for (int t = 0; t < 4; ++t) l |= ((hb >> (8 * t)) & 0xFFu) ? (uint8_t)(1u << t) : (uint8_t)0;
          out[kk] = l ? l : (uint8_t)0x0F;   // (a sender whose row reads zero: load it whole)
        }
      }
    }
    wave_sync_lds();
    {   // (v0 is a multiple of 64: whole bytes per wave)
      if (lane < 32 && v0 + 2 * lane < n)
        lm[(v0 >> 1) + lane] = (uint8_t)(out[2 * lane] | (out[2 * lane + 1] << 4));
    }
    wave_sync_lds();
  }
  flush_stats(st, partial);
}

// per-arc activity mask of a filtered pull round: bit j of
// amask[k] says whether sender gcol[64k + j] is active.  Probing here, with
// no row stream evicting it, keeps the 2 MB activity bitmap L2-resident; the
// pull then skips inactive arcs, and vertices without an active in-arc,
// without loading their column ids.  AM_WORDS mask words per wave, over the
// mask words [kbeg, kbeg + grid) covering the owned vertices' arcs.
constexpr int AM_WORDS = 4;
__global__ __launch_bounds__(BLOCK) void k_arcmask(const int32_t* __restrict__ gcol, const u64* __restrict__ abits,
                                                   u64* __restrict__ amask, int64_t kbeg, int64_t nnz) {
  const int lane = threadIdx.x & 63;
  const int64_t k0 = kbeg + ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * AM_WORDS;
  if (k0 * 64 >= nnz) return;
  int32_t u[AM_WORDS];
#pragma unroll
  for (int q = 0; q < AM_WORDS; ++q) {
    const int64_t e = (k0 + q) * 64 + lane;
    u[q] = e < nnz ? gcol[e] : -1;
  }
  u64 w[AM_WORDS];
#pragma unroll
  for (int q = 0; q < AM_WORDS; ++q) w[q] = u[q] >= 0 ? abits[u[q] >> 6] : 0ull;
  // one writer lane per word: selecting the four ballots into lanes 0-3 and
  // storing from there (one dwordx2 store per wave) produced wrong words for
  // the third ballot on gfx950, a few per 10^5
#pragma unroll
  for (int q = 0; q < AM_WORDS; ++q) {
    const u64 m = __ballot(u[q] >= 0 && ((w[q] >> (u[q] & 63)) & 1ull));
    if (lane == 0 && (k0 + q) * 64 < nnz) amask[k0 + q] = m;
  }
}

// Materialize aliased Message-Lists (SLOT_CMASK): write the
// component row of every aliased vertex (with abits: of this round's senders
// only, before a push round reads them -- the 2 MB activity bitmap first, the
// slot bytes of its set bits only) into S[cur] and point sp there.  One wave
// per 64 vertices, a row per aliased vertex in one coalesced store.
__global__ __launch_bounds__(BLOCK) void k_unalias(uint8_t* __restrict__ sp, uint8_t* __restrict__ ws,
                                                   const u64* __restrict__ abits, const int32_t* __restrict__ midx,
                                                   const u64* __restrict__ cmask, u64* __restrict__ rows,
                                                   int32_t cur, int64_t n, int32_t W) {
  const int lane = threadIdx.x & 63;
  for (int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w * 64 < n; w += (int64_t)gridDim.x * WAVES) {
    const int64_t v = w * 64 + lane;
    const u64 sel = abits ? abits[w] : ~0ull;
    if (sel == 0ull) continue;
    const bool al = v < n && ((sel >> lane) & 1ull) && sp[v] == SLOT_CMASK;
    u64 todo = __ballot(al);
    if (al) {
      sp[v] = (uint8_t)cur;
      ws[v] |= (uint8_t)(1u << cur);
    }
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int64_t u = w * 64 + b;
      const int32_t k = midx[u];
      if (lane < W) rows[(size_t)u * W + lane] = cmask[(size_t)k * W + lane];
    }
  }
}

int unalias(Ctx* c, bool senders_only) {
  if (!c->carry.alias_active) return 0;
  hipLaunchKernelGGL(k_unalias, dim3(std::min(grid_for((c->n_alloc + 63) / 64, WAVES), c->cu_count * 8 * GS)),
                     dim3(BLOCK), 0, c->stream, c->d_sp, c->d_ws, senders_only ? c->d_abits : nullptr,
                     c->d_midx, c->d_cmask, c->d_slot[c->cur], c->cur, c->n_alloc, c->words);
  GP_HIP(hipGetLastError());
  if (!senders_only) c->carry.alias_active = false;
  return 0;
}

// unfiltered rounds: every in-neighbour row of S[r & 1] is
// read, so each must be a subset of its vertex's Message-List -- true for
// every row written this run (seen rows only grow).  Rows of inactive vertices
// whose slot was not written this run hold data of an earlier run: zero them.
// One wave per 64-vertex bitmap word; fully active words cost two loads.
// (Only without liveness: a crashed vertex may hold bits it never sent.)
template <int W>
__global__ __launch_bounds__(BLOCK) void k_fixup_rows(const u64* __restrict__ abits, uint8_t* __restrict__ ws,
                                                      u64* __restrict__ rows, int32_t rslot, int64_t n_alloc) {
  const int lane = threadIdx.x & 63;
  // grid-stride: one wave per 64 vertices as its own launch unit was wave-
  // dispatch-bound (0.39 ms at 2^26 for ~130 MB of bytes)
  for (int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w * 64 < n_alloc;
       w += (int64_t)gridDim.x * WAVES) {
    const int64_t v0 = w * 64 + lane;
    const bool stale = v0 < n_alloc && !((abits[w] >> lane) & 1ull) && !((ws[v0] >> rslot) & 1u);
    u64 todo = __ballot(stale);
    if (stale) ws[v0] |= (uint8_t)(1u << rslot);
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      if (lane < W) rows[(size_t)(w * 64 + b) * W + lane] = 0ull;
    }
  }
}

// Parking (before an unfiltered pull under liveness): a down vertex's row may
// hold bits it never sent (it crashed with them) and the unfiltered pull would
// forward them, so its row moves to slot 2 and both read-slot rows are zeroed.
// One wave per 64 vertices; rows stay parked for the rest of the run.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_park(const uint8_t* __restrict__ state, uint8_t* __restrict__ sp,
                                                u64* __restrict__ s0, u64* __restrict__ s1, u64* __restrict__ s2,
                                                int64_t n_alloc) {
  const int lane = threadIdx.x & 63;
  for (int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w * 64 < n_alloc;
       w += (int64_t)gridDim.x * WAVES) {
    const int64_t v0 = w * 64 + lane;
    uint32_t p = SLOT_NONE;
    if (v0 < n_alloc && (state[v0] & ST_DOWN)) p = sp[v0];
    const bool move = p < 2u;
    u64 todo = __ballot(move);
    if (move) sp[v0] = SLOT_PARKED;
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const uint32_t q = (uint32_t)__shfl((int)p, b);
      if (lane < W) {
        const size_t i = (size_t)(w * 64 + b) * W + lane;
        s2[i] = (q ? s1 : s0)[i];
        s0[i] = 0ull;
        s1[i] = 0ull;
      }
    }
  }
}

// Complete lines of the big vertices' Message-Lists (W = 64; DESIGN.md §3.3
// "Complete lines of a top in-neighbour"): before an early-exit pull without
// liveness, ldone[u] bit l = the 128-B line l of u's current row holds every
// message of u's component on that line, for the candidates u (line_cands.h);
// the pull's receivers probe the bytes of their first two in-neighbours.  A
// half-wave per candidate: u's current Message-List, slot[sp[u]], against the
// component row, 8 lanes per line.  The receivers gather S[r & 1][u], which
// is that row only if u received last round and else an older or zeroed one;
// the rule holds all the same by forward-once (gp_device.h, "expansion"):
// every bit of u's Message-List outside its frontier was sent to v when u
// first received it, so v already holds it, and the frontier is in the row v
// gathers -- v ends the round with all of u's line whichever row it reads.  An aliased candidate holds its whole
// component (0xF, no row read); no row, a parked row or no messages give 0.
// Every candidate's byte is rewritten by every pass, every other byte stays 0.
__global__ __launch_bounds__(BLOCK) void k_line_done(const int32_t* __restrict__ cand, int64_t ncand,
                                                     const uint8_t* __restrict__ sp, const int32_t* __restrict__ midx,
                                                     const u64* __restrict__ cmask, const u64* __restrict__ s0,
                                                     const u64* __restrict__ s1, uint8_t* __restrict__ ldone) {
  const int lane = threadIdx.x & 63, h = lane >> 5, lw = lane & 31;
  const int64_t stride = (int64_t)gridDim.x * WAVES * 2;
  for (int64_t p0 = ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * 2; p0 < ncand; p0 += stride) {
    const int64_t p = p0 + h;
    const bool on = p < ncand;
    const int32_t u = on ? cand[p] : 0;
    const uint32_t s = on ? (uint32_t)sp[u] : (uint32_t)SLOT_NONE;
    const int32_t k = on ? midx[u] : -1;
    bool covered = false;   // this lane's two words hold every message of the component
    if (s < 2u && k >= 0) {
      const u64x2 row = load_piece<64>(s ? s1 : s0, u, lw);
      const u64x2 lack = load_piece<64>(cmask, k, lw) & ~row;
      covered = (lack.x | lack.y) == 0ull;
    }
    const uint32_t hb = (uint32_t)(__ballot(covered) >> (32 * h));
    uint32_t l = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) l |= ((hb >> (8 * t)) & 0xFFu) == 0xFFu ? (1u << t) : 0u;
    if (s == SLOT_CMASK && k >= 0) l = 0xFu;
    if (on && lw == 0) ldone[u] = (uint8_t)l;
  }
}

void launch_line_done(Ctx* c) {
  if (c->n_ld_cand <= 0) return;
  hipLaunchKernelGGL(k_line_done, dim3(std::min(grid_for(c->n_ld_cand, (int64_t)WAVES * 2), c->cu_count * 8 * GS)),
                     dim3(BLOCK), 0, c->stream, c->d_ld_cand, c->n_ld_cand, c->d_sp, c->d_midx, c->d_cmask,
                     c->d_slot[0], c->d_slot[1], c->d_ldone);
}

void launch_mklm(Ctx* c, const ExpandArgs& a) {
  hipLaunchKernelGGL(k_mklm, dim3(std::max(1, std::min(grid_for(c->n_alloc, BLOCK), c->cu_count * 8 * GS))),
                     dim3(BLOCK), 0, c->stream, c->d_fpop[c->cur], a.rows, c->n_alloc, c->d_lm, a.partial);
}

void launch_arcmask(Ctx* c) {   // mask words of the owned vertices' in-arcs
  const int64_t kb = c->h_row_ptr[0] >> 6;
  const int64_t ke = (c->h_row_ptr[(size_t)c->nloc()] + 63) >> 6;
  if (ke > kb)
    hipLaunchKernelGGL(k_arcmask, dim3(grid_for(ke - kb, (int64_t)WAVES * AM_WORDS)), dim3(BLOCK), 0, c->stream,
                       c->d_gcol, c->d_abits, c->d_amask, kb, c->nnz_l);
}

template <int W>
void launch_fixup_rows_w(Ctx* c) {
  hipLaunchKernelGGL(k_fixup_rows<W>, dim3(std::min(grid_for((c->n_alloc + 63) / 64, WAVES), c->cu_count * 8 * GS)),
                     dim3(BLOCK), 0, c->stream, c->d_abits, c->d_ws, c->d_slot[c->cur], c->cur, c->n_alloc);
}

template <int W>
void launch_park_w(Ctx* c) {
  hipLaunchKernelGGL(k_park<W>, dim3(std::min(grid_for((c->n_alloc + 63) / 64, WAVES), c->cu_count * 8 * GS)),
                     dim3(BLOCK), 0, c->stream, c->d_state, c->d_sp, c->d_slot[0], c->d_slot[1], c->d_slot[2],
                     c->n_alloc);
}

template void launch_fixup_rows_w<1>(Ctx*);
template void launch_fixup_rows_w<2>(Ctx*);
template void launch_fixup_rows_w<4>(Ctx*);
template void launch_fixup_rows_w<8>(Ctx*);
template void launch_fixup_rows_w<16>(Ctx*);
template void launch_fixup_rows_w<32>(Ctx*);
template void launch_fixup_rows_w<64>(Ctx*);
template void launch_park_w<1>(Ctx*);
template void launch_park_w<2>(Ctx*);
template void launch_park_w<4>(Ctx*);
template void launch_park_w<8>(Ctx*);
template void launch_park_w<16>(Ctx*);
template void launch_park_w<32>(Ctx*);
template void launch_park_w<64>(Ctx*);

}  // namespace gp
