// lossy_scan.h -- what the kernels that read frontier rows through the loss
// draw share (lossy.hip, repair.hip): the round's arguments beside ExpandArgs
// and the scan of one receiver's in-list.
#pragma once
#include "gp_device.h"
#include "link_loss.h"

namespace gp {

// one lossy round's arguments beside the pull's block (ExpandArgs stays as it
// is, so every other kernel keeps its code)
struct LossArgs {
  const u64* __restrict__ frx;   // exact frontier rows of round r, valid behind fpop[u] != 0
  LossDraw d;
};

// arcs [b, e) of receiver v's in-list: OR of the open live senders' frontier rows
template <int W>
__device__ __forceinline__ void lossy_scan(const ExpandArgs& a, const LossArgs& la, int v, int64_t b, int64_t e,
                                           WaveLds& L, int lane, int g, int lw, u64x2& acc, WaveStats& st) {
  constexpr int RPI = Geo<W>::RPI;
  constexpr int RIF = RowsInFlight<W>::value;
  for (int64_t j0 = b; j0 < e; j0 += 64) {
    const int n = (int)min((int64_t)64, e - j0);
    st.add(S_ARCS, n);
    int32_t ent = -1;
    if (lane < n && !la.d.closed) {
      const int32_t u = a.col[j0 + lane];
      // (a crash zeroes fpop before k_mkbits: a down vertex is no sender)
      if (((a.abits[u >> 6] >> (u & 63)) & 1ull) && arc_open(la.d.key, (uint32_t)(a.vbegin + u), (uint32_t)(a.vbegin + v), la.d.thresh)) ent = u;
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
        if (k < cnt) r[q] = load_piece<W>(la.frx, L.idx[k], lw);
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

// lossy.hip: k_hub_lossy over the hub table (nothing without hub items)
template <int W> void launch_hub_lossy_w(Ctx* c, const ExpandArgs& a, const LossArgs& la);

}  // namespace gp
