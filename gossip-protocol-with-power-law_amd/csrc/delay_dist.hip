// delay_dist.hip -- per-peer delay distributions: for
// every owned vertex v, over the messages k it holds, with D = 16,
//   delay_dist[v][d] = #{ k : min(first[v][k] - inject_round[k], D - 1) = d }   u16 [nloc][16]
// the receipts of delay.hip's sum and maximum, kept per delay value: the time
// column of the reference's arrival log (Peer.py:206, Peer.py:286) grouped by
// the receiving peer gives medians and tails, not a mean alone.  Columns 1 .. 14
// are exact, column 15 is "15 rounds or later", column 0 holds the injections.
//
// Like delay.hip the record has no neighbour term: round r's first receipts are
// new_r(v), the exact frontier rows d_frx[cur ^ 1] behind d_fpop[cur ^ 1] != 0
// after the expansion, each with receipt round rr = r + 1, counted now because
// k_churn zeroes the fpop of a receiver that crashes in round r + 1.
//
// k_delay_dist<W> (a table with several inject rounds) has k_delay's reading
// side: lane = (row slot q, word w), 64 / W rows per wave instruction, 64-vertex
// chunks behind one coalesced guard load and a ballot, the next chunk's guards
// in flight.  The round's window (delay_dist.h: the present inject rounds rr - 14
// .. rr - 1) comes by value in the kernel arguments; a lane turns the 8 plane
// words of its word position into the window's masks once -- w never changes --
// and holds them for the whole kernel.  Per word the window's delays are walked
// wave-uniformly: popc(x & eq) goes into the packed field of d, the remainder
// into field 15.  A lane's row share is 8 u32 of two 16-bit fields each; the W
// lanes of a row add them in a butterfly whose first three steps halve what a
// lane carries (4 + 2 + 1 exchanges instead of 8 per step), so a row of W = 64
// costs 10 exchanges.  A row's fields total <= 4096: the packed sums are exact.
// The lanes left holding a finished u32 park it in the wave's LDS rows (2 KB);
// after the chunk's rows lane = vertex adds its 32-B LDS row to the vertex's
// 32-B record row: one coalesced read-modify-write per chunk, one writer per
// vertex, no atomics, deterministic.
//
// k_delay_dist_uniform (every message of the table starts in round j -- C4, C5):
// delay_dist[v][min(r + 1 - j, 15)] += fpop_next[v] from the guard words alone.
// No row is read and the record does not make the context keep frontier rows
// (Ctx::delay_needs_rows; GP_DELAY_ROWS=1 takes the row pass all the same).
//
// Column 0 is written by no per-round pass: k_delay_dist_zero, launched by the
// reads alone, overwrites it with seenpop[v] - sum_{d >= 1} delay_dist[v][d].
// k_delay_dist_bins (gp_read_delay_dist_bins only) sums the rows by degree bin
// in a per-block 32 x 16 LDS table and sends each nonzero cell to the device
// table with one 64-bit atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "delay_dist.h"
#include "gp_device.h"

namespace gp {

constexpr int DDIST_GROUP = 8;   // rows a lane loads together (as DELAY_GROUP)
constexpr int DDIST_H = 2 * DELAY_DIST_WORDS;   // u32 of a row
constexpr int DDIST_BIN_ROWS = GP_DELAY_BINS, DDIST_BIN_COLS = GP_DELAY_DIST_BINS;
static_assert(GP_DELAY_DIST_BINS == DELAY_DIST_BINS, "gossip_capi.h and delay_dist.h disagree");

// Sum a.h[] over the W lanes of a row (lanes q * W + w, w < W).  Afterwards a
// lane holds max(8 / W, 1) finished u32 in a.h[0 ..): a.h[i] is u32 base + i of
// the row.  Every lane of the wave takes part
template <int W, int S, int N>
__device__ __forceinline__ void dist_row_reduce_step(DistRow& a, int w, int& base) {
  if constexpr ((1 << S) < W) {
    if constexpr (N > 1) {
      // halve: a lane with bit S of w clear keeps the lower half of what it
      // carries and gives the upper half away
      constexpr int H = N / 2;
      const bool up = (w >> S) & 1;
#pragma unroll
      for (int i = 0; i < H; ++i) {
        const uint32_t keep = up ? a.h[i + H] : a.h[i];
        const uint32_t give = up ? a.h[i] : a.h[i + H];
        a.h[i] = keep + (uint32_t)__shfl_xor((int)give, 1 << S);
      }
      base += up ? H : 0;
      dist_row_reduce_step<W, S + 1, H>(a, w, base);
    } else {
      a.h[0] += (uint32_t)__shfl_xor((int)a.h[0], 1 << S);
      dist_row_reduce_step<W, S + 1, 1>(a, w, base);
    }
  }
}

template <int W>
__device__ __forceinline__ void dist_row_reduce(DistRow& a, int w, int& base) {
  base = 0;
  dist_row_reduce_step<W, 0, DDIST_H>(a, w, base);
}

template <int W>
__global__ __launch_bounds__(BLOCK) void k_delay_dist(const u64* __restrict__ rows, const uint32_t* __restrict__ guard,
                                                      const u64* __restrict__ planes, int64_t count, uint32_t rr,
                                                      DelayWindow win, uint16_t* __restrict__ dist) {
  static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W: a power of two up to 64");
  constexpr int RPI = 64 / W;                            // rows per wave instruction
  constexpr int K = W < DDIST_GROUP ? W : DDIST_GROUP;   // rows a lane loads together
  constexpr int G = W / K;                               // such groups per 64-vertex chunk
  constexpr int HOLD = W >= DDIST_H ? 1 : DDIST_H / W;   // finished u32 a lane holds after the reduction
  __shared__ __attribute__((aligned(16))) uint32_t lres[WAVES][64 * DDIST_H];   // per wave: the chunk's 64 packed rows
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int w = lane % W, q = lane / W;
  uint32_t* res = lres[wib];
  const int64_t chunks = (count + 63) >> 6;
  const int64_t nw = (int64_t)gridDim.x * WAVES;
  const int64_t wid = (int64_t)blockIdx.x * WAVES + wib;
  const int64_t per = (chunks + nw - 1) / nw;
  const int64_t c0 = std::min(chunks, wid * per), c1 = std::min(chunks, c0 + per);
  if (c0 >= c1) return;

  const uint32_t dmask = win.dmask;
  uint64_t eq[DELAY_DIST_WINDOW];   // the window's masks of word w
  {
    uint64_t p[DELAY_PLANES];
#pragma unroll
    for (int b = 0; b < DELAY_PLANES; ++b) p[b] = planes[b * W + w];
    dist_eq_masks(p, rr, dmask, eq);
  }

  auto guard_at = [&](int64_t c) -> uint32_t {
    const int64_t v = c * 64 + lane;
    return (c < c1 && v < count) ? guard[v] : 0u;
  };

  uint32_t gnext = guard_at(c0);
  for (int64_t c = c0; c < c1; ++c) {
    const uint32_t gcur = gnext;            // |new_r(v)| of vertex c * 64 + lane
    const u64 gm = __ballot(gcur != 0u);    // receivers of the chunk (bits past count are 0)
    gnext = guard_at(c + 1);                // in flight with this chunk's rows
    if (gm == 0ull) continue;
    const int64_t v0 = c * 64;
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      // vertices [g * K * RPI, (g + 1) * K * RPI) of the chunk: wave-uniform test
      constexpr int SPAN = K * RPI;
      const u64 gs = SPAN == 64 ? gm : (gm >> (g * SPAN)) & ((1ull << (SPAN & 63)) - 1ull);
      if (gs == 0ull) continue;
      uint64_t x[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = (g * K + k) * RPI + q;   // < 64
        x[k] = ((gm >> j) & 1ull) ? rows[(v0 + j) * W + w] : 0ull;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        // the RPI vertices of this instruction: wave-uniform test
        const u64 gk = RPI == 64 ? gs : (gs >> (k * RPI)) & ((1ull << (RPI & 63)) - 1ull);
        if (gk == 0ull) continue;
        const int j = (g * K + k) * RPI + q;
        DistRow acc{};
        dist_word(x[k], eq, dmask, acc);
        int base;
        dist_row_reduce<W>(acc, w, base);
        // (with W > 8 the lanes w and w + 8 hold the same finished u32: one of them parks it)
        if (w < DDIST_H && ((gm >> j) & 1ull)) {
#pragma unroll
          for (int i = 0; i < HOLD; ++i) res[j * DDIST_H + base + i] = acc.h[i];
        }
      }
    }
    // the chunk's 64 vertices commit together, lane = vertex: each adds its
    // packed LDS row to its 32-B record row -- no field carries (delay_dist.h)
    wave_sync_lds();
    if (gcur != 0u) {
      const uint4* l = reinterpret_cast<const uint4*>(res + lane * DDIST_H);
      uint4* d = reinterpret_cast<uint4*>(dist + (v0 + lane) * DELAY_DIST_BINS);
      const uint4 a0 = l[0], a1 = l[1];
      uint4 b0 = d[0], b1 = d[1];
      b0.x += a0.x; b0.y += a0.y; b0.z += a0.z; b0.w += a0.w;
      b1.x += a1.x; b1.y += a1.y; b1.z += a1.z; b1.w += a1.w;
      d[0] = b0;
      d[1] = b1;
    }
    wave_sync_lds();   // (the next chunk overwrites the rows)
  }
}

// every message of the table starts in one round: round r's receipts all have
// the delay r + 1 - j; d = min of that and 15, >= 1
__global__ __launch_bounds__(BLOCK) void k_delay_dist_uniform(const uint32_t* __restrict__ guard, int64_t count,
                                                              uint32_t d, uint16_t* __restrict__ dist) {
  for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < count; v += (int64_t)gridDim.x * BLOCK) {
    const uint32_t tot = guard[v];
    if (tot) dist[v * DELAY_DIST_BINS + d] += (uint16_t)tot;
  }
}

// column 0 = seenpop - the receipts of the other columns (overwritten: idempotent)
__global__ __launch_bounds__(BLOCK) void k_delay_dist_zero(const uint32_t* __restrict__ seenpop, int64_t count,
                                                           uint16_t* __restrict__ dist) {
  for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < count; v += (int64_t)gridDim.x * BLOCK) {
    const uint4* d = reinterpret_cast<const uint4*>(dist + v * DELAY_DIST_BINS);
    const uint4 a = d[0], b = d[1];
    const uint32_t h[DDIST_H] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t later = h[0] >> 16;
#pragma unroll
    for (int i = 1; i < DDIST_H; ++i) later += (h[i] & 0xFFFFu) + (h[i] >> 16);
    dist[v * DELAY_DIST_BINS] = (uint16_t)(seenpop[v] - later);
  }
}

// out[b][d]: sum of delay_dist[v][d] over the vertices of [0, count) with
// delay_bin(in-degree) = b.  thread = one cell of the record
__global__ __launch_bounds__(BLOCK) void k_delay_dist_bins(const int64_t* __restrict__ row_ptr,
                                                           const uint16_t* __restrict__ dist, int64_t count,
                                                           u64* __restrict__ out) {
  constexpr int CELLS = DDIST_BIN_ROWS * DDIST_BIN_COLS;
  __shared__ u64 tb[CELLS];
  for (int t = threadIdx.x; t < CELLS; t += BLOCK) tb[t] = 0ull;
  __syncthreads();
  const int64_t cells = count * DELAY_DIST_BINS;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * BLOCK) {
    const uint32_t x = dist[i];
    if (!x) continue;
    const int64_t v = i / DELAY_DIST_BINS;
    const int bin = std::min(delay_bin(row_ptr[v + 1] - row_ptr[v]), DDIST_BIN_ROWS - 1);   // (the clamp only guards LDS)
    atomicAdd(&tb[bin * DDIST_BIN_COLS + (int)(i % DELAY_DIST_BINS)], (u64)x);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < CELLS; t += BLOCK) {
    const u64 x = tb[t];
    if (x) atomicAdd(&out[t], x);
  }
}

static void delay_dist_free(Ctx* c) {
  dfree(&c->d_ddist);
  dfree(&c->d_ddist_planes);
  dfree(&c->d_ddist_bins);
  c->ddist_rows = 0;
  record_off(c->rec[R_DELAY_DIST]);
}

// gp_reset: gp_track_delay_dist takes effect (32 B per owned vertex, the
// table's planes and presence set, the bins' device result -- or nothing),
// cleared.  As delay_reset: the array follows the owned slice, the planes and
// the presence set are the context's own table's, so a message shard gets its own
static int delay_dist_reset(Ctx* c) {
  const size_t nl = (size_t)std::max<int64_t>(c->nloc(), 1);
  if (!c->d_ddist || c->ddist_rows != nl) {
    delay_dist_free(c);
    if (dalloc(&c->d_ddist, nl * DELAY_DIST_BINS) != 0 ||
        dalloc(&c->d_ddist_bins, (size_t)DDIST_BIN_ROWS * DDIST_BIN_COLS) != 0) {
      delay_dist_free(c);
      return GP_ENOMEM;
    }
    c->ddist_rows = nl;
  }
  if ((int32_t)c->h_inj_round.size() != c->m) return set_error(GP_ESTATE, "internal: delay distributions without a message table");
  const DelayPresent present = delay_present_build(c->h_inj_round.data(), c->m);
  std::memcpy(c->ddist_present, present.w, sizeof(c->ddist_present));
  if (c->delay_by_rows()) {
    GP_TRY(record_need_rows(c, delay_dist_record, c->nloc()));
    std::vector<uint64_t> planes((size_t)DELAY_PLANES * c->words);
    delay_build_planes(c->h_inj_round.data(), c->m, c->words, planes.data());
    if (dalloc(&c->d_ddist_planes, planes.size()) != 0) {
      delay_dist_free(c);
      return GP_ENOMEM;
    }
    GP_TRY(copy_sync(c, c->d_ddist_planes, planes.data(), planes.size() * 8, hipMemcpyHostToDevice));
  } else {
    dfree(&c->d_ddist_planes);
  }
  GP_HIP(hipMemsetAsync(c->d_ddist, 0, nl * DELAY_DIST_BINS * 2, c->stream));
  return 0;
}

template <int W>
static void launch_delay_dist_w(Ctx* c, int64_t count, uint32_t rr, const DelayWindow& win) {
  // a block's 4 waves take >= 16 chunks each where there are that many (k_delay's grid)
  const int64_t grid = std::min<int64_t>(((count + 63) / 64 + WAVES * 16 - 1) / (WAVES * 16), (int64_t)c->cu_count * 8);
  hipLaunchKernelGGL((k_delay_dist<W>), dim3((unsigned)std::max<int64_t>(grid, 1)), dim3(BLOCK), 0, c->stream,
                     (const u64*)c->d_frx[c->cur ^ 1], (const uint32_t*)c->d_fpop[c->cur ^ 1],
                     (const u64*)c->d_ddist_planes, count, rr, win, c->d_ddist);
}

// after E_r: the first receipts of round r, receipt round r + 1
static int delay_dist_count_round(Ctx* c) {
  if (c->nloc() <= 0) return 0;
  const int64_t count = c->nloc();
  const uint32_t rr = (uint32_t)c->round + 1u;
  if (!c->delay_by_rows()) {
    if (c->round < c->delay_uniform) return 0;   // (no message exists yet)
    const uint32_t d = std::min<uint32_t>(rr - (uint32_t)c->delay_uniform, DELAY_DIST_BINS - 1);
    const int grid = std::max(1, std::min(grid_for(count, BLOCK), c->cu_count * 8));
    hipLaunchKernelGGL(k_delay_dist_uniform, dim3(grid), dim3(BLOCK), 0, c->stream,
                       (const uint32_t*)c->d_fpop[c->cur ^ 1], count, d, c->d_ddist);
    GP_HIP(hipGetLastError());
    return 0;
  }
  GP_TRY(record_need_rows(c, delay_dist_record, count));
  if (!c->d_ddist_planes) return set_error(GP_ESTATE, "internal: delay distributions without inject-round planes");
  DelayPresent present;
  std::memcpy(present.w, c->ddist_present, sizeof(present.w));
  const DelayWindow win = delay_window(present, rr);
  GP_TRY(with_words(c->words, [&](auto w) { launch_delay_dist_w<w()>(c, count, rr, win); }));
  GP_HIP(hipGetLastError());
  return 0;
}

// (as delay_record: kept by a partitioned context, rows for several inject rounds only)
static bool delay_dist_frx(const Ctx* c) { return c->delay_needs_rows(); }
GP_RECORD_OPS(delay_dist_record) = {R_DELAY_DIST, "delay distributions", "gp_track_delay_dist", false, 0, nullptr,
                                     delay_dist_frx, delay_dist_reset, delay_dist_free, delay_dist_count_round, nullptr,
                                     nullptr};

// both reads start here: column 0 from the counters
static int delay_dist_column0(Ctx* c) {
  const int64_t count = c->nloc();
  if (count <= 0) return 0;
  const int grid = std::max(1, std::min(grid_for(count, BLOCK), c->cu_count * 8));
  hipLaunchKernelGGL(k_delay_dist_zero, dim3(grid), dim3(BLOCK), 0, c->stream, (const uint32_t*)c->d_seenpop, count,
                     c->d_ddist);
  GP_HIP(hipGetLastError());
  return 0;
}

int delay_dist_read(Ctx* c, void* host, int64_t bytes) {
  GP_TRY(record_readable(c, delay_dist_record));
  const int64_t want = c->nloc() * DELAY_DIST_BINS * 2;
  if (bytes != want) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(want));
  if (bytes == 0) return 0;
  GP_HIP(hipSetDevice(c->device));
  GP_TRY(delay_dist_column0(c));
  return copy_sync(c, host, c->d_ddist, (size_t)bytes, hipMemcpyDeviceToHost);
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_track_delay_dist(gp_ctx* c, int32_t on) { return record_track(c, delay_dist_record, on); }

int gp_read_delay_dist_bins(gp_ctx* c, uint64_t* out, int32_t bins) {
  if (!c || !out) return set_error(GP_EINVAL, "null argument");
  GP_TRY(record_readable(c, delay_dist_record));
  if (bins != DDIST_BIN_ROWS) return set_error(GP_EINVAL, "bins must be " + std::to_string(DDIST_BIN_ROWS));
  GP_HIP(hipSetDevice(c->device));
  constexpr size_t BYTES = (size_t)DDIST_BIN_ROWS * DDIST_BIN_COLS * 8;
  GP_HIP(hipMemsetAsync(c->d_ddist_bins, 0, BYTES, c->stream));
  const int64_t count = c->nloc();
  if (count > 0) {
    GP_TRY(delay_dist_column0(c));
    const int grid = std::max(1, std::min(grid_for(count * DELAY_DIST_BINS, BLOCK), c->cu_count * 8));
    hipLaunchKernelGGL(k_delay_dist_bins, dim3(grid), dim3(BLOCK), 0, c->stream, (const int64_t*)c->d_row_ptr,
                       (const uint16_t*)c->d_ddist, count, c->d_ddist_bins);
    GP_HIP(hipGetLastError());
  }
  return copy_sync(c, out, c->d_ddist_bins, BYTES, hipMemcpyDeviceToHost);
}

}  // extern "C"
