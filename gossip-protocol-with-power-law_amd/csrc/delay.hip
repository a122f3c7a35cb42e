// delay.hip -- per-peer receipt delays: for every owned
// vertex v, over the messages k it holds,
//   delay_sum[v] = sum (first[v][k] - inject_round[k])     u32
//   delay_max[v] = max (first[v][k] - inject_round[k])     u8
// the latency a reader takes from the reference's arrival log, where each line
// carries its time (Peer.py:206, Peer.py:286), grouped by the receiving peer.
// In the round-synchronous model a delay is the receiver's hop distance from
// the origin on the live overlay, so with GP_SEENPOP the mean is a sampled
// closeness and the maximum a sampled eccentricity.
//
// The record has no neighbour term.  Round r's first receipts are new_r(v):
// the exact frontier rows d_frx[cur ^ 1] behind d_fpop[cur ^ 1] != 0 after the
// expansion, k_curve's argument, counted now because k_churn zeroes the fpop of
// a receiver that crashes in round r + 1 and its receipts happened (§2.2).
// Each has receipt round r + 1.  An injection has delay 0 and adds nothing.
//
// k_delay<W> (a table with several inject rounds): lane = (row slot q, word
// w), 64 / W rows per wave instruction.  A wave walks 64-vertex chunks of its
// range: one coalesced load of the 64 guard words, a ballot, and nothing else
// when no vertex of the chunk received.  Otherwise a lane loads its word of up
// to DELAY_GROUP receivers' rows together and takes the sum and the minimum of
// the inject rounds of each word's bits from the 8 inject-round planes of its
// word position (delay_planes.h), which it holds in 16 registers for the whole
// kernel -- w never changes, so neither LDS nor a constant bank is touched per
// row.  The two are reduced over the W lanes of the row, and the row's lane 0
// parks them in the wave's LDS row (256 B); after the chunk's rows lane = vertex
// does delay_sum[v] += (r + 1) * |new_r(v)| - sum and delay_max[v] = max(...,
// r + 1 - min) for the chunk's 64 vertices at once: one coalesced
// read-modify-write per chunk instead of a dependent scattered one per row, one
// writer per vertex, no atomics, deterministic.
//
// k_delay_uniform (every message of the table starts in round j -- C4, C5):
// delay_sum[v] += (r + 1 - j) * fpop_next[v] and delay_max[v] = r + 1 - j from
// the guard words alone.  No row is read, and the record does not make the
// context keep frontier rows (Ctx::delay_needs_rows; GP_DELAY_ROWS=1 at
// gp_create takes the row pass all the same, the lever of the A/B).  It relies on
// d_fpop[cur ^ 1][v] being exactly |new_r(v)| on every commit path: finish_row
// and commit_vertices (gp_device.h) store the popcount of acc & ~seen, the
// non-receivers of a pull store 0, a push or list round clears the array first
// (driver.hip launch_expand).
//
// k_delay_bins (gp_read_delay_bins only, never in a round): the record by
// degree bin, one pass over row_ptr, seenpop and the two arrays; a wave reduces
// the lanes of each bin it meets and books them into the block's 32 x 5 LDS
// table, which goes to the device table with one atomic per nonzero cell.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "delay_planes.h"
#include "gp_device.h"

namespace gp {

constexpr int DELAY_GROUP = 8;   // rows a lane loads together (as CURVE_GROUP)
constexpr int DELAY_BIN_ROWS = GP_DELAY_BINS, DELAY_BIN_COLS = GP_DELAY_COLS;

template <int LPR>
__device__ __forceinline__ uint32_t group_min(uint32_t x) {
#pragma unroll
  for (int s = 1; s < LPR; s <<= 1) x = min(x, (uint32_t)__shfl_xor((int)x, s));
  return x;
}

template <int W>
__global__ __launch_bounds__(BLOCK) void k_delay(const u64* __restrict__ rows, const uint32_t* __restrict__ guard,
                                                 const u64* __restrict__ planes, int64_t count, uint32_t rr,
                                                 uint32_t* __restrict__ dsum, uint8_t* __restrict__ dmax) {
  static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W: a power of two up to 64");
  constexpr int RPI = 64 / W;                            // rows per wave instruction
  constexpr int K = W < DELAY_GROUP ? W : DELAY_GROUP;   // rows a lane loads together
  constexpr int G = W / K;                               // such groups per 64-vertex chunk
  __shared__ uint32_t lres[WAVES][64];   // per wave: inject sum << 8 | inject minimum of the chunk's vertices
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int w = lane % W, q = lane / W;
  uint32_t* res = lres[wib];
  const int64_t chunks = (count + 63) >> 6;
  const int64_t nw = (int64_t)gridDim.x * WAVES;
  const int64_t wid = (int64_t)blockIdx.x * WAVES + wib;
  const int64_t per = (chunks + nw - 1) / nw;
  const int64_t c0 = std::min(chunks, wid * per), c1 = std::min(chunks, c0 + per);
  if (c0 >= c1) return;

  uint64_t p[DELAY_PLANES];   // the planes of word w
#pragma unroll
  for (int b = 0; b < DELAY_PLANES; ++b) p[b] = planes[b * W + w];

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
        const uint32_t inj = group_sum<W>(delay_inject_sum(x[k], p));
        const uint32_t mn = group_min<W>(delay_inject_min(x[k], p));
        // inj < 2^21 and, for a receiver, mn <= 253: one word of the wave's LDS row
        if (w == 0 && ((gm >> j) & 1ull)) res[j] = inj << 8 | (mn & 0xFFu);
      }
    }
    // the chunk's 64 vertices commit together, lane = vertex: one coalesced
    // read-modify-write instead of a dependent scattered one per row
    wave_sync_lds();
    if (gcur != 0u) {
      const int64_t v = v0 + lane;
      const uint32_t r = res[lane];
      dsum[v] += rr * gcur - (r >> 8);
      const uint32_t d = rr - (r & 0xFFu);
      if (d > (uint32_t)dmax[v]) dmax[v] = (uint8_t)d;
    }
    wave_sync_lds();   // (the next chunk overwrites the row)
  }
}

// every message of the table starts in one round: the delay of round r's
// receipts is d = r + 1 - j for all of them (d >= 1: the later receipts are the
// later ones, so the maximum is a plain store)
__global__ __launch_bounds__(BLOCK) void k_delay_uniform(const uint32_t* __restrict__ guard, int64_t count, uint32_t d,
                                                         uint32_t* __restrict__ dsum, uint8_t* __restrict__ dmax) {
  for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < count; v += (int64_t)gridDim.x * BLOCK) {
    const uint32_t tot = guard[v];
    if (tot) {
      dsum[v] += d * tot;
      dmax[v] = (uint8_t)d;
    }
  }
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, s));
  return x;
}

// out[b][0..4]: peers, peers reached, receipts, sum delay_sum, max delay_max of
// the vertices of [0, count) with delay_bin(in-degree) = b
__global__ __launch_bounds__(BLOCK) void k_delay_bins(const int64_t* __restrict__ row_ptr,
                                                      const uint32_t* __restrict__ seenpop,
                                                      const uint32_t* __restrict__ dsum,
                                                      const uint8_t* __restrict__ dmax, int64_t count,
                                                      u64* __restrict__ out) {
  constexpr int CELLS = DELAY_BIN_ROWS * DELAY_BIN_COLS;
  __shared__ u64 tb[CELLS];
  for (int t = threadIdx.x; t < CELLS; t += BLOCK) tb[t] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t chunks = (count + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); c < chunks; c += (int64_t)gridDim.x * WAVES) {
    const int64_t v = c * 64 + lane;
    const bool in = v < count;
    int bin = -1;
    uint32_t sp = 0, ds = 0, dm = 0;
    if (in) {
      bin = std::min(delay_bin(row_ptr[v + 1] - row_ptr[v]), DELAY_BIN_ROWS - 1);   // (a degree is < 2^31: the clamp only guards LDS)
      sp = seenpop[v];
      ds = dsum[v];
      dm = dmax[v];
    }
    u64 todo = __ballot(in);
    while (todo) {   // one pass per bin the wave's vertices fall into
      const int b = __shfl(bin, __ffsll((long long)todo) - 1);
      const bool mine = bin == b;
      const u64 mm = __ballot(mine);
      const u64 reached = __ballot(mine && sp != 0u);
      // u32: 64 vertices x 4096 messages = 2^18 receipts, 64 x delay_sum < 2^27
      const uint32_t rec = wave_sum_u32(mine ? sp : 0u);
      const uint32_t sum = wave_sum_u32(mine ? ds : 0u);
      const uint32_t mx = wave_max_u32(mine ? dm : 0u);
      if (lane == 0) {
        u64* cell = tb + b * DELAY_BIN_COLS;
        atomicAdd(&cell[0], (u64)__popcll(mm));
        if (reached) atomicAdd(&cell[1], (u64)__popcll(reached));
        if (rec) atomicAdd(&cell[2], (u64)rec);
        if (sum) atomicAdd(&cell[3], (u64)sum);
        if (mx) atomicMax(&cell[4], (u64)mx);
      }
      todo &= ~mm;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < CELLS; t += BLOCK) {
    const u64 x = tb[t];
    if (!x) continue;
    if (t % DELAY_BIN_COLS == DELAY_BIN_COLS - 1) atomicMax(&out[t], x);
    else atomicAdd(&out[t], x);
  }
}

// Test and measurement lever: GP_DELAY_ROWS=1 at gp_create takes the row pass
// (and keeps the frontier rows) for a table with one inject round too, so both
// paths can be compared on the same run
bool delay_env_rows() {
  const char* e = getenv("GP_DELAY_ROWS");
  return e && e[0] == '1';
}

static void delay_free(Ctx* c) {
  dfree(&c->d_delay_sum);
  dfree(&c->d_delay_max);
  dfree(&c->d_delay_planes);
  dfree(&c->d_delay_bins);
  c->delay_rows = 0;
  record_off(c->rec[R_DELAY]);
}

// gp_reset: gp_track_delay takes effect (u32 and u8 per owned vertex, the
// table's planes, the bins' device result -- or nothing), cleared.  The arrays
// follow the owned slice, so another overlay or partition re-sizes them; the
// planes are rebuilt from the context's own table, so a message shard gets its
// own.  The frontier rows of the general path are alloc_state's (setup.hip)
static int delay_reset(Ctx* c) {
  const size_t nl = (size_t)std::max<int64_t>(c->nloc(), 1);
  if (!c->d_delay_sum || c->delay_rows != nl) {
    delay_free(c);
    if (dalloc(&c->d_delay_sum, nl) != 0 || dalloc(&c->d_delay_max, nl) != 0 ||
        dalloc(&c->d_delay_bins, (size_t)DELAY_BIN_ROWS * DELAY_BIN_COLS) != 0) {
      delay_free(c);
      return GP_ENOMEM;
    }
    c->delay_rows = nl;
  }
  if ((int32_t)c->h_inj_round.size() != c->m) return set_error(GP_ESTATE, "internal: receipt delays without a message table");
  if (c->delay_by_rows()) {
    GP_TRY(record_need_rows(c, delay_record, c->nloc()));
    std::vector<uint64_t> planes((size_t)DELAY_PLANES * c->words);
    delay_build_planes(c->h_inj_round.data(), c->m, c->words, planes.data());
    if (dalloc(&c->d_delay_planes, planes.size()) != 0) {
      delay_free(c);
      return GP_ENOMEM;
    }
    GP_TRY(copy_sync(c, c->d_delay_planes, planes.data(), planes.size() * 8, hipMemcpyHostToDevice));
  } else {
    dfree(&c->d_delay_planes);
  }
  GP_HIP(hipMemsetAsync(c->d_delay_sum, 0, nl * 4, c->stream));
  GP_HIP(hipMemsetAsync(c->d_delay_max, 0, nl, c->stream));
  return 0;
}

template <int W>
static void launch_delay_w(Ctx* c, int64_t count, uint32_t rr) {
  // a block's 4 waves take >= 16 chunks each where there are that many (k_curve's grid)
  const int64_t grid = std::min<int64_t>(((count + 63) / 64 + WAVES * 16 - 1) / (WAVES * 16), (int64_t)c->cu_count * 8);
  hipLaunchKernelGGL((k_delay<W>), dim3((unsigned)std::max<int64_t>(grid, 1)), dim3(BLOCK), 0, c->stream,
                     (const u64*)c->d_frx[c->cur ^ 1], (const uint32_t*)c->d_fpop[c->cur ^ 1],
                     (const u64*)c->d_delay_planes, count, rr, c->d_delay_sum, c->d_delay_max);
}

// after E_r: the first receipts of round r, receipt round r + 1
static int delay_count_round(Ctx* c) {
  if (c->nloc() <= 0) return 0;
  const int64_t count = c->nloc();
  const uint32_t rr = (uint32_t)c->round + 1u;
  if (!c->delay_by_rows()) {
    if (c->round < c->delay_uniform) return 0;   // (no message exists yet)
    const int grid = std::max(1, std::min(grid_for(count, BLOCK), c->cu_count * 8));
    hipLaunchKernelGGL(k_delay_uniform, dim3(grid), dim3(BLOCK), 0, c->stream, (const uint32_t*)c->d_fpop[c->cur ^ 1],
                       count, rr - (uint32_t)c->delay_uniform, c->d_delay_sum, c->d_delay_max);
    GP_HIP(hipGetLastError());
    return 0;
  }
  GP_TRY(record_need_rows(c, delay_record, count));
  if (!c->d_delay_planes) return set_error(GP_ESTATE, "internal: receipt delays without inject-round planes");
  GP_TRY(with_words(c->words, [&](auto w) { launch_delay_w<w()>(c, count, rr); }));
  GP_HIP(hipGetLastError());
  return 0;
}

// (a partitioned context keeps it for its owned slice; the rows only for a
// table of several inject rounds)
static bool delay_frx(const Ctx* c) { return c->delay_needs_rows(); }
GP_RECORD_OPS(delay_record) = {R_DELAY, "receipt delays", "gp_track_delay", false, 0, nullptr, delay_frx, delay_reset,
                                delay_free, delay_count_round, nullptr, nullptr};

int delay_read(Ctx* c, int32_t what, void* host, int64_t bytes) {
  GP_TRY(record_readable(c, delay_record));
  const int64_t nl = c->nloc();
  const int64_t want = what == GP_DELAY_SUM ? nl * 4 : nl;
  if (bytes != want) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(want));
  if (bytes == 0) return 0;
  return copy_sync(c, host, what == GP_DELAY_SUM ? (const void*)c->d_delay_sum : (const void*)c->d_delay_max,
                   (size_t)bytes, hipMemcpyDeviceToHost);
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_track_delay(gp_ctx* c, int32_t on) { return record_track(c, delay_record, on); }

int gp_read_delay_bins(gp_ctx* c, uint64_t* out, int32_t bins) {
  if (!c || !out) return set_error(GP_EINVAL, "null argument");
  GP_TRY(record_readable(c, delay_record));
  if (bins != DELAY_BIN_ROWS) return set_error(GP_EINVAL, "bins must be " + std::to_string(DELAY_BIN_ROWS));
  GP_HIP(hipSetDevice(c->device));
  constexpr size_t BYTES = (size_t)DELAY_BIN_ROWS * DELAY_BIN_COLS * 8;
  GP_HIP(hipMemsetAsync(c->d_delay_bins, 0, BYTES, c->stream));
  const int64_t count = c->nloc();
  if (count > 0) {
    const int grid = std::max(1, std::min(grid_for((count + 63) / 64, WAVES), c->cu_count * 4));
    hipLaunchKernelGGL(k_delay_bins, dim3(grid), dim3(BLOCK), 0, c->stream, (const int64_t*)c->d_row_ptr,
                       (const uint32_t*)c->d_seenpop, (const uint32_t*)c->d_delay_sum,
                       (const uint8_t*)c->d_delay_max, count, c->d_delay_bins);
    GP_HIP(hipGetLastError());
  }
  return copy_sync(c, out, c->d_delay_bins, BYTES, hipMemcpyDeviceToHost);
}

}  // extern "C"
