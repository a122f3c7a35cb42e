// curve.hip -- per-message spread curves: curve[r][k] = the
// number of owned vertices whose first receipt of message k has receipt round
// r, the column histograms of the first-receipt matrix without keeping the
// matrix.  It is the aggregate of what each reference peer logs per arrival
// (Peer.py:175-216: every received gossip with its time).
//
// Round r adds to two rows, on the engine stream after the expansion:
//   row r      the round's injections at up, owned origins (k_curve_inject,
//              from the inject groups k_inject applied);
//   row r + 1  the expansion's first receipts: the exact frontier rows
//              frx_next of the owned vertices with fpop_next != 0 (k_curve).
//              Counted now and not from round r + 1's frontier: k_churn zeroes
//              the fpop of a receiver that crashes in round r + 1, and its
//              receipts happened (§2.2).  Rows of the other vertices are two
//              rounds stale; the guard excludes them.
//
// k_curve: lane = (row slot q, word w), 64 / W rows per wave instruction as in
// k_bitcount.  A wave walks 64-vertex chunks of its range: one coalesced load
// of the 64 guard words, a ballot, and nothing else when no vertex of the
// chunk received (late rounds cost the guard sweep).  Otherwise every lane
// loads up to 8 receivers' words together (zero for the others) and adds them
// bit-sliced (curve_planes.h); the planes are expanded into the block's LDS
// counts when they fill or the range ends, and each nonzero column of the
// block goes to the u64 row with one atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "curve_planes.h"
#include "gp_device.h"

namespace gp {

constexpr int CURVE_ROWS = 255;   // receipt rounds 0 .. 254 (rounds stop at 253, gp_round)

template <int W>
__global__ __launch_bounds__(BLOCK) void k_curve(const u64* __restrict__ rows, const uint32_t* __restrict__ guard,
                                                 int64_t count, u64* __restrict__ out) {
  static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W: a power of two up to 64");
  constexpr int RPI = 64 / W;                      // rows per wave instruction
  constexpr int K = W < CURVE_GROUP ? W : CURVE_GROUP;   // rows a lane loads together
  constexpr int G = W / K;                         // such groups per 64-vertex chunk
  constexpr int M = W * 64;
  __shared__ uint32_t lc[M];   // [bit][word]: the lanes of one instruction hit distinct banks
  for (int t = threadIdx.x; t < M; t += BLOCK) lc[t] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int w = lane % W, q = lane / W;
  const int64_t chunks = (count + 63) >> 6;
  const int64_t nw = (int64_t)gridDim.x * WAVES;
  const int64_t wid = (int64_t)blockIdx.x * WAVES + wib;
  const int64_t per = (chunks + nw - 1) / nw;
  const int64_t c0 = std::min(chunks, wid * per), c1 = std::min(chunks, c0 + per);

  CurvePlanes p;
  int held = 0;   // rows booked into the planes (wave-uniform)
  auto flush = [&]() {
#pragma unroll 4
    for (int b = 0; b < 64; ++b) {
      const uint32_t cnt = curve_count(p, b);
      if (cnt) atomicAdd(&lc[b * W + w], cnt);
    }
    curve_clear(p);
    held = 0;
  };
  auto guard_at = [&](int64_t c) -> uint32_t {
    const int64_t v = c * 64 + lane;
    return (c < c1 && v < count) ? guard[v] : 0u;
  };

  uint32_t gnext = guard_at(c0);
  for (int64_t c = c0; c < c1; ++c) {
    const u64 gm = __ballot(gnext != 0u);   // receivers of the chunk (bits past count are 0)
    gnext = guard_at(c + 1);                // in flight with this chunk's rows
    if (gm == 0ull) continue;
    const int64_t v0 = c * 64;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      // vertices [g * K * RPI, (g + 1) * K * RPI) of the chunk: wave-uniform test
      constexpr int SPAN = K * RPI;
      const u64 gs = SPAN == 64 ? gm : (gm >> (g * SPAN)) & ((1ull << (SPAN & 63)) - 1ull);
      if (gs == 0ull) continue;
      uint64_t x[CURVE_GROUP];
#pragma unroll
      for (int k = 0; k < CURVE_GROUP; ++k) {
        x[k] = 0ull;
        if (k < K) {
          const int j = (g * K + k) * RPI + q;   // < 64
          if ((gm >> j) & 1ull) x[k] = rows[(v0 + j) * W + w];
        }
      }
      if (!curve_fits(held, CURVE_GROUP)) flush();
      curve_add8(p, x);
      held += CURVE_GROUP;
    }
  }
  if (held > 0) flush();
  __syncthreads();
  for (int t = threadIdx.x; t < M; t += BLOCK) {
    const uint32_t cnt = lc[t];
    if (cnt) atomicAdd(&out[(t % W) * 64 + t / W], (u64)cnt);
  }
}

// injections of round r: one thread per (group, word) of the round's span; the
// state test is k_inject's own (no kernel between them takes a vertex down)
__global__ void k_curve_inject(const int32_t* __restrict__ origin, const u64* __restrict__ bits,
                               const uint8_t* __restrict__ state, int64_t off, int64_t groups, int32_t words,
                               int64_t nloc, u64* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= groups * words) return;
  const int64_t gi = off + t / words;
  const int32_t w = (int32_t)(t % words);
  const int32_t o = origin[gi];
  if (o < 0 || o >= nloc || (state[o] & ST_DOWN)) return;   // owned local ids are [0, nloc)
  u64 x = bits[gi * words + w];
  while (x) {
    const int b = __ffsll((long long)x) - 1;
    x &= x - 1;
    atomicAdd(&out[w * 64 + b], 1ull);
  }
}

int curve_alloc(Ctx* c, bool on) {
  c->rec[R_CURVE].valid = false;   // (a new buffer holds no run's counts)
  c->curve_alloc = false;
  if (!on) {
    dfree(&c->d_curve);
    return 0;
  }
  // (one more row: the yardstick's scratch, curve_yardstick below)
  GP_TRY(dalloc(&c->d_curve, (size_t)(CURVE_ROWS + 1) * c->words * 64));
  c->curve_alloc = true;
  return 0;
}

// gp_reset: cleared, counted from here on.  The buffer is alloc_state's
// (curve_alloc), which gp_reset has run whenever the request changed
static int curve_reset(Ctx* c) {
  if (!c->curve_alloc || !c->d_curve) return set_error(GP_ESTATE, "internal: spread curve without its buffer");
  GP_HIP(hipMemsetAsync(c->d_curve, 0, (size_t)CURVE_ROWS * c->words * 64 * 8, c->stream));
  return 0;
}

static void curve_free(Ctx* c) {
  (void)curve_alloc(c, false);
  record_off(c->rec[R_CURVE]);
}

int curve_env_grid() {
  const char* e = getenv("GP_CURVE_GRID");
  if (!e) return 0;
  const long k = strtol(e, nullptr, 10);
  return k >= 1 && k <= (1 << 20) ? (int)k : 0;
}

template <int W>
static void launch_curve_w(Ctx* c, const u64* rows, const uint32_t* guard, int64_t count, u64* out) {
  // a block's 4 waves take >= 16 chunks each where there are that many
  int64_t grid = std::min<int64_t>(((count + 63) / 64 + WAVES * 16 - 1) / (WAVES * 16), (int64_t)c->cu_count * 8);
  if (c->curve_grid > 0) grid = std::min<int64_t>(grid, c->curve_grid);
  hipLaunchKernelGGL((k_curve<W>), dim3((unsigned)std::max<int64_t>(grid, 1)), dim3(BLOCK), 0, c->stream, rows, guard,
                     count, out);
}

static int launch_curve(Ctx* c, u64* out) {
  const int64_t count = c->nloc();
  const u64* rows = c->d_frx[c->cur ^ 1];
  const uint32_t* guard = c->d_fpop[c->cur ^ 1];
  GP_TRY(with_words(c->words, [&](auto w) { launch_curve_w<w()>(c, rows, guard, count, out); }));
  GP_HIP(hipGetLastError());
  return 0;
}

// Measurement lever (scripts/curve_cost.py): GP_CURVE_YARDSTICK=1 at gp_create
// times k_curve with events of its own and, over the same guarded rows, the
// per-bit k_bitsum<W, true, false> of driver.hip -- the only way to count them
// before k_curve -- into the scratch row; it compares the two rows and prints
// one line per round to stderr.  It synchronizes the stream: never on in a
// timed run.
bool curve_env_yardstick() {
  const char* e = getenv("GP_CURVE_YARDSTICK");
  return e && e[0] == '1';
}
static int curve_yardstick(Ctx* c, u64* out) {
  const size_t M = (size_t)c->words * 64;
  hipStream_t s = c->stream;
  u64* scratch = c->d_curve + (size_t)CURVE_ROWS * M;
  hipEvent_t ev[4] = {};
  hipError_t e = hipSuccess;   // (one exit: the events are destroyed whatever failed)
  for (auto& x : ev)
    if (e == hipSuccess) e = hipEventCreate(&x);
  if (e == hipSuccess) e = hipMemsetAsync(scratch, 0, M * 8, s);
  if (e == hipSuccess) e = hipEventRecord(ev[0], s);
  int rc = e == hipSuccess ? launch_curve(c, out) : 0;
  if (e == hipSuccess) e = hipEventRecord(ev[1], s);
  if (e == hipSuccess) e = hipEventRecord(ev[2], s);
  if (e == hipSuccess && rc == 0)
    rc = bitsum_count_rows(c, c->d_frx[c->cur ^ 1], c->d_fpop[c->cur ^ 1], c->nloc(), scratch);
  if (e == hipSuccess) e = hipEventRecord(ev[3], s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  float ms_curve = 0.f, ms_bitsum = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms_curve, ev[0], ev[1]);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms_bitsum, ev[2], ev[3]);
  for (auto& x : ev)
    if (x) (void)hipEventDestroy(x);
  GP_TRY(rc);
  GP_HIP(e);
  std::vector<u64> a(M), b(M);
  GP_TRY(copy_sync(c, a.data(), out, M * 8, hipMemcpyDeviceToHost));
  GP_TRY(copy_sync(c, b.data(), scratch, M * 8, hipMemcpyDeviceToHost));
  fprintf(stderr, "gp_curve_yardstick round=%d words=%d k_curve_ms=%.4f k_bitsum_ms=%.4f equal=%d\n", c->round,
          c->words, ms_curve, ms_bitsum, a == b ? 1 : 0);
  return 0;
}

// after E_r (and before the exchange moves on): rows r and r + 1 of the curve
static int curve_count_round(Ctx* c) {
  const int r = c->round;
  if (r + 1 >= CURVE_ROWS) return set_error(GP_ESTATE, "internal: spread curve past its last row");
  GP_TRY(record_need_rows(c, curve_record, c->nloc()));
  const size_t M = (size_t)c->words * 64;
  hipStream_t s = c->stream;
  auto it = c->inject.find(r);
  if (it != c->inject.end() && it->second.cnt > 0)
    hipLaunchKernelGGL(k_curve_inject, dim3(grid_for(it->second.cnt * c->words, 256)), dim3(256), 0, s, c->d_inj_origin,
                       c->d_inj_bits, c->d_state, it->second.off, it->second.cnt, c->words, c->nloc(),
                       c->d_curve + (size_t)r * M);
  GP_HIP(hipGetLastError());
  if (c->nloc() <= 0) return 0;
  u64* out = c->d_curve + (size_t)(r + 1) * M;
  return c->curve_yard ? curve_yardstick(c, out) : launch_curve(c, out);
}

// (kept by a partitioned context for its owned slice)
GP_RECORD_OPS(curve_record) = {R_CURVE, "spread curve", "gp_track_curve", false, 0, nullptr, nullptr, curve_reset,
                                curve_free, curve_count_round, nullptr, nullptr};

}  // namespace gp

using namespace gp;

extern "C" {

int gp_track_curve(gp_ctx* c, int32_t on) { return record_track(c, curve_record, on); }

int gp_read_curve(gp_ctx* c, int32_t job, uint64_t* host, int32_t cap_rows, int32_t* rows_out) {
  if (!c || !host || !rows_out) return set_error(GP_EINVAL, "null argument");
  if (job != 0 && job != 1) return set_error(GP_EINVAL, "job must be 0 or 1");
  GP_HIP(hipSetDevice(c->device));
  if (job == 1) {   // the job record of gp_shard_combine (shard.hip)
    if (!c->j_ready) return set_error(GP_ESTATE, "gp_shard_combine first");
    if (!c->j_curve_valid) return set_error(GP_ENOTRACK, "a rank of the job tracked no spread curve");
    if (cap_rows < c->j_curve_rows)
      return set_error(GP_EINVAL, "cap_rows < " + std::to_string(c->j_curve_rows) + " rows");
    GP_TRY(copy_sync(c, host, c->d_jcurve, (size_t)c->j_curve_rows * (size_t)c->jm * 8, hipMemcpyDeviceToHost));
    *rows_out = c->j_curve_rows;
    return 0;
  }
  GP_TRY(record_readable(c, curve_record));
  const int32_t rows = c->round + 1;
  if (cap_rows < rows) return set_error(GP_EINVAL, "cap_rows < " + std::to_string(rows) + " rows");
  GP_HIP(hipStreamSynchronize(c->stream));
  GP_HIP(hipMemcpy2D(host, (size_t)c->m * 8, c->d_curve, (size_t)c->words * 64 * 8, (size_t)c->m * 8, (size_t)rows,
                     hipMemcpyDeviceToHost));
  *rows_out = rows;
  return 0;
}

}  // extern "C"
