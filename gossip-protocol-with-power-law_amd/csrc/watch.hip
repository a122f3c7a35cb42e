// watch.hip -- watched peers: the arrival log of a
// caller-chosen list of peers v_0 .. v_{K-1}, link by link -- what every
// reference peer writes line by line (Peer.py:206, Peer.py:286 through
// Peer.log, Peer.py:40-47), kept as two byte matrices on the device at any
// scale.  With watched arc a = watch_ptr[s] + i the i-th arc of row v_s of the
// in-CSR, sender u = col[row_ptr[v_s] + i],
//
//   watch_first[s][k]   = first[v_s][k]                                     u8 [K][m]
//   watch_arrival[a][k] = r + 1  if k in frontier_r(u), v_s up in E_r       u8 [A][m]
//
// 255 = never.  Forward-once puts a message on a link at most once, so a cell
// is written at most once per run and the matrix is the whole log.
//
// The reading side is k_fresh's: after E_r, d_frx[cur] behind fpop[cur] != 0 is
// frontier_r and d_frx[cur ^ 1] behind fpop[cur ^ 1] != 0 is new_r.  The pass
// never touches the overlay's CSR: gp_reset copies the watched in-lists into
// d_watch_col / d_watch_slot (8 B per arc beside 64 W B of record).
//
// k_watch<W>: the work unit is the watched arc.  One-wave blocks, 64 arcs of
// the flat arc sequence each: one coalesced load of the sender ids, their guard
// words and the receiver's state, a ballot, and nothing else when no arc of the
// chunk is live -- a quiet round costs the guard sweep over A arcs.  The live
// arcs are compacted into LDS; their frontier rows are gathered 128 / W per
// wave instruction at 16 B per lane (Geo<W>), WATCH_RIF instructions in flight,
// and parked in LDS as bits.  The wave then walks the batch's record rows as a
// flat sequence of 16-byte pieces, lane = piece: 16 message bits from LDS, and
// where they are not zero one 16-byte read-modify-write of the record
// (watch_bytes.h).  Consecutive lanes write consecutive pieces of a row, 1 KiB
// per wave instruction on a dense row; a piece without a bit loads and stores
// nothing.  A hub's in-list spreads over blocks by itself: no hub kernel, no
// hub_threshold.  Every 16-byte piece of the record has one writing lane per
// round and rounds follow each other on the engine stream: no atomic, and the
// record is deterministic.
//
// k_watch_own<W>: the K peers' own rows, one wave per slot.  frontier_r(v_s)
// -- new_{r-1}(v_s), written with the same value the round before, and round
// r's injections at v_s when it is up -- gets r; new_r(v_s) gets r + 1, counted
// when it happens (a receiver that crashes in round r + 1 still received,
// k_delay's argument).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <unordered_set>
#include <vector>

#include "gp_device.h"
#include "watch_bytes.h"

namespace gp {

constexpr int WATCH_RIF = 4;   // frontier rows per lane in flight (k_fresh's)
constexpr int WATCH_PIF = 4;   // record pieces per lane in flight
constexpr int64_t WATCH_DEFAULT_BYTES = (int64_t)1 << 30;

struct WatchArgs {
  const int32_t* __restrict__ wcol;      // [A] sender of watched arc a
  const int32_t* __restrict__ wslot;     // [A] its receiver's slot
  const int32_t* __restrict__ wv;        // [K] the watched vertices
  const uint8_t* __restrict__ state;
  const u64* __restrict__ cur_rows;      // [n][W] frontier_r, valid where cur_guard != 0
  const uint32_t* __restrict__ cur_guard;
  const u64* __restrict__ next_rows;     // [n][W] new_r, valid where next_guard != 0
  const uint32_t* __restrict__ next_guard;
  uint8_t* __restrict__ first;           // [K][64 W]
  uint8_t* __restrict__ arrival;         // [A][64 W]
  int64_t arcs;
  int32_t peers;
  uint32_t r;                            // the round
};

// `value` into the bytes of the 16 set message bits of one 16-byte piece
__device__ __forceinline__ void watch_put16(uint8_t* __restrict__ piece, uint32_t bits16, uint32_t value) {
  u64x2* p = reinterpret_cast<u64x2*>(piece);
  u64x2 x = *p;
  uint64_t lo = x.x, hi = x.y;
  watch_merge16(lo, hi, bits16, value);
  x.x = lo;
  x.y = hi;
  *p = x;
}

template <int W>
__global__ __launch_bounds__(64) void k_watch(WatchArgs a) {
  static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W: a power of two up to 64");
  constexpr int WPL = Geo<W>::WPL, LPR = Geo<W>::LPR, RPI = Geo<W>::RPI;
  constexpr int RIF = WATCH_RIF * RPI <= 64 ? WATCH_RIF : 64 / RPI;   // a chunk has 64 arcs
  constexpr int ROWS = RIF * RPI;                                      // rows of a batch
  constexpr int PCS = 4 * W;                                           // 16-byte pieces of a record row
  __shared__ int32_t idx[64];
  __shared__ uint8_t pos[64];
  __shared__ u64 bits[ROWS * W];   // <= 4 KB
  const int lane = threadIdx.x;
  const int g = lane / LPR, lw = lane % LPR;
  const int64_t a0 = (int64_t)blockIdx.x * 64, arc = a0 + lane;
  int32_t u = -1;
  if (arc < a.arcs) {
    u = a.wcol[arc];
    if (a.cur_guard[u] == 0u || (a.state[a.wv[a.wslot[arc]]] & ST_DOWN)) u = -1;   // a stale row, or nobody to hear it
  }
  const u64 m = __ballot(u >= 0);
  if (m == 0ull) return;
  if (u >= 0) {
    const int rk = lane_rank(m);
    idx[rk] = u;
    pos[rk] = (uint8_t)lane;   // the arc is a0 + lane
  }
  wave_sync_lds();
  const int cnt = __popcll(m);
  const uint32_t value = a.r + 1u;
  const uint16_t* __restrict__ b16 = reinterpret_cast<const uint16_t*>(bits);
  for (int k0 = 0; k0 < cnt; k0 += ROWS) {
    u64x2 r[RIF];
#pragma unroll
    for (int q = 0; q < RIF; ++q) {
      const int k = k0 + g + q * RPI;
      r[q] = u64x2{0, 0};
      if (k < cnt) r[q] = load_piece<W>(a.cur_rows, idx[k], lw);
    }
#pragma unroll
    for (int q = 0; q < RIF; ++q) {
      u64* row = bits + (g + q * RPI) * W + lw * WPL;
      row[0] = r[q].x;
      if (WPL == 2) row[1] = r[q].y;
    }
    wave_sync_lds();
    // row t of the batch is record row a0 + pos[k0 + t]; its pieces are the u16
    // [t * PCS, (t + 1) * PCS) of the LDS rows (little-endian: message 16 p + b
    // is bit b of u16 p and byte b of piece p)
    const int total = std::min(ROWS, cnt - k0) * PCS;
    for (int p0 = 0; p0 < total; p0 += 64 * WATCH_PIF) {
      uint32_t bw[WATCH_PIF];
      u64x2* dst[WATCH_PIF];
      u64x2 old[WATCH_PIF];
#pragma unroll
      for (int t = 0; t < WATCH_PIF; ++t) {
        const int p = p0 + t * 64 + lane;
        bw[t] = p < total ? (uint32_t)b16[p] : 0u;
        dst[t] = nullptr;
        old[t] = u64x2{0, 0};
        if (bw[t]) {
          dst[t] = reinterpret_cast<u64x2*>(a.arrival + (size_t)(a0 + pos[k0 + p / PCS]) * (size_t)(64 * W) +
                                            (size_t)(p % PCS) * 16);
          old[t] = *dst[t];
        }
      }
#pragma unroll
      for (int t = 0; t < WATCH_PIF; ++t) {
        if (bw[t]) {
          uint64_t lo = old[t].x, hi = old[t].y;
          watch_merge16(lo, hi, bw[t], value);
          u64x2 x;
          x.x = lo;
          x.y = hi;
          *dst[t] = x;
        }
      }
    }
    wave_sync_lds();   // (the next batch overwrites the rows)
  }
}

// slot s's own row: `rows[v]` behind `guard[v] != 0` written with `value`
template <int W>
__device__ __forceinline__ void watch_own_row(const u64* __restrict__ rows, const uint32_t* __restrict__ guard,
                                              int64_t v, uint8_t* __restrict__ out, uint32_t value, int lane) {
  constexpr int PCS = 4 * W;
  if (guard[v] == 0u) return;
  const uint16_t* __restrict__ b16 = reinterpret_cast<const uint16_t*>(rows + v * W);
  for (int p = lane; p < PCS; p += 64) {
    const uint32_t bw = b16[p];
    if (bw) watch_put16(out + (size_t)p * 16, bw, value);
  }
}

template <int W>
__global__ __launch_bounds__(64) void k_watch_own(WatchArgs a) {
  const int s = blockIdx.x;
  if (s >= a.peers) return;
  const int64_t v = a.wv[s];
  uint8_t* out = a.first + (size_t)s * (size_t)(64 * W);
  watch_own_row<W>(a.cur_rows, a.cur_guard, v, out, a.r, threadIdx.x);         // frontier_r: injections of round r
  watch_own_row<W>(a.next_rows, a.next_guard, v, out, a.r + 1u, threadIdx.x);  // new_r (disjoint from it)
}

// the watched in-lists, copied out of the in-CSR once per reset
__global__ __launch_bounds__(64) void k_watch_build(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                    const int32_t* __restrict__ wv, const int64_t* __restrict__ wptr,
                                                    int32_t* __restrict__ wcol, int32_t* __restrict__ wslot) {
  const int s = blockIdx.x;
  const int64_t b = row_ptr[wv[s]], o = wptr[s], deg = wptr[s + 1] - o;
  for (int64_t i = threadIdx.x; i < deg; i += 64) {
    wcol[o + i] = col[b + i];
    wslot[o + i] = s;
  }
}

static void watch_free(Ctx* c) {
  dfree(&c->d_watch_v);
  dfree(&c->d_watch_ptr);
  dfree(&c->d_watch_col);
  dfree(&c->d_watch_slot);
  dfree(&c->d_watch_first);
  dfree(&c->d_watch_arrival);
  c->h_watch_v.clear();
  c->h_watch_ptr.clear();
  c->watch_arcs = 0;
  c->watch_words = 0;
  record_off(c->rec[R_WATCH]);
}

// a new overlay: the ids of the list are another overlay's
static void watch_forget(Ctx* c) {
  watch_free(c);
  c->h_watch_want.clear();
}

// K peers with A arcs at row width W: the two byte arrays
static int64_t watch_bytes(int64_t peers, int64_t arcs, int32_t words) { return (arcs + peers) * 64 * (int64_t)words; }

static int64_t watch_count_arcs(const Ctx* c, const std::vector<int32_t>& verts) {
  int64_t arcs = 0;
  for (int32_t v : verts) arcs += c->h_row_ptr[(size_t)v + 1] - c->h_row_ptr[(size_t)v];
  return arcs;
}

// gp_reset: gp_watch's list takes effect.  The index arrays and the record are
// (re)built for the list, the overlay and the row width of this run, the record
// filled with 0xFF; with no list nothing is allocated.  The exact frontier rows
// are alloc_state's (setup.hip: frx_rows)
static int watch_reset(Ctx* c) {
  if (c->h_row_ptr.size() != (size_t)c->n + 1) return set_error(GP_ESTATE, "internal: watched peers without the overlay's offsets");
  GP_TRY(record_need_rows(c, watch_record, c->n));
  const std::vector<int32_t>& want = c->h_watch_want;
  const int64_t K = (int64_t)want.size(), A = watch_count_arcs(c, want);
  const int64_t need = watch_bytes(K, A, c->words);
  if (need > c->watch_max_bytes) {   // (the message table grew after gp_watch checked)
    watch_free(c);
    return set_error(GP_ENOMEM, "watched peers: the record needs " + std::to_string(need) + " bytes, gp_watch allowed " +
                                    std::to_string(c->watch_max_bytes));
  }
  const bool same = c->d_watch_first && c->h_watch_v == want && c->watch_arcs == A && c->watch_words == c->words;
  const size_t row = (size_t)c->words * 64;
  if (!same) {
    watch_free(c);
    std::vector<int64_t> ptr((size_t)K + 1, 0);
    for (int64_t s = 0; s < K; ++s)
      ptr[(size_t)s + 1] = ptr[(size_t)s] + (c->h_row_ptr[(size_t)want[(size_t)s] + 1] - c->h_row_ptr[(size_t)want[(size_t)s]]);
    if (dalloc(&c->d_watch_v, (size_t)K) != 0 || dalloc(&c->d_watch_ptr, (size_t)K + 1) != 0 ||
        dalloc(&c->d_watch_col, (size_t)A) != 0 || dalloc(&c->d_watch_slot, (size_t)A) != 0 ||
        dalloc(&c->d_watch_first, (size_t)K * row) != 0 || dalloc(&c->d_watch_arrival, (size_t)A * row) != 0) {
      watch_free(c);
      return GP_ENOMEM;
    }
    GP_TRY(copy_sync(c, c->d_watch_v, want.data(), (size_t)K * 4, hipMemcpyHostToDevice));
    GP_TRY(copy_sync(c, c->d_watch_ptr, ptr.data(), ((size_t)K + 1) * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_watch_build, dim3((unsigned)K), dim3(64), 0, c->stream, (const int64_t*)c->d_row_ptr,
                       (const int32_t*)c->d_col, (const int32_t*)c->d_watch_v, (const int64_t*)c->d_watch_ptr,
                       c->d_watch_col, c->d_watch_slot);
    GP_HIP(hipGetLastError());
    c->h_watch_v = want;
    c->h_watch_ptr = ptr;
    c->watch_arcs = A;
    c->watch_words = c->words;
  }
  GP_HIP(hipMemsetAsync(c->d_watch_first, 0xFF, (size_t)K * row, c->stream));
  if (A) GP_HIP(hipMemsetAsync(c->d_watch_arrival, 0xFF, (size_t)A * row, c->stream));
  return 0;
}

template <int W>
static void launch_watch_w(Ctx* c, const WatchArgs& a) {
  hipStream_t s = c->stream;
  if (a.arcs > 0) hipLaunchKernelGGL((k_watch<W>), dim3(grid_for(a.arcs, 64)), dim3(64), 0, s, a);
  hipLaunchKernelGGL((k_watch_own<W>), dim3((unsigned)a.peers), dim3(64), 0, s, a);
}

// after E_r: round r's arrivals at the watched peers, and their own first receipts
static int watch_count_round(Ctx* c) {
  GP_TRY(record_need_rows(c, watch_record, c->n));
  if (c->watch_words != c->words) return set_error(GP_ESTATE, "internal: watched peers at another row width");
  const int cur = c->cur;
  WatchArgs a{};
  a.wcol = c->d_watch_col;
  a.wslot = c->d_watch_slot;
  a.wv = c->d_watch_v;
  a.state = c->d_state;
  a.cur_rows = c->d_frx[cur];
  a.cur_guard = c->d_fpop[cur];
  a.next_rows = c->d_frx[cur ^ 1];
  a.next_guard = c->d_fpop[cur ^ 1];
  a.first = c->d_watch_first;
  a.arrival = c->d_watch_arrival;
  a.arcs = c->watch_arcs;
  a.peers = (int32_t)c->h_watch_v.size();
  a.r = (uint32_t)c->round;
  GP_TRY(with_words(c->words, [&](auto w) { launch_watch_w<w()>(c, a); }));
  GP_HIP(hipGetLastError());
  return 0;
}

// (the request is gp_watch's list, not a flag)
static bool watch_wanted(const Ctx* c) { return c->watch_want(); }
GP_RECORD_OPS(watch_record) = {R_WATCH, "watched peers", "gp_watch", true, 6, watch_wanted, nullptr, watch_reset,
                                watch_free, watch_count_round, watch_forget, nullptr};

// `rows` record rows from `src` (device stride 64 W) to the host's m columns
static int watch_copy_rows(Ctx* c, void* host, const uint8_t* src, int64_t rows) {
  if (rows <= 0 || c->m <= 0) return 0;
  GP_HIP(hipSetDevice(c->device));
  GP_HIP(hipStreamSynchronize(c->stream));
  GP_HIP(hipMemcpy2D(host, (size_t)c->m, src, (size_t)c->words * 64, (size_t)c->m, (size_t)rows, hipMemcpyDeviceToHost));
  return 0;
}

int watch_read(Ctx* c, int32_t what, void* host, int64_t bytes) {
  GP_TRY(record_readable(c, watch_record));
  const int64_t K = (int64_t)c->h_watch_v.size(), A = c->watch_arcs;
  const int64_t want = what == GP_WATCH_PTR ? (K + 1) * 8 : (what == GP_WATCH_FIRST ? K : A) * (int64_t)c->m;
  if (bytes != want) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(want));
  if (what == GP_WATCH_PTR) {
    std::copy(c->h_watch_ptr.begin(), c->h_watch_ptr.end(), static_cast<int64_t*>(host));
    return 0;
  }
  return what == GP_WATCH_FIRST ? watch_copy_rows(c, host, c->d_watch_first, K)
                                : watch_copy_rows(c, host, c->d_watch_arrival, A);
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_watch(gp_ctx* c, int32_t count, const int32_t* verts, int64_t max_bytes) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  if (count < 0 || (count > 0 && !verts) || max_bytes < 0) return set_error(GP_EINVAL, "bad argument");
  if (count == 0) {
    c->h_watch_want.clear();   // (freed at the next gp_reset)
    return 0;
  }
  const bool single = c->nranks == 1;   // (a vertex-partitioned context keeps no record: its reads say so)
  if (c->n <= 0 || (single && c->h_row_ptr.size() != (size_t)c->n + 1)) return set_error(GP_ESTATE, "no graph loaded");
  if (count > GP_WATCH_MAX_PEERS)
    return set_error(GP_EINVAL, "more than " + std::to_string(GP_WATCH_MAX_PEERS) + " watched peers");
  std::vector<int32_t> list(verts, verts + count);
  std::unordered_set<int32_t> seen;
  for (int32_t v : list) {
    if (v < 0 || (int64_t)v >= c->n) return set_error(GP_EINVAL, "watched peer " + std::to_string(v) + " is not a vertex");
    if (!seen.insert(v).second) return set_error(GP_EINVAL, "watched peer " + std::to_string(v) + " is listed twice");
  }
  const int64_t limit = max_bytes ? max_bytes : WATCH_DEFAULT_BYTES;
  const int64_t need = single ? watch_bytes(count, watch_count_arcs(c, list), c->words) : 0;
  if (need > limit)
    return set_error(GP_ENOMEM, "watched peers: the record needs " + std::to_string(need) + " bytes, max_bytes is " +
                                    std::to_string(limit));
  c->h_watch_want.swap(list);   // (allocated, and kept, from the next gp_reset)
  c->watch_max_bytes = limit;
  return 0;
}

int gp_watch_info(gp_ctx* c, int32_t* count, int64_t* arcs, int64_t* bytes) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  const bool on = c->rec[R_WATCH].on && state_ready(c);
  const int64_t K = on ? (int64_t)c->h_watch_v.size() : 0, A = on ? c->watch_arcs : 0;
  if (count) *count = (int32_t)K;
  if (arcs) *arcs = A;
  if (bytes) *bytes = on ? watch_bytes(K, A, c->watch_words) : 0;
  return 0;
}

int gp_read_watch_peer(gp_ctx* c, int32_t slot, void* first_row, void* arrival, int64_t arrival_bytes) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  GP_TRY(record_readable(c, watch_record));
  if (slot < 0 || (size_t)slot >= c->h_watch_v.size()) return set_error(GP_EINVAL, "no such slot");
  const int64_t b = c->h_watch_ptr[(size_t)slot], deg = c->h_watch_ptr[(size_t)slot + 1] - b;
  if (arrival_bytes != deg * (int64_t)c->m)
    return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(deg * (int64_t)c->m));
  if (!first_row || (arrival_bytes > 0 && !arrival)) return set_error(GP_EINVAL, "null argument");
  const size_t row = (size_t)c->words * 64;
  GP_TRY(watch_copy_rows(c, first_row, c->d_watch_first + (size_t)slot * row, 1));
  return watch_copy_rows(c, arrival, c->d_watch_arrival + (size_t)b * row, deg);
}

}  // extern "C"
