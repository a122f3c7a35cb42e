// load.hip -- per-peer traffic record: sent[u], the
// gossip lines peer u put on the wire, and recv[v], the lines that arrived at
// v, duplicates included.  It is the total of what every reference peer keeps
// line by line: Peer.py:206 and Peer.py:286 log each arriving message with the
// peer it came from, Peer.py:402-404 send on every outgoing link.
//
//   sent[u] += x[u] * max(deg_live[u], 0)
//   recv[v] += up(v) * sum_{u in In(v)} x[u]
//
// with x = |frontier_r| (fpop[cur] at the hook of round r, driver.hip
// round_launch) when the run counts per round (eager: liveness, or
// GP_LOAD_EAGER=1), and x = seenpop - fpop[cur] once at read time when no
// vertex was ever down (lazy: every held bit was in its holder's frontier
// exactly once, but for the current, unsent frontier).
//
// k_load: one-wave blocks.  A wave takes 64 consecutive receivers and streams
// their in-arcs as one flat sequence (load_seg.h: prefix of the row lengths
// and the rows' first arcs in LDS), LOAD_K chunks of 64 column ids per step,
// the next step's column ids in flight while this step gathers x and adds.
// Each lane finds its owner by a search of the LDS prefix.  A chunk inside one
// row -- every chunk of a long row but its ends -- is a wave reduction and one
// LDS add; a chunk over several short rows adds per lane.  The lane phase adds
// sent[] for the wave's 64 vertices.  Hubs (in-degree > hub_threshold) are left to k_load_hub, one wave
// per HubItem of the existing hub table: strided sum, wave reduction, one
// 64-bit atomicAdd (integer adds commute: the totals are deterministic).
//
// Width: x <= 4096 (messages per context).  A u32 partial is used only where
// arcs * 4096 < 2^32 is certain (stated there); everything else is u64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "gp_device.h"
#include "load_seg.h"

namespace gp {

constexpr int LOAD_K = 4;   // chunks of 64 column ids per step (two steps in flight)

struct LoadArgs {
  const int64_t* __restrict__ row_ptr;
  const int32_t* __restrict__ col;
  const uint32_t* __restrict__ x;        // [n] lines each vertex sends per out-link
  const u64* __restrict__ abits;         // PROBE >= 1: bit u = (x[u] != 0)
  const u64* __restrict__ sbits;         // PROBE == 2: bit w = (abits[w] != 0)
  const uint8_t* __restrict__ state;
  const int32_t* __restrict__ deg_live;
  const HubItem* __restrict__ items;
  u64* __restrict__ sent;
  u64* __restrict__ recv;
  int64_t n, n_items;
  int64_t hub_thr;
};

// PROBE: what a lane reads before the random 4-B load of x[u].  0: nothing
// (most vertices send: x sits in the Infinity Cache and the probes only add
// their own trip).  1: the activity bitmap (2 MB at 2^24, L2-resident).  2:
// its summary level first (32 KB at 2^24: stays in the CU's vector cache), for
// rounds with so few senders that the bitmap probes, one L2 request per arc,
// are the whole pass
template <int PROBE>
__device__ __forceinline__ uint32_t load_x(const LoadArgs& a, int32_t u) {
  if (u < 0) return 0u;
  if (PROBE == 2 && !((a.sbits[u >> 12] >> ((u >> 6) & 63)) & 1ull)) return 0u;
  if (PROBE >= 1 && !((a.abits[u >> 6] >> (u & 63)) & 1ull)) return 0u;
  return a.x[u];
}

template <int PROBE>
__global__ __launch_bounds__(64) void k_load(LoadArgs a) {
  typedef int64_t P;   // flat positions of the wave's arcs (load_seg.h)
  __shared__ P pre[LOAD_ROWS + 1];
  __shared__ int64_t beg[LOAD_ROWS];
  __shared__ u64 acc[LOAD_ROWS];
  const int lane = threadIdx.x;
  const int64_t v = (int64_t)blockIdx.x * LOAD_ROWS + lane;
  const bool in = v < a.n;
  int64_t b = 0, e = 0;
  bool up = false;
  if (in) {
    b = a.row_ptr[v];
    e = a.row_ptr[v + 1];
    up = !(a.state[v] & ST_DOWN);
    const uint32_t xv = a.x[v];
    if (xv) {   // the lane phase: v as a sender
      const int32_t dl = max(a.deg_live[v], 0);
      if (dl) a.sent[v] += (u64)xv * (u64)(uint32_t)dl;
    }
  }
  P inc = load_row_len(b, e, up, a.hub_thr);
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const P t = (P)__shfl_up((long long)inc, s);
    if (lane >= s) inc += t;
  }
  if (lane == 0) pre[0] = 0;
  pre[lane + 1] = inc;
  beg[lane] = b;
  acc[lane] = 0ull;
  __syncthreads();
  const P total = pre[LOAD_ROWS];
  struct Step {
    int32_t c[LOAD_K];    // column id (-1: past the end)
    int own[LOAD_K];      // owner row of the lane's position
    bool one[LOAD_K];     // the chunk lies in one row (wave-uniform)
  };
  auto fetch = [&](P p0, Step& s) {
#pragma unroll
    for (int k = 0; k < LOAD_K; ++k) {
      const P pc = p0 + (P)(k * 64);   // wave-uniform
      s.c[k] = -1;
      s.own[k] = 0;
      s.one[k] = false;
      if (pc < total) {
        const P p = pc + (P)lane;
        const P last = std::min<P>(pc + (P)64, total);
        const int o = load_owner(pre, std::min<P>(p, last - 1));   // (lanes past the end: the last position's)
        s.own[k] = o;
        s.one[k] = load_chunk_in_row(pre, uniform(o), last);       // lane 0 holds position pc
        if (p < total) s.c[k] = a.col[load_arc(pre, beg, o, p)];
      }
    }
  };
  Step cur;
  fetch((P)0, cur);
  for (P p0 = 0; p0 < total; p0 += (P)(64 * LOAD_K)) {
    Step nxt;
    fetch(p0 + (P)(64 * LOAD_K), nxt);
    uint32_t val[LOAD_K];
#pragma unroll
    for (int k = 0; k < LOAD_K; ++k) val[k] = load_x<PROBE>(a, cur.c[k]);
#pragma unroll
    for (int k = 0; k < LOAD_K; ++k) {
      if (p0 + (P)(k * 64) >= total) break;
      if (cur.one[k]) {
        // u32: 64 arcs x 4096 messages = 2^18
        const uint32_t s = wave_sum_u32(val[k]);
        if (lane == 0 && s) atomicAdd(&acc[cur.own[k]], (u64)s);
      } else if (val[k]) {
        atomicAdd(&acc[cur.own[k]], (u64)val[k]);
      }
    }
    cur = nxt;
  }
  __syncthreads();
  // this wave alone writes its non-hub receivers (a hub's acc is 0: no arcs)
  if (in && acc[lane]) a.recv[v] += acc[lane];
}

template <int PROBE>
__global__ __launch_bounds__(HBLOCK) void k_load_hub(LoadArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t it = (int64_t)blockIdx.x * HWAVES + (threadIdx.x >> 6);
  if (it >= a.n_items) return;
  const HubItem h = a.items[it];
  if (a.state[h.v] & ST_DOWN) return;
  // u64: an item holds up to hub_threshold arcs, a lane a 64th of them
  u64 s = 0;
  for (int64_t j0 = h.beg; j0 < h.end; j0 += 64 * LOAD_K) {
    int32_t c[LOAD_K];
#pragma unroll
    for (int k = 0; k < LOAD_K; ++k) {
      const int64_t j = j0 + k * 64 + lane;
      c[k] = j < h.end ? a.col[j] : -1;
    }
#pragma unroll
    for (int k = 0; k < LOAD_K; ++k) s += load_x<PROBE>(a, c[k]);
  }
  s = wave_sum_u64(s);
  if (lane == 0 && s) atomicAdd(&a.recv[h.v], s);
}

// lazy read: x[v] = lines v has sent per out-link so far
__global__ void k_load_x(const uint32_t* __restrict__ seenpop, const uint32_t* __restrict__ fpop,
                         uint32_t* __restrict__ x, int64_t n) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) x[v] = seenpop[v] - fpop[v];
}

bool load_env_eager() {
  const char* e = getenv("GP_LOAD_EAGER");
  return e && e[0] == '1';
}

static void load_free(Ctx* c) {
  dfree(&c->d_load_sent);
  dfree(&c->d_load_recv);
  dfree(&c->d_load_x);
  record_off(c->rec[R_LOAD]);
}

// gp_reset: gp_track_load takes effect (two u64[n] and one u32[n], or none), cleared
static int load_reset(Ctx* c) {
  if (!c->d_load_sent) {
    const size_t n = (size_t)c->n;
    if (dalloc(&c->d_load_sent, n) != 0 || dalloc(&c->d_load_recv, n) != 0 || dalloc(&c->d_load_x, n) != 0) {
      load_free(c);
      return GP_ENOMEM;
    }
  }
  GP_HIP(hipMemsetAsync(c->d_load_sent, 0, (size_t)c->n * 8, c->stream));
  GP_HIP(hipMemsetAsync(c->d_load_recv, 0, (size_t)c->n * 8, c->stream));
  return 0;
}

template <int PROBE>
static void launch_load_p(Ctx* c, const LoadArgs& a) {
  hipStream_t s = c->stream;
  const dim3 g(grid_for(c->n, LOAD_ROWS));
  hipLaunchKernelGGL(k_load<PROBE>, g, dim3(64), 0, s, a);
  if (c->n_hub_items > 0)
    hipLaunchKernelGGL(k_load_hub<PROBE>, dim3(grid_for(c->n_hub_items, HWAVES)), dim3(HBLOCK), 0, s, a);
}

static int launch_load(Ctx* c, const uint32_t* x, int probe) {
  if (c->n <= 0) return 0;
  LoadArgs a{};
  a.row_ptr = c->d_row_ptr;
  a.col = c->d_col;
  a.x = x;
  a.abits = c->d_abits;
  a.sbits = c->d_sbits;
  a.state = c->d_state;
  a.deg_live = c->d_deg_live;
  a.items = c->d_hub_items;
  a.sent = c->d_load_sent;
  a.recv = c->d_load_recv;
  a.n = c->n;
  a.n_items = c->n_hub_items;
  a.hub_thr = c->cfg.hub_threshold;
  if (probe == 2) launch_load_p<2>(c, a);
  else if (probe == 1) launch_load_p<1>(c, a);
  else launch_load_p<0>(c, a);
  GP_HIP(hipGetLastError());
  return 0;
}

// the run counts per round: some vertex may be down, or the lever says so
static bool load_eager(const Ctx* c) { return c->load_force || c->liveness_active; }
static bool load_lazy(const Ctx* c) { return !load_eager(c); }
static bool load_counting(const Ctx* c) { return c->rec[R_LOAD].on && c->rec[R_LOAD].valid; }

// round r, after L_r and I_r: fpop[cur] is |frontier_r|, state and deg_live are E_r's
int load_before_expand(Ctx* c) {
  if (!load_counting(c) || !load_eager(c)) return 0;
  // this round's senders are last round's receivers and this round's origins
  // (crashes aside), and the arcs that leave them are the gathers a probe
  // cannot save.  The choice moves time only: every variant adds the same.
  // (C4, per round: no probe 4.6 ms flat; bitmap 1.6 ms + 4.1 ms x the sender
  // arcs' share, so even at 3/4; profiles/r12_load_cost.txt)
  const u64 senders = c->prev_receivers + (u64)c->inj_groups_at(c->round);
  const u64 sender_arcs =
      c->prev_next_arcs + ((size_t)c->round < c->inj_arcs.size() ? (u64)c->inj_arcs[(size_t)c->round] : 0ull);
  const int probe = sender_arcs * 4 >= (u64)c->nnz * 3 ? 0 : senders * 256 <= (u64)c->n ? 2 : 1;
  // the activity bitmap is not current here: k_mkbits builds d_abits (and
  // k_mksum d_sbits) inside launch_expand, after this hook, from the same
  // fpop[cur].  The pass has them built ahead, into the same buffers
  if (probe >= 1) GP_TRY(launch_activity_bits(c, probe == 2));
  return launch_load(c, c->d_fpop[c->cur], probe);
}

// a lazy run's totals from its state: cleared and computed from scratch (idempotent)
static int load_flush(Ctx* c) {
  hipStream_t s = c->stream;
  GP_HIP(hipMemsetAsync(c->d_load_sent, 0, (size_t)c->n * 8, s));
  GP_HIP(hipMemsetAsync(c->d_load_recv, 0, (size_t)c->n * 8, s));
  hipLaunchKernelGGL(k_load_x, dim3(grid_for(c->n, 256)), dim3(256), 0, s, c->d_seenpop, c->d_fpop[c->cur],
                     c->d_load_x, c->n);
  return launch_load(c, c->d_load_x, 0);
}

// gp_crash is about to turn liveness on in a lazy run: the rounds so far are
// booked once, before the crash is applied; the run is eager from here on
int load_before_liveness(Ctx* c) {
  if (!load_counting(c) || load_eager(c)) return 0;
  return load_flush(c);
}

// No count_round: the eager pass runs before the expansion (load_before_expand).
// The accumulators are not in a checkpoint's blob: a lazy run needs none (its
// totals are a function of the restored state), an eager one past round 0 has
// lost its own.  The pass reads no frontier rows
static bool load_no_rows(const Ctx*) { return false; }
GP_RECORD_OPS(load_record) = {R_LOAD, "per-peer loads", "gp_track_load", true, 1, nullptr, load_no_rows, load_reset,
                               load_free, nullptr, nullptr, load_lazy};

int load_read(Ctx* c, int32_t what, void* host, int64_t bytes) {
  GP_TRY(record_readable(c, load_record));
  if (bytes != c->n * 8) return set_error(GP_EINVAL, "bytes mismatch: expected " + std::to_string(c->n * 8));
  if (!load_eager(c)) GP_TRY(load_flush(c));
  return copy_sync(c, host, what == GP_LOAD_SENT ? c->d_load_sent : c->d_load_recv, (size_t)bytes,
                   hipMemcpyDeviceToHost);
}

}  // namespace gp

using namespace gp;

extern "C" {

int gp_track_load(gp_ctx* c, int32_t on) { return record_track(c, load_record, on); }

}  // extern "C"
