// gp_internal.h -- context layout and helpers shared by the translation units of
// libgossip_hip.so.  Not part of the ABI (include/gossip_capi.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gossip_capi.h"
#include "gp_common.h"
#include "records.h"
#include "round_plan.h"

namespace gp {

typedef unsigned long long u64;

// stats slots in the device counter block (u64 each)
// slots [0, NST) are per-block partial sums (all-reduced across ranks);
// the cursors above are rank-local device counters
enum StatSlot {
  S_INJECTED = 0, S_LOST, S_NEW_BITS, S_RECEIVERS, S_SENDS, S_ACTIVE, S_CRASHED,
  S_REPORTS, S_REMOVALS, S_DUP, S_ARCS, S_GATHERED, S_SEEN_READ, S_WRITTEN,
  S_VISITED, S_NEXT_ARCS, S_ATOMICS, S_ROW_BYTES,
  S_XROWS, S_XBYTES,   // boundary entries / bytes sent (vertex partition, written by the pack step)
  S_DNB,               // receivers completed from a done in-neighbour (k_expand)
  S_LM_ROWS,           // senders' rows read by k_mklm to build line masks
  S_ALIASED,           // receivers committed as an alias of their component row (no row write, §3.2)
  NST,
  // boundary entries the unpack found inconsistent with the exchange plan
  // (partition.hip k_rx_unpack); all-reduced with the counters, fails the round
  S_XERR = NST + 1,
  S_REPORT_CURSOR = 26, S_CAND, S_ACTIVE_CURSOR, S_BIG_CURSOR, S_TOUCH_CURSOR, S_DET_BIG,
  S_ULIST,  // entries of the next round's receiver list (k_expand survivors)
  S_REPAIR_X, S_REPAIR_LINES   // a repair round's exchanges and lines carried (k_repair_offer)
};
static_assert(S_REPAIR_LINES < 64, "the counter block read back each round holds 64 slots");
static_assert(S_XERR < S_REPORT_CURSOR, "S_XERR must be inside the all-reduced counter slots");

struct HubItem {       // one wave's share of a hub's in-list
  int32_t v;           // hub vertex
  int32_t hub;         // index into the hub table
  int64_t beg, end;    // arc range
};

struct InjectSpan { int64_t off; int64_t cnt; };

struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[6] = {};
  // side stream of the pull rounds (pull.hip launch_expand_w): the hub chunks
  // run on it beside the round's main pull kernel, between ev_fork (recorded
  // on the engine stream) and ev_join (which the engine stream waits for).
  // Nothing else is ever enqueued on it
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  gp_config cfg{};

  // graph (full, replicated on every rank)
  int64_t n = 0, nnz = 0;
  int directed = 0;
  int64_t* d_row_ptr = nullptr;
  int32_t* d_col = nullptr;
  int64_t* d_out_row_ptr = nullptr;   // directed only
  int32_t* d_out_col = nullptr;
  int32_t* d_deg_out = nullptr;
  int32_t* d_comp = nullptr;          // weakly connected component label (min vertex id)
  std::vector<int64_t> h_row_ptr;     // host copy (hub table, partition)

  // partition.  Kernels address vertices by LOCAL id: one rank (nranks == 1)
  // holds the whole overlay and local == global; a vertex-partitioned context
  // (nranks > 1, partition.hip) holds its owned slice as local ids [0, nloc),
  // then its ghosts -- the non-owned in-neighbours of owned vertices, sorted by
  // global id, hence grouped by owner -- then the message origins that are
  // neither ("extras", so that every rank sees every origin's liveness).
  int32_t rank = 0, nranks = 1;
  std::vector<int64_t> h_bounds;      // [nranks + 1] owned slices (xplan.h partition_bounds)
  int64_t vbegin = 0, vend = 0;       // owned vertices, GLOBAL ids
  int64_t n_alloc = 0;                // local vertex slots: nloc + nghost + nextra
  bool local = false;                 // vertex-partitioned (local ids != global ids)
  int64_t nghost = 0, nextra = 0;
  int64_t nnz_l = 0;                  // arcs of the device CSR (local CSR when partitioned)
  int32_t* d_l2g = nullptr;           // [n_alloc] global id of each local vertex (partitioned only)
  std::vector<int32_t> h_l2g;         // host copy
  std::vector<int32_t> h_comp_g;      // global component labels (extras need theirs)
  std::vector<int32_t> h_deg_g;       // global degrees (partitioned: extras, inj_arcs)
  int64_t base_nv = 0;                // nloc + nghost (local slots before the extras)
  // boundary exchange (partitioned): the owned vertices that are
  // ghosts on rank q, peer-major (flat entry t, [bnd_ptr[q], bnd_ptr[q+1])) and
  // vertex-major (owned boundary vertex k -> its entries).  Rank q's ghosts of
  // owner p are, in the same order, exactly B_pq: no id lists are exchanged.
  std::vector<int64_t> h_bnd_ptr;     // [nranks + 1]
  std::vector<int64_t> h_gh_ptr;      // [nranks + 1] ghost index offsets per owner
  int64_t n_bnd = 0, n_bvx = 0;       // flat entries, owned boundary vertices
  int32_t* d_bnd_e = nullptr;         // [n_bnd] index of entry t within its peer list
  int32_t* d_bnd_k = nullptr;         // [n_bnd] vertex-major index of entry t
  int32_t* d_bvx_v = nullptr;         // [n_bvx] owned local vertex
  int32_t* d_bvx_ptr = nullptr;       // [n_bvx + 1] -> d_bvx_t
  int32_t* d_bvx_t = nullptr;         // [n_bnd] entries of vertex k
  int64_t* d_bnd_ptr = nullptr;       // [nranks + 1]
  u64* d_bvx_info = nullptr;          // [n_bvx] word mask of this round's new row (0: none)
  uint8_t* d_bvx_flag = nullptr;      // [n_bvx] bit 0: new row, bit 1: removed this round
  u64* d_bnd_scan = nullptr;          // [n_bnd + 1] exclusive scan of (heads << 40 | words)
  u64* d_xsize = nullptr;             // [max(n_bnd, nghost) + 1] entry sizes (scan input)
  u64* d_sbuf_h = nullptr;            // send heads (e | flags << 32 | popc << 40)
  u64* d_sbuf_w = nullptr;            // send words (mask word, then the nonzero words)
  u64* d_rbuf_h = nullptr;            // received heads, by sender rank
  u64* d_rbuf_w = nullptr;            // received words, by sender rank
  u64* d_rscan = nullptr;             // [nghost + 1] word offsets of the received entries
  u64* d_cnt = nullptr;               // [4 * nranks] per peer: head start, heads, word start, words
  u64* d_cnt_all = nullptr;           // [nranks][4 * nranks]
  u64* h_cnt_all = nullptr;           // pinned copy
  std::vector<int64_t> h_ghosts_all;  // [nranks][nranks] ghosts rank d holds of owner q (checked once)
  u64* d_alive_all = nullptr;         // [nranks][W]
  void* d_scan_tmp = nullptr;
  size_t scan_tmp_bytes = 0;

  // messages
  int32_t m = 0, words = 0;
  std::map<int32_t, InjectSpan> inject;   // round -> groups
  int32_t last_inject_round = -1;
  int64_t n_groups = 0;               // (round, origin) injection groups
  bool done_at_valid = false;
  int32_t* d_inj_origin = nullptr;
  u64* d_inj_bits = nullptr;
  uint32_t* d_inj_cnt = nullptr;

  // per-run state
  // Message-List slots: v's seen row lives in d_slot[d_sp[v]];
  // round r reads S[r & 1] and writes S[(r + 1) & 1]; cur == r & 1
  u64* d_slot[3] = {nullptr, nullptr, nullptr};    // [n_alloc][W]; slot 2: parked rows (below)
  u64* d_rows = nullptr;            // the allocation of d_slot[0], d_slot[1] and d_acc (in that order)
  // parking: an unfiltered pull under liveness reads every in-neighbour's row
  // of slot r & 1, so before it the rows of down vertices move to slot 2
  // (sp = 2) and both read-slot rows are zeroed; slot 2 is allocated lazily
  // (carry.park_failed: it could not be)
  uint8_t* d_sp = nullptr;          // [n_alloc] slot of v's seen row (0xFF: none)
  uint8_t* d_ws = nullptr;          // [n_alloc] bit p: slot p written this run
  u64* d_frx[2] = {nullptr, nullptr};     // exact frontier rows, kept while anyone wants them (records.h frx_users)
  int64_t frx_rows = 0;                   // rows d_frx covers (partitioned: the owned ones)
  uint32_t frx_sized = 0;                 // frx_users() when alloc_state sized them
  // the per-run records' request / in force / valid flags (records.h), by RecordId
  RecordState rec[R_COUNT];
  // spread curve (curve.hip): [255][W * 64] first receipts per
  // receipt round and message over the owned vertices.  alloc_state makes the
  // buffer with the run state (it follows the row width): curve_alloc
  u64* d_curve = nullptr;
  bool curve_alloc = false;
  int curve_grid = 0;                     // GP_CURVE_GRID at gp_create: cap of k_curve's grid (0: none)
  bool curve_yard = false;                // GP_CURVE_YARDSTICK=1 at gp_create: time k_curve beside k_bitsum
  // per-peer traffic record (load.hip): lines sent / received
  // per vertex since gp_reset, and the lazy read's scratch (x = seenpop - fpop).
  // A lazy run's totals are a function of its state: a restore keeps them
  u64* d_load_sent = nullptr;             // [n]
  u64* d_load_recv = nullptr;             // [n]
  uint32_t* d_load_x = nullptr;           // [n]
  bool load_force = false;                // GP_LOAD_EAGER=1 at gp_create: count per round from round 0
  // per-peer fresh deliveries (fresh.hip): of those lines, the
  // ones that carried a first receipt, per sender and per receiver since
  // gp_reset
  u64* d_fresh_sent = nullptr;            // [n]
  u64* d_fresh_recv = nullptr;            // [n]
  bool fresh_gather = false;              // GP_FRESH_GATHER=1 at gp_create: undirected overlays gather once per role
  // fresh-delivery curve (fresh_curve.hip): [255][W * 64] the
  // deliverers of every message's first receipts per receipt round, the
  // per-message split of fresh_recv
  u64* d_fresh_curve = nullptr;
  size_t fresh_curve_words = 0;           // u64 d_fresh_curve holds
  int fresh_curve_grid = 0;               // GP_FRESH_CURVE_GRID at gp_create: cap of k_fresh_curve's grid (0: none)
  // per-link fresh deliveries (link.hip): the same news per arc
  // of the in-CSR, the matrix d_fresh_sent / d_fresh_recv are the column / row
  // sums of.  u16 per arc: over a run arc u -> v counts a message at most once
  // (v receives it for the first time once), so link_fresh[j] <= m <= 4096 --
  // and a path with every message injected at one end attains it
  uint16_t* d_link = nullptr;             // [nnz] in-CSR arc order
  u64* d_link_hist = nullptr;             // [4097] gp_read_link_hist's device result
  size_t link_arcs = 0;                   // arcs d_link holds
  // per-peer receipt delays (delay.hip): over the owned
  // vertices, the sum and the maximum of first[v][k] - inject_round[k] over the
  // messages v holds.  A table whose messages all start in one round needs no
  // frontier rows (delay_uniform).  Partitioned contexts keep it for their
  // owned slice
  uint32_t* d_delay_sum = nullptr;        // [nloc]
  uint8_t* d_delay_max = nullptr;         // [nloc]
  u64* d_delay_planes = nullptr;          // [8][W] inject-round planes of the context's table (delay_planes.h)
  u64* d_delay_bins = nullptr;            // [32][5] gp_read_delay_bins' device result
  size_t delay_rows = 0;                  // vertices the two arrays hold
  std::vector<uint8_t> h_inj_round;       // [m] inject round of every message of the context's table
  int32_t delay_uniform = -1;             // the table's one inject round (-1: they differ)
  bool delay_force_rows = false;          // GP_DELAY_ROWS=1 at gp_create: the row pass for a one-round table too
  bool delay_by_rows() const { return delay_uniform < 0 || delay_force_rows; }
  // per-peer delay distributions (delay_dist.hip): the same
  // receipts per delay value, u16 [nloc][16] (delays 0 .. 14, 15 or more).  The
  // two records are independent, share delay_uniform / delay_force_rows, and
  // either one with a table of several inject rounds keeps the frontier rows
  uint16_t* d_ddist = nullptr;            // [nloc][16]
  u64* d_ddist_planes = nullptr;          // [8][W] inject-round planes of the context's table
  u64* d_ddist_bins = nullptr;            // [32][16] gp_read_delay_dist_bins' device result
  uint64_t ddist_present[4] = {0, 0, 0, 0};   // the table's inject rounds as a 256-bit set (delay_dist.h)
  size_t ddist_rows = 0;                  // vertices the array holds
  bool delay_needs_rows() const {
    return delay_rows_needed(rec[R_DELAY].want, rec[R_DELAY_DIST].want, delay_uniform, delay_force_rows);
  }
  // delivery multiplicity (mult.hip): how many in-neighbours
  // delivered each first receipt -- the histogram of that number, and per peer
  // the receipts with one deliverer, as receiver and as that deliverer
  uint32_t* d_sole_recv = nullptr;        // [n]
  u64* d_sole_sent = nullptr;             // [n]
  u64* d_mult_hist = nullptr;             // [256][17] copies of the histogram (bin 0 unused: the injections)
  u64* d_sole_bins = nullptr;             // [32][4] gp_read_sole_bins' device result
  u64* d_mult_scratch = nullptr;          // [n_hub_items][5][W] the hub items' counters of one round
  u64* d_mult_hub_sole = nullptr;         // [n_hubs][W] the hubs' sole masks of one round
  size_t mult_rows = 0, mult_scratch_words = 0, mult_hub_words = 0;   // what the arrays were sized for
  // watched peers (watch.hip): the arrival log of a caller-chosen
  // list of peers, one byte per (in-arc, message) and per (peer, message).
  // h_watch_want is what gp_watch set, for the next gp_reset; h_watch_v /
  // h_watch_ptr are the list in force and its arc offsets
  std::vector<int32_t> h_watch_want, h_watch_v;
  std::vector<int64_t> h_watch_ptr;       // [K + 1]
  int64_t watch_max_bytes = 0;            // gp_watch's budget for the two byte arrays
  int32_t* d_watch_v = nullptr;           // [K]
  int64_t* d_watch_ptr = nullptr;         // [K + 1]
  int32_t* d_watch_col = nullptr;         // [A] senders of the watched arcs (a compact copy of the in-lists)
  int32_t* d_watch_slot = nullptr;        // [A] their receivers' slots
  uint8_t* d_watch_first = nullptr;       // [K][W * 64], 255 = never
  uint8_t* d_watch_arrival = nullptr;     // [A][W * 64]
  int64_t watch_arcs = 0;                 // A
  int32_t watch_words = 0;                // the row width the arrays were made for
  bool watch_want() const { return !h_watch_want.empty(); }
  // lossy links (lossy.hip): every arc drops the lines of
  // a round with probability p, by a draw of the ordered pair and the round.
  // loss_want / loss_p_want / loss_seed_want are what gp_link_loss asked for,
  // loss_on / loss_p / loss_seed the setting of the run since the last gp_reset
  // (single-rank contexts only)
  bool loss_want = false, loss_on = false;
  double loss_p_want = 0.0, loss_p = 0.0;
  uint64_t loss_seed_want = 0, loss_seed = 0;
  // delayed links (delayed.hip): the link between u and
  // v takes d(u, v) in [1, dmax] rounds, fixed for the run (link_delay.h).
  // lag_want / lag_dmax_want / lag_seed_want are what gp_link_delay asked for,
  // lag_on / lag_dmax / lag_seed the setting of the run since the last gp_reset
  // (single-rank contexts only).  While the ring is in force (lag_ring > 0) it
  // owns every frontier-row buffer: d_lag_frx[0] and [1] are alloc_state's two,
  // the rest its own, and d_frx[cur] / d_frx[cur ^ 1] are rotated through them
  // each round (lag_rotate); lag_release hands the first two back to d_frx
  // before anything frees or reallocates them
  bool lag_want = false, lag_on = false;
  int32_t lag_dmax_want = 1, lag_dmax = 1;
  uint64_t lag_seed_want = 0, lag_seed = 0;
  uint32_t lag_hist = 0;               // bit k: round - 1 - k of this run had a sender (lag_in_flight)
  int32_t lag_ring = 0;                   // buffers of the ring in force: lag_dmax + 1 (0: no ring)
  u64* d_lag_frx[9] = {};                 // [lag_ring] frontier rows of round s live in slot s % lag_ring
  u64* d_lag_bits = nullptr;              // [lag_dmax + 1][lag_nw] k_mkbits' bitmap of round s in row s % lag_dmax; last row: their OR
  int64_t lag_nw = 0;                     // words per bitmap row
  uint8_t* d_lag_arc = nullptr;           // [nnz] d(u, v) per arc of the in-CSR
  // anti-entropy repair (repair.hip): in every round r
  // with (r + 1) % period == 0 each up receiver pulls the Message-List of one
  // in-neighbour drawn from the receiver and the round.  repair_want /
  // repair_period_want / repair_seed_want are what gp_repair asked for,
  // repair_on / repair_period / repair_seed the setting of the run since the
  // last gp_reset (single-rank contexts only, no shard job, no link delay)
  bool repair_want = false, repair_on = false;
  int32_t repair_period_want = 1, repair_period = 1;
  uint64_t repair_seed_want = 0, repair_seed = 0;
  int32_t repair_quiet = 0;               // most recent consecutive rounds >= the last inject round with no new bit
  bool repair_rec_valid = true;           // false: the run was restored past round 0, its record is not kept
  std::vector<uint64_t> repair_rec;       // [rounds][2] exchanges, lines per round since gp_reset
  u64* d_rbits = nullptr;                 // [n_alloc/64] a repair round's receivers below hub_threshold whose
                                          //   accumulator row holds an offer (written whole by k_repair_offer)
  int64_t rbits_words = 0;
  bool holds_frx() const { return frx_users(this) != 0; }
  uint32_t* d_fpop[2] = {nullptr, nullptr};    // [n_alloc]
  int cur = 0;
  uint32_t* d_seenpop = nullptr;    // [nloc]
  uint8_t* d_first = nullptr;       // [nloc][W*64]
  u64* d_digest = nullptr;     // [nloc]
  uint8_t* d_state = nullptr;       // [n_alloc]
  uint8_t* d_miss = nullptr;        // [n_alloc]
  int32_t* d_deg_live = nullptr;    // [n_alloc]
  int32_t* d_cand = nullptr;        // [n] detection candidates of a round
  int32_t* d_det_big = nullptr;     // deferred (big) detection candidates and their counters (k_det_big_*)
  int64_t* d_det_pre = nullptr;
  uint32_t* d_det_live = nullptr;
  uint32_t* d_det_cur = nullptr;
  u64* d_det_base = nullptr;
  // this round's plan (round_plan.h: direction, scan mode, every switch of
  // the pull, its kernel) and what the run's rounds hand to the next one
  RoundPlan plan;
  RoundCarry carry;
  // [n_alloc/64] frontier_r activity bitmap (fpop != 0): 2 MB at 2^24
  u64* d_nbits = nullptr;           // [n_alloc/64] narrow push rounds: receivable vertices (k_mkneed)
  u64* d_abits = nullptr;
  u64* d_sbits = nullptr;   // summary level of d_abits (summary probes)
  // [n_alloc/64] done bitmap of early-exit rounds without liveness (single
  // context): bit v = v held every message of its component at the end of the
  // last round (done in-neighbours)
  u64* d_dbits = nullptr;
  // [n_alloc] line masks (W = 64): bit l = 128-B line l of v's
  // row in this round's slot holds a nonzero word; 0 = not a sender.  Built by
  // k_mklm from the very rows the round's filtered pull reads (SCAN_LINES)
  uint8_t* d_lm = nullptr;
  // [2][n_alloc / 2] the same masks written by the commits of a 64-word pull
  // for the next round's senders (nibbles, by round parity like d_fpop): a
  // line-mask round after such a round (no liveness, one context) probes them
  // without k_mklm's pass over the senders' rows
  uint8_t* d_lmw[2] = {nullptr, nullptr};
  // receiver lists: late early-exit pulls append the
  // receivers that are still neither done nor sated to d_ulist[carry.ul_cur ^ 1];
  // the next pull, when the list is short, launches waves for those alone
  // (SCAN_LIST) and leaves the senders' accounting to k_mkbits
  int32_t* d_ulist[2] = {nullptr, nullptr};
  int32_t acc_row = 0;      // a degree-split round's accumulator rows as rows of its slot buffer
  // [nnz/64 + 2] per-arc activity mask of filtered pull rounds (gcol order): 33.5 MB at C4
  u64* d_amask = nullptr;
  // push (sparse-round) mode
  u64* d_acc = nullptr;             // [nloc][W] OR accumulator, kept all-zero between uses (inside d_rows)
  u64* d_tbits = nullptr;           // [n_alloc/64] receivers pushed to this round
  int32_t* d_touched = nullptr;     // [n_alloc] receivers touched this round
  int32_t* d_active = nullptr;      // [n_alloc] senders (deg <= hub threshold)
  int32_t* d_big = nullptr;         // [n_alloc] senders above the hub threshold
  std::vector<int64_t> inj_arcs;    // per inject round: sum of origin out-degrees
  u64 prev_next_arcs = 0;           // out-degree sum of the last round's receivers
  u64 prev_new_bits = 0;            // new bits of the last round (global)
  u64 prev_receivers = 0;           // receivers of the last round (global)
  u64 held_bits = 0;                // messages held so far, summed over vertices (global)
  // compact Message-Lists: 128-B records per vertex, per slot
  u64* d_cml[2] = {nullptr, nullptr};   // [n_alloc][16] records
  u64* d_cmk[2] = {nullptr, nullptr};   // [n_alloc / 64] dense bitmaps (bit v: no record, read the row)
  int64_t inj_groups_at(int32_t r) const {
    auto it = inject.find(r);
    return it == inject.end() ? 0 : it->second.cnt;
  }
  int32_t* d_gcol = nullptr;        // [nnz] in-CSR columns, rows sorted by neighbour degree desc
  uint32_t* d_hub_done = nullptr;   // [n_hubs] early-exit rounds: a chunk covered its hub's target (hub.hip)
  uint32_t hub_epoch = 0;           // stamp of the last pull launch (k_hub_partial's hub_done)
  int32_t* d_prehi = nullptr;       // [n] degree-split rounds: gather-order prefix of senders with
                                    //   in-degree >= prehi_deg (build_prehi, built on first use)
  int32_t prehi_deg = 0;
  int32_t* d_midx = nullptr;        // [n_alloc] component mask row of v (-1: none)
  u64* d_cmask = nullptr;           // [K][W] messages per component
  std::vector<int32_t> h_inj_origin;   // host copies of the injection groups
  std::vector<u64> h_inj_bits;
  std::vector<int32_t> h_deg_out;
  uint32_t* d_done_at = nullptr;    // [n_alloc] messages of the vertex's component (this run)
  // pristine copies of done_at / cmask: a message whose origin is down at its
  // inject round never exists, so the run drops it from its component's target
  // (k_lost_clear, k_done_fix); gp_reset restores the pristine targets
  uint32_t* d_done_at0 = nullptr;   // [n_alloc]
  u64* d_cmask0 = nullptr;          // [K][W]
  uint32_t* d_lostcnt = nullptr;    // [K] messages lost per component this round
  int32_t cmask_rows = 0;           // K
  bool done_dirty = false;          // the working targets differ from the pristine ones
  u64* d_msg_cov = nullptr;    // [W*64]
  u64* d_msg_fwd = nullptr;    // [W*64]
  u64* d_alive = nullptr;      // [2][W] alive messages per round parity
  u64* d_bc_keys = nullptr;    // [nloc] (degree << 32 | v) sorted: weighted bitcount order (bitcount.hip)
  uint32_t* d_bc_part = nullptr;   // per-block bitcount partials
  size_t bc_part_words = 0;
  int64_t bc_split = 0;        // owned vertices of degree <= the bitcount tail threshold
  u64* d_fin_comp = nullptr;   // finalize by components: [K] counts, [K] degree sums, list cursor
  u64* d_fin_list = nullptr;   // [nloc] incomplete rows (degree << 32 | v)
  int32_t fin_comp_rows = 0;
  gp_report* d_reports = nullptr;
  int64_t report_cap = 0;
  u64* d_stats = nullptr;      // [NSTAT]
  u64* h_stats = nullptr;      // pinned [NSTAT]
  int32_t round = 0;
  bool liveness_active = false;
  // first round whose alive set F_r is complete in d_alive (-1: none yet).
  // The sets are built only while liveness is active, so when an explicit
  // crash turns it on at round r, F_r was never built: r's pull must not
  // narrow its early-exit target with it (F_{r+1} is built by round r)
  int32_t alive_from = -1;
  bool pending_crash = false;
  bool msg_forwards_valid = true;
  int64_t last_reports = 0;

  // hub split
  std::vector<HubItem> h_hub_items;
  HubItem* d_hub_items = nullptr;
  int32_t* d_hubs = nullptr;          // hub vertex per hub
  int32_t* d_hub_item_ptr = nullptr;  // [n_hubs+1]
  u64* d_hub_partial = nullptr;  // [items][W]
  uint32_t* d_hub_pnz = nullptr;      // [items]
  int64_t n_hubs = 0, n_hub_items = 0;
  // [ceil(nloc / 64)] launch order of k_expand's blocks: the blocks with a long
  // non-hub in-list first (block_order.h; rebuilt with the hub table)
  int32_t* d_border = nullptr;
  // per-line done-neighbour rule (line_cands.h): the owned
  // vertices of in-degree >= ld_min_deg (rebuilt with the hub table), and a
  // byte per vertex -- bit l: line l of its Message-List held every message of
  // its component when k_line_done last ran; 0 for every non-candidate
  int32_t* d_ld_cand = nullptr;
  int64_t n_ld_cand = 0;
  uint8_t* d_ldone = nullptr;       // [n_alloc], per-run state
  size_t ldone_bytes = 0;           // its size as allocated
  int32_t ld_env = -1;              // GP_LINE_DONE in the environment at gp_create: 0 off, 1 on, -1 by size
  int32_t ld_min_deg = 0;           // GP_LINE_DONE_MIN_DEG there, else the compile-time default
  int32_t lp_env = -1;              // GP_LINE_PACK in the environment at gp_create: 0 off, 1 on, -1 by size

  // rccl
  ncclComm_t comm = nullptr;

  // message-shard job (shard.hip): jnranks > 0 once a transport
  // is set; the rounds then record the receiver / sender bitmaps of the run
  ncclComm_t jcomm = nullptr;           // gp_shard_comm_init
  gp_allgather_fn jhost = nullptr;      // gp_shard_host_init
  void* jhost_user = nullptr;
  int32_t jrank = 0, jnranks = 0;
  u64* d_hist = nullptr;                // [hist_cap][2][hist_nw]: round r's receivers, then senders
  int32_t hist_cap = 0, hist_rounds = 0;
  int64_t hist_nw = 0;                  // bitmap words d_hist was allocated for (ceil(n_alloc / 64))
  bool hist_valid = true;               // false: the run did not start at gp_reset in this job (restored from a
                                        // checkpoint, transport joined in mid-run): no job record, rounds go on
  std::vector<gp_round_stats> run_stats;   // this run's rounds, as gp_round returned them
  int32_t fin_round = -1;               // round count at the last gp_finalize_messages of this run
  u64* d_jscr = nullptr;                // combine scratch (send / receive chunks)
  size_t jscr_words = 0;
  u64* d_jdig = nullptr;                // [P * ceil(n / P)] the job's digest (first n valid)
  size_t jdig_words = 0;
  u64* d_jcf = nullptr;                 // [2][jm] the job's coverage, forwards
  int32_t jm = 0;                       // messages of the job
  bool j_ready = false, j_fwd_valid = false, j_dig_valid = false;
  u64* d_jcurve = nullptr;              // [j_curve_rows][jm] the job's spread curve
  size_t jcurve_words = 0;
  int32_t j_curve_rows = 0;
  bool j_curve_valid = false;           // every rank tracked a valid curve

  // kernel geometry
  int cu_count = 256;

  int64_t nloc() const { return vend - vbegin; }
  // lookup of a global vertex id among the local ids (-1: not local)
  int64_t to_local(int64_t g) const;

};

// error helpers (thread-local message, negative status)
int set_error(int code, const std::string& msg);
#define GP_HIP(call)                                                              \
  do {                                                                            \
    hipError_t _e = (call);                                                       \
    if (_e != hipSuccess)                                                         \
      return ::gp::set_error(GP_EHIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
  } while (0)
#define GP_RCCL(call)                                                             \
  do {                                                                            \
    ncclResult_t _r = (call);                                                     \
    if (_r != ncclSuccess)                                                        \
      return ::gp::set_error(GP_ERCCL, std::string(#call) + ": " + ncclGetErrorString(_r)); \
  } while (0)
#define GP_TRY(expr)                                                              \
  do { int _rc = (expr); if (_rc != 0) return _rc; } while (0)

// f(std::integral_constant<int, W>{}) for the row width `words`, one of the
// seven the kernels are built for; any other is GP_EINVAL
template <class F>
int with_words(int words, F&& f) {
  switch (words) {
    case 1: f(std::integral_constant<int, 1>{}); return 0;
    case 2: f(std::integral_constant<int, 2>{}); return 0;
    case 4: f(std::integral_constant<int, 4>{}); return 0;
    case 8: f(std::integral_constant<int, 8>{}); return 0;
    case 16: f(std::integral_constant<int, 16>{}); return 0;
    case 32: f(std::integral_constant<int, 32>{}); return 0;
    case 64: f(std::integral_constant<int, 64>{}); return 0;
    default: return set_error(GP_EINVAL, "unsupported word count");
  }
}

template <class T>
int dalloc(T** p, size_t count) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (count == 0) count = 1;
  hipError_t e = hipMalloc((void**)p, count * sizeof(T));
  if (e != hipSuccess) {
    *p = nullptr;
    return set_error(GP_ENOMEM, std::string("hipMalloc ") + std::to_string(count * sizeof(T)) +
                                    " bytes: " + hipGetErrorString(e));
  }
  return 0;
}
template <class T>
void dfree(T** p) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
}

// blocking copy ordered on the engine stream.  A plain hipMemcpy runs on the
// null stream, which a non-blocking stream does not wait for (and a pageable
// host-to-device hipMemcpy may return before its DMA lands), so kernels on
// c->stream could read stale data or race with the copy.
int copy_sync(Ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
// graph_build.hip
int build_chung_lu(Ctx* c, int64_t n, double dbar, double gamma, uint64_t seed);
int build_gather_order(Ctx* c);
int build_prehi(Ctx* c, int32_t T);
// setup.hip
int finish_graph(Ctx* c);
int build_hubs(Ctx* c);
// bitcount.hip
int bitcount_messages(Ctx* c, bool weighted, u64* cov, u64* fwd);   // coverage / forwards of the owned rows
int finalize_by_components(Ctx* c, bool weighted, u64* cov, u64* fwd);   // the same via cmask rows
void bitcount_free(Ctx* c);
// curve.hip
int curve_alloc(Ctx* c, bool on);              // with the run state: the count buffer (or none)
int curve_env_grid();                          // GP_CURVE_GRID in the environment (0: unset)
bool curve_env_yardstick();                    // GP_CURVE_YARDSTICK=1 in the environment
// load.hip: the traffic record's hooks outside the table's walks (records.h)
int load_before_expand(Ctx* c);                // after L_r and I_r of an eager run: round r's sends and arrivals
int load_before_liveness(Ctx* c);              // gp_crash turns liveness on: a lazy run books its rounds so far
bool load_env_eager();                         // GP_LOAD_EAGER=1 in the environment
// the records' typed reads behind gp_read (each in its record's unit)
int load_read(Ctx* c, int32_t what, void* host, int64_t bytes);    // GP_LOAD_SENT / GP_LOAD_RECV
int fresh_read(Ctx* c, int32_t what, void* host, int64_t bytes);   // GP_FRESH_SENT / GP_FRESH_RECV
int link_read(Ctx* c, void* host, int64_t bytes);                  // GP_LINK_FRESH
int delay_read(Ctx* c, int32_t what, void* host, int64_t bytes);   // GP_DELAY_SUM / GP_DELAY_MAX
int delay_dist_read(Ctx* c, void* host, int64_t bytes);            // GP_DELAY_DIST
int mult_read(Ctx* c, int32_t what, void* host, int64_t bytes);    // GP_SOLE_SENT / GP_SOLE_RECV
int watch_read(Ctx* c, int32_t what, void* host, int64_t bytes);   // GP_WATCH_FIRST / GP_WATCH_ARRIVAL / GP_WATCH_PTR
bool fresh_env_gather();                       // GP_FRESH_GATHER=1 in the environment
int fresh_curve_env_grid();                    // GP_FRESH_CURVE_GRID in the environment (0: unset)
bool delay_env_rows();                         // GP_DELAY_ROWS=1 in the environment
// lossy.hip
int loss_reset(Ctx* c);                        // gp_reset: gp_link_loss takes effect, or the reset is refused
// repair.hip
int repair_check_reset(const Ctx* c);          // gp_reset, before anything changes: gp_repair's request can take effect, or the reset is refused
int repair_reset(Ctx* c);                      // gp_reset: it takes effect; the mark bitmap, the record and `quiet` start over
void repair_free(Ctx* c);
int repair_check_round(const Ctx* c);          // before a round: GP_ESTATE when repair is in force in a shard job
bool repair_now(const Ctx* c);                 // repair is in force and the context's round is a repair round
void repair_collect(Ctx* c, const u64* h_stats, u64 new_bits, int32_t r);   // round_collect: the record's row, `quiet`
void repair_restored(Ctx* c, int32_t round);   // gp_checkpoint_load: the record of a run restored past round 0 is not kept
// delayed.hip
int lag_reset(Ctx* c);                         // gp_reset, before anything changes: gp_link_delay's request can take effect, or the reset is refused
int lag_prepare(Ctx* c);                       // gp_reset, with the run state in place: it takes effect; the ring, the bitmaps, the arc delays
void lag_release(Ctx* c);                      // d_frx owns its two buffers again; the ring's own are freed
bool lag_ready(const Ctx* c);                  // the ring in force matches the setting in force
void lag_rotate(Ctx* c);                       // round r: d_frx[cur] / d_frx[cur ^ 1] = the ring's slots of rounds r / r + 1
int lag_check_round(const Ctx* c);             // before a round: GP_ESTATE when delay is in force without its ring, or in a shard job
int32_t lag_in_flight(const Ctx* c);           // past send rounds whose lines may still arrive (0: delay off, or none)
int lag_read(Ctx* c, void* host, int64_t bytes);   // GP_ARC_DELAY
// driver.hip: k_mkbits (and k_mksum) over fpop[cur], ahead of launch_expand
int launch_activity_bits(Ctx* c, bool summary);
// driver.hip: cnt[m] += the rows' bit m over rows [0, count) with guard[i] != 0 (the per-bit k_bitsum)
int bitsum_count_rows(Ctx* c, const u64* rows, const uint32_t* guard, int64_t count, u64* cnt);
// driver.hip: forwards read from the Message-Lists of a run that stopped before
// quiescence, on a context without frontier rows: not kept (GP_ENOTRACK)
bool fwd_pending(const Ctx* c);
bool forwards_unknown(const Ctx* c);
// partition.hip
int localize(Ctx* c);                          // global overlay -> owned + ghost local CSR, boundary lists
int set_extras(Ctx* c, const std::vector<int32_t>& origins_global);   // origins neither owned nor ghosts
void free_partition(Ctx* c);
int alloc_exchange(Ctx* c);                    // exchange buffers for the current row width
int pack_boundary(Ctx* c);                     // after E_r: this round's boundary entries -> send buffers
int exchange_rccl(Ctx* c);                     // counts, rows, alive sets over RCCL, then unpack
int exchange_group(Ctx** ctxs, int32_t nctx);  // the same through device-to-device copies
// pull_aux.hip: write the component rows of aliased vertices (all, or this
// round's senders only) into S[cur]; with all, the run holds no alias after
int unalias(Ctx* c, bool senders_only);
// shard.hip
int shard_prepare_round(Ctx* c);               // before round r of a shard job: history in step, room for r
int shard_record_round(Ctx* c);                // after E_r of a shard job: round r's bitmaps
void shard_free(Ctx* c);
void shard_reset(Ctx* c);                      // new run (gp_reset, checkpoint load)
// state bit: removed by this rank's seed step in the current round (sent to the
// ranks holding the vertex as a ghost; cleared by the next round's k_churn)
constexpr uint8_t ST_RMNEW = 8;
// sated (churn runs): no injection left and v holds every
// message of its component that anyone still forwards; the alive sets only
// shrink from round to round, so v never receives again and the pull skips it
constexpr uint8_t ST_SATED = 16;

}  // namespace gp

// the ABI handle is the context itself
struct gp_ctx : public gp::Ctx {};
