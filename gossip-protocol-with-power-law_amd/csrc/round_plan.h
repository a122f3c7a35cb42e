// round_plan.h -- the plan of one expansion round E_r as a pure function of
// plain numbers: direction (push / pull), scan mode, every per-round switch of
// the pull and the k_expand variant that runs it.  Host
// code without HIP: driver.hip's launch_expand gathers a RoundFacts from the
// context, calls plan_round and enqueues what the plan says; the tests drive
// the same function on the CPU (tests/native/round_plan_shim.cpp).  The
// comments at each rule carry the measurements that set its threshold.
#pragma once
#include <cstdint>

#include "../../include/gossip_capi.h"

namespace gp {

// scan modes of a pull round (compile-time): the per-arc activity probe, the
// per-arc activity mask built by k_arcmask before the round, or no check at all
// (unfiltered dense rounds)
enum ScanMode { SCAN_FILTERED = 0, SCAN_MASKED = 1, SCAN_UNFILTERED = 2, SCAN_PRE = 3,
                SCAN_CML = 4 /* flag: read / write compact Message-Lists (W = 64) */,
                SCAN_ALIVE = 8 /* flag: early-exit targets narrowed to the alive messages (k_expand);
                                  a variant of its own: +2-3 VGPRs cost a wave per SIMD */,
                SCAN_LINES = 32 /* flag (W = 64, filtered): the probe reads the sender's line mask
                                   (k_mklm) and the gather loads only its nonzero 128-B lines */,
                SCAN_DPROBE = 64 /* flag (k_expand, W = 64, filtered / unfiltered): every scanned arc
                                    probes the done bitmap (a.dprobe rounds, aliased Message-Lists);
                                    a variant of its own: +4 VGPRs cost the unfiltered pull a wave */,
                SCAN_LIST = 128 /* flag (k_expand, W >= 32, filtered / unfiltered): the waves take
                                   their receivers from a.ulist, the vertices that could still
                                   receive (late rounds), not 64 consecutive ids */,
                SCAN_QUADS = 256 /* flag (k_expand, unfiltered): W = 64: done-neighbour receivers
                                    four per wave step (dnb_quads) without the done probe, and (no
                                    liveness) receivers of in-degree <= 32 two per step
                                    (gather_pairs): the first aliasing round, near-done pulls,
                                    alive pulls from the half-held round; W = 32 / 16 / 8
                                    near-done pulls: low in-degree receivers 4 / 8 / 16 per step
                                    (gather_groups) */,
                SCAN_PACK = 512 /* flag (k_expand, W = 64, unfiltered early-exit pulls without liveness,
                                   list or done probe): the serial loop's row gather deals its lanes
                                   out over the lines the receiver still misses (gather_rows_pack);
                                   a variant of its own: 1 KB of LDS per wave, and the other
                                   variants keep their code */ };

// The k_expand<W, MODE> variants that are built: MODE, and the narrowest W it
// is instantiated for (narrower rows take the flat kernel by default, line
// masks / records / aliases / receiver lists exist at W = 64 only).  Every
// width guard of the pull's plan and launch is this table.
#define EXPAND_VARIANTS(V)                                                                         \
  V(SCAN_FILTERED, 1) V(SCAN_MASKED, 1) V(SCAN_UNFILTERED, 1) V(SCAN_PRE, 1)                       \
  V(SCAN_UNFILTERED | SCAN_QUADS, 8)                                                               \
  V(SCAN_UNFILTERED | SCAN_PACK, 64)                                                               \
  V(SCAN_UNFILTERED | SCAN_ALIVE, 32) V(SCAN_PRE | SCAN_ALIVE, 32) V(SCAN_FILTERED | SCAN_ALIVE, 32) \
  V(SCAN_UNFILTERED | SCAN_ALIVE | SCAN_QUADS, 64)                                                 \
  V(SCAN_UNFILTERED | SCAN_DPROBE, 64) V(SCAN_FILTERED | SCAN_DPROBE, 64)                          \
  V(SCAN_PRE | SCAN_CML, 64) V(SCAN_FILTERED | SCAN_CML, 64) V(SCAN_FILTERED | SCAN_LINES, 64)     \
  V(SCAN_UNFILTERED | SCAN_LIST, 64) V(SCAN_FILTERED | SCAN_LIST, 64)                              \
  V(SCAN_UNFILTERED | SCAN_ALIVE | SCAN_LIST, 64) V(SCAN_FILTERED | SCAN_ALIVE | SCAN_LIST, 64)    \
  V(SCAN_UNFILTERED | SCAN_DPROBE | SCAN_LIST, 64) V(SCAN_FILTERED | SCAN_DPROBE | SCAN_LIST, 64)

constexpr int expand_min_width(int mode) {
  switch (mode) {
#define V(MODE, MINW) case (MODE): return MINW;
    EXPAND_VARIANTS(V)
#undef V
    default: return 1 << 30;   // not built
  }
}

#ifndef GP_EE_DIV
#define GP_EE_DIV 16.0
#endif
// rows of <= 8 words (the 512-message shards of an 8-GPU job) take the
// edge-parallel kernel, whose early-exit variant costs one 2-arc prefix pass
// when receivers cannot complete: it pays from m/64 new bits per vertex.  The
// shards of the slower messages cross m/16 a round late, and their dense
// round then gathered every active row (profiles/r05_ee_shards.txt: ranks 5-6
// of the N = 8 job 11.3-11.4 -> 8.7-9.0 ms; W = 16 and 64 keep m/16, the
// 1024-message shard's round 3 lost 0.7 ms at m/64)
#ifndef GP_EE_DIV_NARROW
#define GP_EE_DIV_NARROW 64.0
#endif
#ifndef GP_NARROW_PUSH_SCALE
#define GP_NARROW_PUSH_SCALE 0.25
#endif
#ifndef GP_NARROW_PUSH_MAXW
#define GP_NARROW_PUSH_MAXW 16
#endif
#ifndef GP_ULIST_DIV
#define GP_ULIST_DIV 3
#endif
// summary probes only while at most n / SUMMARY_RATIO vertices send
constexpr double SUMMARY_RATIO = 256.0;
constexpr double NARROW_ND_DIV = 16;
constexpr double CML_AVG_BITS = 16.0;

// What the rounds of a run hand to the next one (Ctx::carry).  RoundCarry{} is
// the state at gp_reset; round_collect advances it.
struct RoundCarry {
  bool cml_written = false;    // the last round's commits wrote compact Message-List records
  bool lm_written = false;     // ... wrote the line masks of this round's senders (d_lmw)
  // the run holds aliased Message-Lists: readers of rows
  // outside the done-probe pulls materialize them first (k_unalias)
  bool alias_active = false;
  bool ulist_valid = false;    // the last round appended a receiver list ...
  int64_t ulist_n = 0;         // ... of this many vertices ...
  int32_t ul_cur = 0;          // ... into d_ulist[ul_cur]
  int32_t sate_since = -1;     // first round that marked sated vertices (-1: none yet this run)
  bool park_failed = false;    // slot 2 could not be allocated: no unfiltered pull under liveness
};

// Everything the plan reads, gathered from the context in one place.
struct RoundFacts {
  int64_t n = 0, n_alloc = 0, nloc = 0, nnz = 0;
  int32_t m = 0, words = 0, round = 0;
  gp_config cfg{};
  // the last round's counters (global), and the messages held so far
  uint64_t prev_new_bits = 0, prev_receivers = 0, prev_next_arcs = 0, held_bits = 0;
  // this round's injection: out-degree sum of its origins, (round, origin) groups
  uint64_t inj_arcs = 0;
  int64_t inj_groups = 0;
  int32_t last_inject_round = -1;
  bool local = false;             // vertex-partitioned context (local ids != global ids)
  bool liveness_active = false;
  bool alive_on = false;          // the round builds the next alive set
  bool alive_now = false;         // this round's alive set is complete and may narrow targets
  bool have_cml = false, have_lm = false, have_lmw = false, have_ldone = false;   // the buffers exist
  bool have_ld_cand = false;      // the per-line rule has candidates (n_ld_cand > 0)
  // the accumulator rows' offset in this round's slot buffer, in rows (0: not
  // addressable as its rows, or past int32: no degree-split round)
  int64_t acc_row = 0;
  int32_t ld_env = -1, lp_env = -1;   // GP_LINE_DONE / GP_LINE_PACK at gp_create: 0 off, 1 on, -1 by size
  // the lazily allocated buffers may be used (the caller clears these when
  // an allocation the plan asked for fails, and plans again)
  bool can_park = true, can_list = true;
  RoundCarry carry;
  // lossy links: every arc may drop this round's lines
  bool lossy = false;
};

// Which kernel pulls this round, and what its pre- and post-passes need to know.
enum PullKernel { PULL_NONE, PULL_FLAT, PULL_LIST, PULL_RECEIVER, PULL_RECORD,
                  PULL_LOSSY /* k_expand_lossy: frontier rows through the per-arc draw (lossy.hip) */ };
struct PullChoice {
  PullKernel kernel = PULL_NONE;
  int mode = 0;                   // k_expand's MODE (flat: SCAN_FILTERED / SCAN_UNFILTERED)
  bool masked = false;            // the per-arc mask is built first (k_arcmask)
  bool lines = false;             // the senders' line masks are read (SCAN_LINES, hub chunks) ...
  bool lm_from_commits = false;   // ... as the last round's commits wrote them (else k_mklm builds them)
};

struct RoundPlan {
  bool mode_push = false;     // direction of the round
  double push_est = 0.0;      // sender arcs the direction estimate saw
  bool early_exit = false;    // coverage-checked scan
  bool near_done = false;     // early exit, no liveness, half the messages held
  bool sate = false;          // receivers that end the round with every alive message are marked sated
  // a pull round's switches (all false in a push round)
  bool unfiltered = false;    // the pull skips the activity check
  bool arc_mask = false;      // the filtered pull reads the per-arc mask
  bool sum = false;           // the probes read the summary level first
  bool prefilter = false;     // the filtered pull probes low-degree in-lists lane-parallel
  bool split = false;         // degree-split round: low-degree senders push, receivers probe a prefix
  bool cml_read = false, cml_write = false;   // compact Message-List records gathered / written
  bool lines = false;         // the senders' line masks are offered to the pull (ExpandArgs.lm)
  bool lm_write = false;      // the commits write the next round's line masks
  bool dnb = false;           // the pull reads the done bitmap (done in-neighbours)
  bool narrow_pr = false;     // W = 8 / 16 near-done pull on the per-receiver kernel
  // aliased Message-Lists: a receiver that completes its
  // component in a W = 64 early-exit pull writes no row; sp = SLOT_CMASK says
  // its Message-List is cmask[midx[v]].  dprobe: the pull probes the done
  // bitmap for every arc it scans (a receiver with any done in-neighbour takes
  // its target and gathers nothing, so an aliased row is never gathered);
  // alias: its complete receivers alias
  bool alias = false, dprobe = false;
  bool ulist_read = false;    // the waves take their receivers from the last round's list
  bool ulist_emit = false;    // the survivors are appended to the next list
  bool line_done = false;     // targets seeded from the complete lines of a top in-neighbour
  bool line_pack = false;     // the packed gather (SCAN_PACK)
  PullChoice pull;
  // the lazily allocated buffers this plan relies on: slot 2 (parked rows), the receiver lists
  bool need_park_slot = false, need_ulist = false;
  // gp_round_stats.scan
  int scan() const {
    if (mode_push) return 0;
    const bool ran_lines = (pull.mode & SCAN_LINES) != 0;
    return (unfiltered ? 2 : arc_mask ? 1 : prefilter ? 3 : 0) | (cml_read ? 4 : 0) | (ran_lines ? 8 : 0) |
           (ran_lines && pull.lm_from_commits ? 16 : 0) | (split ? 32 : 0) | (dprobe ? 64 : 0) |
           (ulist_read ? 128 : 0);
  }
};

// last round's receivers + this round's injected origins send this round
inline double round_senders(const RoundFacts& f) { return (double)f.prev_receivers + (double)f.inj_groups; }
// (nearly) every vertex is a sender: >= unfiltered_pct % of n
inline bool all_send(const RoundFacts& f) {
  return f.cfg.unfiltered_pct > 0 && round_senders(f) * 100.0 >= (double)f.cfg.unfiltered_pct * (double)f.n;
}

// The pull of the round, were it one: every switch and the kernel.  `p`
// arrives with the direction-independent fields set.
inline RoundPlan plan_pull(const RoundFacts& f, RoundPlan p) {
  const gp_config& cfg = f.cfg;
  const int W = f.words;
  const double n = (double)f.n, nm = (double)f.n * (double)f.m;
  const bool single_ctx = !f.local && f.nloc == f.n_alloc;   // one context: local ids are global ids
  const bool half_held = (double)f.held_bits * 2.0 >= nm;
  const bool ee = p.early_exit;
  const double senders = round_senders(f);
  // unfiltered pull when (nearly) every vertex is a sender: last round's
  // receivers + this round's injected origins >= unfiltered_pct % of n.  With
  // liveness a crashed vertex's Message-List may hold bits it never sent, so
  // the down vertices' rows are parked first (k_park; one vertex set per
  // context, hence not in a vertex partition, whose ghosts' rows are frontiers)
  // (slot 2 out of memory: stay filtered)
  p.unfiltered = all_send(f) && (!f.liveness_active || (!f.local && f.can_park));
  p.need_park_slot = p.unfiltered && f.liveness_active;
  // done in-neighbours: without liveness a receiver with an
  // in-neighbour that held its whole component at the end of the last round
  // receives exactly cmask & ~seen.  Pull rounds of the per-receiver kernel
  // once most messages are held (before that hardly any vertex is done, and
  // the probes only cost); the done bitmap comes with the activity bitmap (one
  // context: seenpop and done_at share the vertex index)
  // Narrow rows (W = 8 / 16: the message shards of 4- and 8-GPU jobs) take the
  // per-receiver kernel instead of the flat one in the thin late rounds (under
  // 1/NARROW_ND_DIV of the n x m bits still missing): its receivers go
  // eight / sixteen per wave step (dnb_groups, gather_groups), while the flat
  // kernel keeps the dense rounds, the last of which leaves a shard ~1 % short
  // (profiles/r06_ab_narrow_nd.txt; a threshold of n*m/4 or n*m/2 was no
  // better, n*m/2 slower: LEDGER.md "Receiver groups for the message shards")
  p.narrow_pr = (W == 8 || W == 16) && W <= cfg.flat_max_words && ee && !f.liveness_active && single_ctx &&
                (nm - (double)f.held_bits) * NARROW_ND_DIV < nm;
  // With liveness the done bitmap is the sated marks (up and sated: holds every
  // alive message of its component; k_mkbits): a receiver with such an
  // in-neighbour receives exactly cmask & F_r & ~seen, since every bit of it
  // lies in that neighbour's frontier (it sent everything older while both were
  // up, and crashes are final).  From the round after the first marking round.
  p.dnb = ee && single_ctx &&
          (f.liveness_active ? f.alive_now && W > cfg.flat_max_words && f.carry.sate_since >= 0 &&
                                   f.round > f.carry.sate_since
                             : (W > cfg.flat_max_words || p.narrow_pr) && half_held);
  // aliased Message-Lists (W = 64, no liveness, one context,
  // no compact records): in done-neighbour rounds receivers that complete
  // commit SLOT_CMASK instead of a 512-B row.  Once a run holds aliases every
  // pull probes the done bitmap for each arc it scans (a receiver with any
  // done in-neighbour takes its target, so no aliased row slot is gathered);
  // held bits only grow, so early exit and the done bitmap stay on.  The
  // first aliasing round reads rows written before any alias and needs no
  // probe (C4 round 4: 74.6 M arcs whose probe would sit in each pass's
  // dependent chain).  A push round first writes its aliased senders' rows
  // (k_unalias; profiles/r06_ab_alias.txt)
  const bool alias_ok = W == 64 && !f.liveness_active && single_ctx && cfg.compact_rows == 0 &&
                        W > cfg.flat_max_words;
  p.alias = p.dnb && alias_ok;
  p.dprobe = p.alias && f.carry.alias_active;
  // receiver lists (W = 64 early-exit pulls, one context):
  // once most messages are held, each pull appends the receivers that stay
  // neither done nor sated; a pull whose list is under a third of the
  // vertices launches waves for those alone, k_mkbits does every sender's
  // accounting and the receivers' fpop_next starts zeroed (C5 round 6: 1.26 M
  // receivers of 64 M vertices; profiles/r06_ab_lists_c5.txt)
  const bool list_ok = single_ctx && W == 64 && W > cfg.flat_max_words && cfg.compact_rows == 0 && ee;
  p.ulist_read = list_ok && f.carry.ulist_valid && f.carry.ulist_n * GP_ULIST_DIV < f.n_alloc;
  // filtered pull: probe every arc inside the scan, or build the per-arc mask
  // first (pays once the probes are many: senders >= arc_mask_permille of n)
  const bool mask_pays = !p.unfiltered && cfg.arc_mask_permille > 0 &&
                         senders * 1000.0 >= (double)cfg.arc_mask_permille * n;
  const bool probes = !p.unfiltered && !mask_pays;   // a filtered round that probes the activity bitmap per arc
  // summary probes: filtered rounds of overlays whose activity bitmap outgrows
  // an XCD's L2, while few enough vertices send that most summary bits are 0
  p.sum = probes && cfg.summary_min_n > 0 && f.n_alloc >= cfg.summary_min_n && senders * SUMMARY_RATIO <= n;
  // the scan modes of the done-probe and list variants are filtered and
  // unfiltered alone: the switches below belong to the other rounds
  if (!p.dprobe && !p.ulist_read) {
    p.arc_mask = mask_pays;
    // Message-List records (W = 64): written while the rows are sparse (last
    // round's receivers got <= CML_AVG_BITS new bits on average), read by a
    // filtered pull without early exit whose senders all wrote theirs (or their
    // dense bit) in the previous round.  Senders are exactly the vertices with
    // fpop != 0 under liveness too (a crash zeroes fpop), and a sender's record
    // mirrors its row, so records and full rows give the same OR.
    const bool cml_ok = f.have_cml && W == 64 && probes;
    const bool sparse = (double)f.prev_new_bits <=
                        CML_AVG_BITS * (double)(f.prev_receivers > 1 ? f.prev_receivers : 1);
    p.cml_read = cml_ok && f.carry.cml_written && !ee;
    p.cml_write = cml_ok && sparse;   // the kernels that write them
    // line masks (W = 64): a filtered pull without early exit reads its
    // senders' rows while they are still sparse; their zero 128-B lines are
    // skipped.  The kernel choice narrows this to the plain
    // per-receiver kernel (k_expand<64, SCAN_FILTERED | SCAN_LINES>)
    p.lines = W == 64 && f.have_lm && probes && !ee && f.n_alloc <= (int64_t(1) << 27);   // (u << 4) | lines
    // this round's 64-word pull commits write the next round's masks: one
    // context (ghosts' rows come from the exchange), per-receiver kernel, no
    // records; under liveness k_churn zeroes a crashing sender's nibble with
    // its fpop (round 4 of the build; k_mklm ran there until then)
    // (only sparse rounds: a line-mask round follows a round with few new bits,
    // and early-exit rounds would pay the commits' extra stores for nothing --
    // C4 rounds 3-4 +0.3 ms when every pull wrote them)
    p.lm_write = W == 64 && f.have_lmw && !ee && !f.local && !p.cml_read && !p.cml_write;
    // sparse filtered pull: the lane phase probes the in-lists of low-degree receivers
    p.prefilter = probes && cfg.prefilter_pct > 0 && senders * 100.0 < (double)cfg.prefilter_pct * n;
    // degree-split: a prefiltered per-receiver pull without
    // early exit (C4 / C5 round 1), one context, no compact Message-Lists:
    // senders of in-degree < split_deg push (few arcs: they are the
    // low-degree minority of a degree-biased sender set), receivers probe only
    // the gather-order prefix of bigger senders
    // Only while the senders are a sliver of the vertices (C4 / C5 round 1:
    // 0.1-0.4 %): the 512-message shards' round 2, prefiltered with 7-13 % of
    // the vertices sending, pushed 30-67 M low-degree arcs in 3.3-5.9 ms
    // against a 1.8-1.9 ms pull half (profiles/r04_split_cap.txt)
    // (accumulator rows as rows of this round's slot buffer: same allocation, same stride)
    p.split = cfg.split_deg > 0 && p.prefilter && !ee && single_ctx && !p.cml_read && !p.cml_write &&
              senders * 1000.0 < (double)cfg.split_max_permille * n && f.acc_row > 0;
  }
  // (only once the rounds thin out: last round's new bits under m/4 per
  // vertex -- C4 round 4's survivors, 7.6 M, would make no list worth reading,
  // and appending them cost the round 0.07 ms)
  // (lists out of memory: no lists)
  p.ulist_emit = list_ok && f.can_list && half_held && (double)f.prev_new_bits * 4.0 < nm && !p.arc_mask &&
                 !p.prefilter && !p.split && !p.cml_read && !p.cml_write && !p.lines;
  p.need_ulist = p.ulist_emit;
  // Complete lines of a top in-neighbour: the unfiltered
  // early-exit pulls of k_expand<64> that read no receiver list (an aliased
  // candidate of a done-probe round holds every line: no row is read), under
  // alias_ok's conditions.  By default only where it paid: once the
  // Message-Lists outgrow the Infinity Cache (n_alloc x 8W > 256 MiB: below
  // that the dense rounds are not HBM-bound) and before the done-neighbour
  // rounds (C4 round 3: 71.1 -> 47.6 GB of row bytes, 16.0 -> 14.5 ms; round
  // 4's row bytes fell by 21 % too, but the round, which waits on the
  // per-receiver chain, ran 0.07 ms slower: profiles/r09_ab_line_done.txt).
  // GP_LINE_DONE=1 turns it on in every eligible round whatever the size,
  // GP_LINE_DONE=0 off
  const bool ld_big = (double)f.n_alloc * 8.0 * (double)W > 256.0 * 1024.0 * 1024.0;
  const bool whole_rows = alias_ok && ee && p.unfiltered && !p.ulist_read;
  p.line_done = whole_rows && f.have_ldone && f.have_ld_cand && (f.ld_env < 0 ? ld_big && !p.dnb : f.ld_env == 1);
  // The packed gather: the same pulls -- k_expand<64>'s
  // unfiltered early-exit rounds without liveness, receiver list or done
  // probe.  By default under the per-line rule's size gate (the live lines
  // collapse to one under the spread order at W = 64, and nothing was measured
  // below that size) and before the done-neighbour rounds (the plain variant,
  // C4 round 3).  GP_LINE_PACK=1 turns it on in every eligible round whatever
  // the size, GP_LINE_PACK=0 off
  p.line_pack = whole_rows && !p.dprobe && (f.lp_env < 0 ? ld_big && !p.dnb : f.lp_env == 1);

  // the kernel
  PullChoice& k = p.pull;
  const auto built = [W](int mode) { return W >= expand_min_width(mode); };
  const bool unf = p.unfiltered;
  const int scan = unf ? SCAN_UNFILTERED : SCAN_FILTERED;
  // the flat kernel (built for W <= 32) up to flat_max_words, 16 by default:
  // W = 32 rows take the per-receiver kernel in every round, whose receiver
  // groups beat the flat kernel in the dense near-done rounds too
  // (profiles/r06_ab_w32_groups.txt), W = 8 / 16 in the thin late rounds
  const bool flat = W <= 32 && W <= cfg.flat_max_words && !p.narrow_pr;
  // early-exit rounds with alive sets (liveness) take the SCAN_ALIVE variants
  const bool alive_ee = f.alive_now && ee;
  const bool records = p.cml_read || p.cml_write;
  k.masked = !unf && !flat && p.arc_mask;
  k.lines = built(SCAN_FILTERED | SCAN_LINES) && p.lines && !flat && !k.masked && !unf && !records &&
            !p.prefilter && !alive_ee;
  k.lm_from_commits = k.lines && f.carry.lm_written;
  if (f.nloc > 0 && flat) {   // narrow rows: edge-parallel pull
    k.kernel = PULL_FLAT;
    k.mode = scan;
  } else if (p.ulist_read && built(scan | SCAN_LIST)) {   // receiver-list round: waves for the listed vertices
    k.kernel = PULL_LIST;
    k.mode = scan | SCAN_LIST | (alive_ee ? SCAN_ALIVE : p.dprobe ? SCAN_DPROBE : 0);
  } else if (f.nloc > 0 && unf) {
    k.kernel = PULL_RECEIVER;
    // The first aliasing round (alias without the done probe) runs the quads
    // variant (done-neighbour receivers four at a time, low in-degree ones two
    // at a time: profiles/r06_ab_alias_quads.txt), and so do the other
    // unfiltered pulls once most messages are held: near-done rounds without
    // liveness and, under liveness (parked rows), the alive early-exit pulls
    // from the round that starts with half the messages held (C5 rounds 4-5;
    // round 3, the dense one, keeps the plain alive variant:
    // profiles/r06_ab_quads_c5.txt, r06_ab_gather_pairs.txt)
    if (alive_ee && built(scan | SCAN_ALIVE))
      k.mode = scan | SCAN_ALIVE | (half_held && built(scan | SCAN_ALIVE | SCAN_QUADS) ? SCAN_QUADS : 0);
    else if (p.dprobe && built(scan | SCAN_DPROBE)) k.mode = scan | SCAN_DPROBE;   // (done-probe rounds)
    else if ((p.alias || p.near_done) && built(scan | SCAN_QUADS)) k.mode = scan | SCAN_QUADS;
    else k.mode = scan;
    // the packed gather: the plain pull, its serial loop's
    // lanes dealt out over the live lines.  (Not the quads variant, whose
    // receivers of in-degree <= 32 go through gather_pairs: with the serial
    // loop alone packed it took 76 VGPRs against 72 and C4 round 4 ran 6.42 ->
    // 7.14 ms, profiles/r11_ab_line_pack.txt)
    if (p.line_pack && k.mode == scan && built(scan | SCAN_PACK)) k.mode |= SCAN_PACK;
  } else if (f.nloc > 0) {
    k.kernel = PULL_RECEIVER;
    const int pre = p.prefilter ? SCAN_PRE : SCAN_FILTERED;
    if (p.dprobe && built(scan | SCAN_DPROBE)) {
      k.mode = scan | SCAN_DPROBE;
    } else if (k.masked) {
      k.mode = SCAN_MASKED;
    } else if (records && built(pre | SCAN_CML)) {   // compact Message-Lists read and / or written
      if (p.cml_read && !ee && !p.prefilter && !f.alive_now) k.kernel = PULL_RECORD;
      else k.mode = pre | SCAN_CML;
    } else if (alive_ee && built(pre | SCAN_ALIVE)) {
      k.mode = pre | SCAN_ALIVE;
    } else if (k.lines) {
      k.mode = SCAN_FILTERED | SCAN_LINES;
    } else {
      k.mode = pre;
    }
  }
  return p;
}

// The round's plan.  No side effects: the same facts give the same plan.
inline RoundPlan plan_round(const RoundFacts& f) {
  // Lossy links: one kernel family and none of the switches,
  // whatever the other facts say.  Push, early-exit target narrowing, the
  // done-neighbour rules, aliases, line masks, records, the degree split,
  // receiver lists, sating and parking each rest on "a neighbour's whole
  // Message-List was sent to me", which a dropped line breaks
  if (f.lossy) {
    RoundPlan p;
    p.pull.kernel = PULL_LOSSY;
    return p;
  }
  const gp_config& cfg = f.cfg;
  const double nm = (double)f.n * (double)f.m;
  const bool half_held = (double)f.held_bits * 2.0 >= nm;
  RoundPlan base;
  // early exit pays once frontier rows are dense: >= m/16 new bits per vertex last round
  // or once most messages are held: receivers then miss a few words at most, and
  // the word skip loads only those (under churn the component targets may be
  // out of reach -- a message cut off by crashes -- so the done-skip alone
  // leaves nearly every receiver scanning whole rows)
  const double ee_div = f.words <= 8 ? GP_EE_DIV_NARROW : GP_EE_DIV;
  base.early_exit = cfg.early_exit != 0 && ((double)f.prev_new_bits * ee_div >= nm || half_held);
  // (not with liveness: messages cut off by crashes keep the component targets
  // out of reach, receivers scan to the end and want every row in flight --
  // C5 rounds 5-6 56.8 -> 64.3 ms with the switch on)
  base.near_done = base.early_exit && !f.liveness_active && half_held;
  // sated vertices (churn): with no injection left, a receiver that ends the
  // round holding every alive message of its component never receives again
  base.sate = f.alive_now && base.early_exit && f.round >= f.last_inject_round;
  const double est = (double)((f.round == 0 ? 0ull : f.prev_next_arcs) + f.inj_arcs);
  base.push_est = est;
  const RoundPlan pull = plan_pull(f, base);
  // direction: push when the senders' arcs are a small share of all arcs
  // narrow rows push at a lower ratio: the pull's per-arc scan does not
  // shrink with W, the push's row words do (k_apply_lanes, k_mkneed)
  // (early rounds only: late rounds' pulls skip the done receivers, which the
  // estimate does not see -- the 512-message shard's round 6 pulls in 0.27 ms
  // and pushes in 0.72)
  const bool narrow = f.words <= GP_NARROW_PUSH_MAXW && !half_held;
  const double ratio = cfg.push_ratio * (narrow ? GP_NARROW_PUSH_SCALE : 1.0);
  const bool push = cfg.push_ratio > 0.0 && est * ratio <= (double)f.nnz;
  // narrow rows: a round that pushes only because of the narrow scale pulls
  // as a degree-split round instead (its prefix probes are a fraction of the
  // arcs, its push half only the low-degree senders' arcs) -- but only when
  // the pull would be one (records: W = 64 only; 512-message shard 14.62 ->
  // 14.16 ms, profiles/r04_ab_shards.txt).  (A round whose unfiltered pull
  // only the missing parking slot forbids is none of these: it pushes)
  const bool park_veto = all_send(f) && !pull.unfiltered;
  const bool narrow_split = push && f.words < 64 && pull.split && !park_veto && est * cfg.push_ratio > (double)f.nnz;
  if (!push || narrow_split) return pull;
  base.mode_push = true;
  return base;
}

}  // namespace gp
