// round_plan_shim.cpp -- test-only C wrapper around csrc/round_plan.h (host
// code, no HIP), compiled with g++ by tests/test_round_plan.py so the round's
// direction, scan mode and pull kernel are checked on the CPU.  Facts and plan
// cross as flat structs of 8-byte fields (a numpy structured array each).
#include "round_plan.h"

extern "C" {

struct FlatFacts {
  int64_t n, n_alloc, nloc, nnz, m, words, round;
  int64_t prev_new_bits, prev_receivers, prev_next_arcs, held_bits, inj_arcs, inj_groups, last_inject_round;
  int64_t local, liveness_active, alive_on, alive_now;
  int64_t have_cml, have_lm, have_lmw, have_ldone, have_ld_cand;
  int64_t acc_row, ld_env, lp_env, can_park, can_list;
  // the carry
  int64_t cml_written, lm_written, alias_active, ulist_valid, ulist_n, ul_cur, sate_since, park_failed;
  // the configuration fields the plan reads
  double push_ratio;
  int64_t early_exit, arc_mask_permille, prefilter_pct, compact_rows, unfiltered_pct, flat_max_words,
      summary_min_n, split_deg, split_max_permille;
};

struct FlatPlan {
  int64_t mode_push, early_exit, near_done, sate, unfiltered, arc_mask, sum, prefilter, split, cml_read, cml_write,
      lines, lm_write, dnb, narrow_pr, alias, dprobe, ulist_read, ulist_emit, line_done, line_pack;
  int64_t kernel, mode, mode_min_width, k_masked, k_lines, k_lm_from_commits;
  int64_t need_park_slot, need_ulist, scan;
  double push_est;
};

static gp::RoundFacts facts_of(const FlatFacts& a) {
  gp::RoundFacts f;
  f.n = a.n; f.n_alloc = a.n_alloc; f.nloc = a.nloc; f.nnz = a.nnz;
  f.m = (int32_t)a.m; f.words = (int32_t)a.words; f.round = (int32_t)a.round;
  f.prev_new_bits = (uint64_t)a.prev_new_bits; f.prev_receivers = (uint64_t)a.prev_receivers;
  f.prev_next_arcs = (uint64_t)a.prev_next_arcs; f.held_bits = (uint64_t)a.held_bits;
  f.inj_arcs = (uint64_t)a.inj_arcs; f.inj_groups = a.inj_groups; f.last_inject_round = (int32_t)a.last_inject_round;
  f.local = a.local != 0; f.liveness_active = a.liveness_active != 0;
  f.alive_on = a.alive_on != 0; f.alive_now = a.alive_now != 0;
  f.have_cml = a.have_cml != 0; f.have_lm = a.have_lm != 0; f.have_lmw = a.have_lmw != 0;
  f.have_ldone = a.have_ldone != 0; f.have_ld_cand = a.have_ld_cand != 0;
  f.acc_row = a.acc_row; f.ld_env = (int32_t)a.ld_env; f.lp_env = (int32_t)a.lp_env;
  f.can_park = a.can_park != 0; f.can_list = a.can_list != 0;
  f.carry.cml_written = a.cml_written != 0; f.carry.lm_written = a.lm_written != 0;
  f.carry.alias_active = a.alias_active != 0; f.carry.ulist_valid = a.ulist_valid != 0;
  f.carry.ulist_n = a.ulist_n; f.carry.ul_cur = (int32_t)a.ul_cur; f.carry.sate_since = (int32_t)a.sate_since;
  f.carry.park_failed = a.park_failed != 0;
  f.cfg.push_ratio = a.push_ratio;
  f.cfg.early_exit = (int32_t)a.early_exit; f.cfg.arc_mask_permille = (int32_t)a.arc_mask_permille;
  f.cfg.prefilter_pct = (int32_t)a.prefilter_pct; f.cfg.compact_rows = (int32_t)a.compact_rows;
  f.cfg.unfiltered_pct = (int32_t)a.unfiltered_pct; f.cfg.flat_max_words = (int32_t)a.flat_max_words;
  f.cfg.summary_min_n = a.summary_min_n; f.cfg.split_deg = (int32_t)a.split_deg;
  f.cfg.split_max_permille = (int32_t)a.split_max_permille;
  return f;
}

// out[i] = plan_round(in[i]) for i in [0, count)
void rp_plan(const FlatFacts* in, FlatPlan* out, long long count) {
  for (long long i = 0; i < count; ++i) {
    const gp::RoundPlan p = gp::plan_round(facts_of(in[i]));
    FlatPlan& o = out[i];
    o.mode_push = p.mode_push; o.early_exit = p.early_exit; o.near_done = p.near_done; o.sate = p.sate;
    o.unfiltered = p.unfiltered; o.arc_mask = p.arc_mask; o.sum = p.sum; o.prefilter = p.prefilter;
    o.split = p.split; o.cml_read = p.cml_read; o.cml_write = p.cml_write; o.lines = p.lines;
    o.lm_write = p.lm_write; o.dnb = p.dnb; o.narrow_pr = p.narrow_pr; o.alias = p.alias; o.dprobe = p.dprobe;
    o.ulist_read = p.ulist_read; o.ulist_emit = p.ulist_emit; o.line_done = p.line_done; o.line_pack = p.line_pack;
    o.kernel = (int64_t)p.pull.kernel; o.mode = p.pull.mode; o.mode_min_width = gp::expand_min_width(p.pull.mode);
    o.k_masked = p.pull.masked; o.k_lines = p.pull.lines; o.k_lm_from_commits = p.pull.lm_from_commits;
    o.need_park_slot = p.need_park_slot; o.need_ulist = p.need_ulist; o.scan = p.scan();
    o.push_est = p.push_est;
  }
}

long long rp_sizes(int which) { return which == 0 ? (long long)sizeof(FlatFacts) : (long long)sizeof(FlatPlan); }

}  // extern "C"
