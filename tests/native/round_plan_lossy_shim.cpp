// round_plan_lossy_shim.cpp -- test-only C wrapper around csrc/round_plan.h
// for tests/test_round_plan_lossy.py: plan_round with RoundFacts::lossy set
// from a column of its own.  The flat structs and facts_of are
// round_plan_shim.cpp's, included as they are (that file fills a RoundFacts
// without the field, which is what this one is compared with).
#include "round_plan_shim.cpp"

extern "C" {

// out[i] = plan_round(in[i] with lossy = lossy[i]) for i in [0, count)
void rpl_plan(const FlatFacts* in, const long long* lossy, FlatPlan* out, long long count) {
  for (long long i = 0; i < count; ++i) {
    gp::RoundFacts f = facts_of(in[i]);
    f.lossy = lossy[i] != 0;
    const gp::RoundPlan p = gp::plan_round(f);
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

long long rpl_pull_lossy() { return (long long)gp::PULL_LOSSY; }

}  // extern "C"
