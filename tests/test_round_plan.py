"""The round's plan (csrc/round_plan.h) on the CPU: direction, scan mode, every
per-round switch of the pull and the k_expand variant, as a pure function of
plain numbers.

driver.hip's launch_expand gathers the facts and enqueues what plan_round
says; this test drives plan_round, compiled with g++ through a test-only shim
(tests/native/round_plan_shim.cpp):
 - each gate at its threshold and one unit off it, the expected side read from
   launch_expand / choose_pull of the commit before the planner existed (the
   inequality is quoted at each case);
 - a sweep over every combination of the boolean facts and every row width,
   for what that code guaranteed only by the order of its statements;
 - a replay of the runs recorded with that commit's library
   (tests/golden/round_plan_trace.json, tests/round_trace.py): the planner must
   choose every round's recorded `mode` and `scan`.
The plan only schedules the expansion, whose result is the reference's send
loop over every link (Peer.py:402-404) whatever the plan.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "round_plan_shim.cpp")
TRACE = os.path.join(ROOT, "tests", "golden", "round_plan_trace.json")

I_FACTS = ("n n_alloc nloc nnz m words round prev_new_bits prev_receivers prev_next_arcs held_bits inj_arcs "
           "inj_groups last_inject_round local liveness_active alive_on alive_now have_cml have_lm have_lmw "
           "have_ldone have_ld_cand acc_row ld_env lp_env can_park can_list cml_written lm_written alias_active "
           "ulist_valid ulist_n ul_cur sate_since park_failed").split()
CFG_I = ("early_exit arc_mask_permille prefilter_pct compact_rows unfiltered_pct flat_max_words summary_min_n "
         "split_deg split_max_permille").split()
FACTS = np.dtype([(k, "<i8") for k in I_FACTS] + [("push_ratio", "<f8")] + [(k, "<i8") for k in CFG_I])
FLAGS = ("mode_push early_exit near_done sate unfiltered arc_mask sum prefilter split cml_read cml_write lines "
         "lm_write dnb narrow_pr alias dprobe ulist_read ulist_emit line_done line_pack").split()
PLAN = np.dtype([(k, "<i8") for k in FLAGS + "kernel mode mode_min_width k_masked k_lines k_lm_from_commits "
                 "need_park_slot need_ulist scan".split()] + [("push_est", "<f8")])
PULL_NONE, PULL_FLAT, PULL_LIST, PULL_RECEIVER, PULL_RECORD = range(5)
# the switches of a pull round: a push round has none (early_exit, near_done and sate go to both)
PULL_FLAGS = FLAGS[4:]


@pytest.fixture(scope="module")
def rp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("round_plan") / "libround_plan_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, SHIM,
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.rp_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    lib.rp_plan.restype = None
    lib.rp_sizes.restype = ctypes.c_longlong
    assert lib.rp_sizes(0) == FACTS.itemsize and lib.rp_sizes(1) == PLAN.itemsize
    return lib


def test_header_stands_alone(tmp_path):
    """plain C++17 without HIP: g++ -Wall compiles the header on its own"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "round_plan.h"\nint main() { return gp::plan_round(gp::RoundFacts{}).mode_push; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o",
                           str(tmp_path / "alone")])
    text = open(os.path.join(CSRC, "round_plan.h"), encoding="utf-8").read()
    assert [l for l in text.splitlines() if l.startswith("#include")] == \
        ["#include <cstdint>", '#include "../../include/gossip_capi.h"']


def plan_many(rp, facts):
    facts = np.ascontiguousarray(facts, FACTS)
    out = np.zeros(facts.shape, PLAN)
    rp.rp_plan(facts.ctypes.data, out.ctypes.data, facts.size)
    return out


# a W = 64 pull round of one context: 1000 vertices, 4096 messages, the
# library's default configuration but push_ratio = 0 (always pull)
BASE = dict(n=1000, n_alloc=1000, nloc=1000, nnz=100_000, m=4096, words=64, round=3, last_inject_round=0,
            have_lm=1, have_lmw=1, have_ldone=1, have_ld_cand=1, acc_row=1000, ld_env=-1, lp_env=-1,
            can_park=1, can_list=1, sate_since=-1, push_ratio=0.0, early_exit=1, arc_mask_permille=0,
            prefilter_pct=20, compact_rows=0, unfiltered_pct=90, flat_max_words=16, summary_min_n=1 << 25,
            split_deg=128, split_max_permille=10)
NM = 1000 * 4096
W8 = dict(m=512, words=8)   # a 512-message shard: nm = 512,000
NM8 = 1000 * 512
BIG = 524_288   # n_alloc x 8 x 64 bytes = 256 MiB


def plan(rp, **kw):
    f = np.zeros(1, FACTS)
    for k, v in {**BASE, **kw}.items():
        f[k] = v
    return {k: (float if k == "push_est" else int)(plan_many(rp, f)[0][k]) for k in PLAN.names}


def _dense(n):
    """an unfiltered early-exit round before the half-held rounds, n vertices"""
    return dict(n=n, n_alloc=n, nloc=n, acc_row=n, prev_receivers=n, prev_new_bits=n * 4096 // 16)


# (gate, facts, plan field, expected value): at the threshold, then one unit off
GATES = [
    # early_exit_now = cfg.early_exit != 0 && (prev_new_bits * ee_div >= n * m || held_bits * 2 >= n * m),
    # ee_div = words <= 8 ? GP_EE_DIV_NARROW (64) : GP_EE_DIV (16)
    ("ee dense", dict(prev_new_bits=NM // 16), "early_exit", 1),
    ("ee dense", dict(prev_new_bits=NM // 16 - 1), "early_exit", 0),
    ("ee dense W<=8", dict(W8, prev_new_bits=NM8 // 64), "early_exit", 1),
    ("ee dense W<=8", dict(W8, prev_new_bits=NM8 // 64 - 1), "early_exit", 0),
    ("ee dense W=16 keeps m/16", dict(m=1024, words=16, prev_new_bits=1000 * 1024 // 16 - 1), "early_exit", 0),
    # held_bits * 2.0 >= n * m
    ("half held", dict(held_bits=NM // 2), "early_exit", 1),
    ("half held", dict(held_bits=NM // 2 - 1), "early_exit", 0),
    ("half held: near_done", dict(held_bits=NM // 2), "near_done", 1),
    ("half held: near_done", dict(held_bits=NM // 2 - 1, prev_new_bits=NM), "near_done", 0),
    # unfiltered_now = !mode_push && unfiltered_pct > 0 && senders * 100.0 >= unfiltered_pct * n,
    # senders = prev_receivers + inj_groups_at(r)
    ("unfiltered_pct", dict(prev_receivers=890, inj_groups=10), "unfiltered", 1),
    ("unfiltered_pct", dict(prev_receivers=889, inj_groups=10), "unfiltered", 0),
    # arc_mask_now = !mode_push && !unfiltered_now && arc_mask_permille > 0 && senders * 1000.0 >= arc_mask_permille * n
    ("arc_mask_permille", dict(arc_mask_permille=500, prev_receivers=500), "arc_mask", 1),
    ("arc_mask_permille", dict(arc_mask_permille=500, prev_receivers=499), "arc_mask", 0),
    # prefilter_now = ... && prefilter_pct > 0 && senders * 100.0 < prefilter_pct * n
    ("prefilter_pct", dict(prev_receivers=200), "prefilter", 0),
    ("prefilter_pct", dict(prev_receivers=199), "prefilter", 1),
    # split_now = split_deg > 0 && prefilter_now && !early_exit_now && ... && senders * 1000.0 < split_max_permille * n
    ("split_max_permille", dict(prev_receivers=10), "split", 0),
    ("split_max_permille", dict(prev_receivers=9), "split", 1),
    # sum_now: summary_min_n > 0 && n_alloc >= summary_min_n && senders * SUMMARY_RATIO (256) <= n
    ("summary_min_n", dict(summary_min_n=1000, prev_receivers=3), "sum", 1),
    ("summary_min_n", dict(summary_min_n=1001, prev_receivers=3), "sum", 0),
    ("SUMMARY_RATIO", dict(n=1024, n_alloc=1024, nloc=1024, summary_min_n=1, prev_receivers=4), "sum", 1),
    ("SUMMARY_RATIO", dict(n=1024, n_alloc=1024, nloc=1024, summary_min_n=1, prev_receivers=5), "sum", 0),
    # mode_push = push_ratio > 0.0 && est * ratio <= nnz, est = (r == 0 ? 0 : prev_next_arcs) + inj_arcs,
    # ratio = push_ratio * (words <= GP_NARROW_PUSH_MAXW (16) && held_bits * 2 < n * m ? GP_NARROW_PUSH_SCALE (0.25) : 1)
    ("push", dict(push_ratio=100.0, prev_next_arcs=900, inj_arcs=100), "mode_push", 1),
    ("push", dict(push_ratio=100.0, prev_next_arcs=901, inj_arcs=100), "mode_push", 0),
    ("push: round 0 counts the injection alone", dict(push_ratio=100.0, round=0, prev_next_arcs=5000, inj_arcs=1000),
     "mode_push", 1),
    ("push, narrow scale", dict(W8, push_ratio=100.0, prev_next_arcs=4000, prev_receivers=500), "mode_push", 1),
    ("push, narrow scale", dict(W8, push_ratio=100.0, prev_next_arcs=4001, prev_receivers=500), "mode_push", 0),
    ("push, narrow rows half held: no scale", dict(W8, push_ratio=100.0, prev_next_arcs=1001, held_bits=NM8 // 2),
     "mode_push", 0),
    ("push, narrow rows half held: no scale", dict(W8, push_ratio=100.0, prev_next_arcs=1001, held_bits=NM8 // 2 - 1,
                                                   prev_receivers=500), "mode_push", 1),
    # narrow_split = mode_push && pull_splits && est * push_ratio > nnz: the round pulls as a degree-split round
    ("narrow split", dict(W8, push_ratio=100.0, prev_next_arcs=1001, prev_receivers=9), "split", 1),
    ("narrow split", dict(W8, push_ratio=100.0, prev_next_arcs=1001, prev_receivers=9), "mode_push", 0),
    ("narrow split", dict(W8, push_ratio=100.0, prev_next_arcs=1000, prev_receivers=9), "mode_push", 1),
    ("narrow split: the pull would not split", dict(W8, push_ratio=100.0, prev_next_arcs=1001, prev_receivers=10),
     "mode_push", 1),
    # narrow_pr_now = (words == 8 || words == 16) && words <= flat_max_words && early_exit_now && ... &&
    # (nm - held_bits) * NARROW_ND_DIV (16) < nm
    ("NARROW_ND_DIV", dict(W8, held_bits=NM8 - NM8 // 16), "narrow_pr", 0),
    ("NARROW_ND_DIV", dict(W8, held_bits=NM8 - NM8 // 16 + 1), "narrow_pr", 1),
    ("NARROW_ND_DIV: the kernel", dict(W8, held_bits=NM8 - NM8 // 16), "kernel", PULL_FLAT),
    ("NARROW_ND_DIV: the kernel", dict(W8, held_bits=NM8 - NM8 // 16 + 1), "kernel", PULL_RECEIVER),
    # sparse = prev_new_bits <= CML_AVG_BITS (16) * max(prev_receivers, 1); cml_write_now = ok && sparse && ...
    ("CML_AVG_BITS", dict(have_cml=1, compact_rows=1, prev_receivers=10, prev_new_bits=160), "cml_write", 1),
    ("CML_AVG_BITS", dict(have_cml=1, compact_rows=1, prev_receivers=10, prev_new_bits=161), "cml_write", 0),
    ("CML_AVG_BITS: no receiver", dict(have_cml=1, compact_rows=1, prev_new_bits=16), "cml_write", 1),
    # ulist_read_now = list_ok && ulist_valid && ulist_n * GP_ULIST_DIV (3) < n_alloc
    ("ulist_n * 3 < n_alloc", dict(n=999, n_alloc=999, nloc=999, held_bits=999 * 4096, ulist_valid=1, ulist_n=333),
     "ulist_read", 0),
    ("ulist_n * 3 < n_alloc", dict(n=999, n_alloc=999, nloc=999, held_bits=999 * 4096, ulist_valid=1, ulist_n=332),
     "ulist_read", 1),
    ("no list left by the last round", dict(held_bits=NM, ulist_valid=0, ulist_n=0), "ulist_read", 0),
    # ulist_emit_now = list_ok && held_bits * 2 >= n * m && prev_new_bits * 4.0 < n * m && ...
    ("list emit", dict(held_bits=NM // 2, prev_receivers=500, prev_new_bits=NM // 4), "ulist_emit", 0),
    ("list emit", dict(held_bits=NM // 2, prev_receivers=500, prev_new_bits=NM // 4 - 1), "ulist_emit", 1),
    ("list emit: not half held", dict(held_bits=NM // 2 - 1, prev_receivers=500, prev_new_bits=NM // 4 - 1), "ulist_emit", 0),
    # ld_big = n_alloc * 8.0 * words > 256.0 * 1024.0 * 1024.0;
    # line_done_now = ... && (ld_env < 0 ? ld_big && !dnb_now : ld_env == 1); line_pack_now likewise with lp_env
    ("256 MiB", _dense(BIG), "line_done", 0),
    ("256 MiB", _dense(BIG + 1), "line_done", 1),
    ("256 MiB", _dense(BIG), "line_pack", 0),
    ("256 MiB", _dense(BIG + 1), "line_pack", 1),
    ("256 MiB: the packed variant", _dense(BIG + 1), "mode", 2 | 512),
    ("256 MiB: the plain variant", _dense(BIG), "mode", 2),
    ("GP_LINE_DONE=0", dict(_dense(BIG + 1), ld_env=0), "line_done", 0),
    ("GP_LINE_DONE=0 leaves the packed gather", dict(_dense(BIG + 1), ld_env=0), "line_pack", 1),
    ("GP_LINE_DONE=1", dict(_dense(BIG), ld_env=1), "line_done", 1),
    ("GP_LINE_DONE=1 leaves the packed gather", dict(_dense(BIG), ld_env=1), "line_pack", 0),
    ("GP_LINE_PACK=0", dict(_dense(BIG + 1), lp_env=0), "line_pack", 0),
    ("GP_LINE_PACK=0 leaves the line rule", dict(_dense(BIG + 1), lp_env=0), "line_done", 1),
    ("GP_LINE_PACK=1", dict(_dense(BIG), lp_env=1), "line_pack", 1),
    ("GP_LINE_PACK=1 leaves the line rule", dict(_dense(BIG), lp_env=1), "line_done", 0),
    ("by size: not in done-neighbour rounds", dict(_dense(BIG + 1), held_bits=(BIG + 1) * 2048), "line_done", 0),
    ("by size: not in done-neighbour rounds", dict(_dense(BIG + 1), held_bits=(BIG + 1) * 2048), "line_pack", 0),
    ("GP_LINE_DONE=1: in done-neighbour rounds too", dict(_dense(BIG), held_bits=BIG * 2048, ld_env=1), "line_done", 1),
    ("GP_LINE_PACK=1: the flag, but the quads variant runs", dict(_dense(BIG), held_bits=BIG * 2048, lp_env=1),
     "mode", 2 | 256),
    # lines_now = words == 64 && d_lm && ... && n_alloc <= (int64_t(1) << 27)
    ("line masks: (u << 4) | lines", dict(n=1 << 27, n_alloc=1 << 27, nloc=1 << 27, prev_receivers=1 << 25), "lines", 1),
    ("line masks: (u << 4) | lines", dict(n=(1 << 27) + 1, n_alloc=(1 << 27) + 1, nloc=(1 << 27) + 1,
                                           prev_receivers=1 << 25), "lines", 0),
    # dnb_now under liveness: ... && sate_since >= 0 && round > sate_since
    ("round > sate_since", dict(liveness_active=1, alive_on=1, alive_now=1, held_bits=NM, sate_since=3, round=4), "dnb", 1),
    ("round > sate_since", dict(liveness_active=1, alive_on=1, alive_now=1, held_bits=NM, sate_since=3, round=3), "dnb", 0),
    ("no sated vertex yet", dict(liveness_active=1, alive_on=1, alive_now=1, held_bits=NM, sate_since=-1, round=4), "dnb", 0),
    # a.sate = alive_now(c) && early_exit_now && round >= last_inject_round
    ("sate", dict(liveness_active=1, alive_on=1, alive_now=1, held_bits=NM, last_inject_round=3), "sate", 1),
    ("sate", dict(liveness_active=1, alive_on=1, alive_now=1, held_bits=NM, last_inject_round=4), "sate", 0),
]


@pytest.mark.parametrize("k", range(len(GATES)), ids=[f"{g[0]}-{g[2]}={g[3]}" for g in GATES])
def test_gate(rp, k):
    _, facts, field, want = GATES[k]
    assert plan(rp, **facts)[field] == want


def test_lazy_buffers(rp):
    """A plan names the lazily allocated buffer it relies on; with the
    capability cleared the round stays filtered / writes no list."""
    churn = dict(liveness_active=1, alive_on=1, alive_now=1, prev_receivers=950)
    p = plan(rp, **churn)
    assert p["unfiltered"] == 1 and p["need_park_slot"] == 1
    p = plan(rp, **churn, can_park=0)
    assert p["unfiltered"] == 0 and p["need_park_slot"] == 0 and p["scan"] & 3 == 0
    assert plan(rp, prev_receivers=950)["need_park_slot"] == 0   # (no liveness: nothing to park)
    late = dict(held_bits=NM, prev_receivers=500, prev_new_bits=10)
    p = plan(rp, **late)
    assert p["ulist_emit"] == 1 and p["need_ulist"] == 1
    p = plan(rp, **late, can_list=0)
    assert p["ulist_emit"] == 0 and p["need_ulist"] == 0


def _sweep_facts():
    """Every combination of the boolean facts x every row width, twice; the
    numeric facts and the configuration are drawn per case (fixed seed) from
    small sets with values on either side of every threshold."""
    bools = ("local liveness_active alive_on alive_now have_cml have_lm have_lmw have_ldone have_ld_cand can_park "
             "can_list cml_written lm_written alias_active ulist_valid").split()
    widths = np.array([1, 2, 4, 8, 16, 32, 64])
    nb = 1 << len(bools)
    idx = np.arange(nb * len(widths) * 2)
    f = np.zeros(idx.size, FACTS)
    for b, name in enumerate(bools):
        f[name] = (idx >> b) & 1
    W = widths[(idx >> len(bools)) % len(widths)]
    f["words"], f["m"] = W, 64 * W
    rng = np.random.default_rng(20)
    n = 1000
    nm = n * 64 * W

    def pick(*vals):
        return np.asarray(vals)[rng.integers(0, len(vals), idx.size)]

    def frac(num, den, off):   # nm * num / den + off, per case
        return nm * num // den + off
    f["n"] = f["n_alloc"] = n
    f["nloc"] = np.where(f["local"] != 0, n // 2, n)
    f["nnz"] = 100_000
    f["round"] = pick(0, 1, 5)
    f["last_inject_round"] = pick(0, 5, 6)
    k = rng.integers(0, 7, idx.size)
    f["held_bits"] = np.choose(k, [0 * nm, frac(1, 2, -1), frac(1, 2, 0), frac(15, 16, 0), frac(15, 16, 1), nm - 1, nm])
    k = rng.integers(0, 8, idx.size)
    f["prev_new_bits"] = np.choose(k, [0 * nm, frac(1, 64, -1), frac(1, 64, 0), frac(1, 16, -1), frac(1, 16, 0),
                                       frac(1, 4, -1), frac(1, 4, 0), 16 + 0 * nm])
    f["prev_receivers"] = pick(0, 1, 3, 4, 9, 10, 199, 200, 499, 500, 899, 900, 1000)
    f["inj_groups"] = pick(0, 0, 1)
    f["prev_next_arcs"] = pick(0, 1000, 1001, 4000, 4001, 50_000)
    f["inj_arcs"] = pick(0, 0, 1)
    f["acc_row"] = pick(0, n, 2 * n)
    f["ld_env"], f["lp_env"] = pick(-1, 0, 1), pick(-1, 0, 1)
    f["ulist_n"] = pick(0, 333, 334, 1000)
    f["sate_since"] = pick(-1, 0, 4, 5)
    f["push_ratio"] = pick(0.0, 100.0)
    f["early_exit"] = pick(0, 1, 1)
    f["arc_mask_permille"] = pick(0, 500)
    f["prefilter_pct"] = pick(0, 20)
    f["compact_rows"] = pick(0, 1)
    f["unfiltered_pct"] = pick(0, 90)
    f["flat_max_words"] = pick(0, 16, 32)
    f["summary_min_n"] = pick(0, 1000, 1001)
    f["split_deg"] = pick(0, 128)
    f["split_max_permille"] = pick(0, 10, 1000)
    return f


def test_sweep(rp):
    f = _sweep_facts()
    assert f.size > 400_000
    p = plan_many(rp, f)
    B = lambda a: a != 0   # noqa: E731
    W = f["words"]
    push = B(p["mode_push"])
    # every side of the rules is reached
    for name in FLAGS + ["k_masked", "k_lines", "k_lm_from_commits", "need_park_slot", "need_ulist"]:
        assert 0 < B(p[name]).sum() < f.size, name
    assert set(np.unique(p["kernel"])) == {PULL_NONE, PULL_FLAT, PULL_LIST, PULL_RECEIVER, PULL_RECORD}
    # the chosen MODE is built for W
    kexp = (p["kernel"] == PULL_LIST) | (p["kernel"] == PULL_RECEIVER)
    assert (W[kexp] >= p["mode_min_width"][kexp]).all()
    flat = p["kernel"] == PULL_FLAT
    assert (W[flat] <= 32).all() and np.isin(p["mode"][flat], (0, 2)).all()
    assert (W[p["kernel"] == PULL_RECORD] == 64).all()
    assert (p["kernel"][~push & (f["nloc"] > 0)] != PULL_NONE).all()
    # a push round has no pull flag set, and no pull kernel
    for name in PULL_FLAGS + ["k_masked", "k_lines", "k_lm_from_commits", "need_park_slot", "need_ulist", "scan", "mode"]:
        assert not B(p[name])[push].any(), name
    assert (p["kernel"][push] == PULL_NONE).all()
    # the done-probe and list variants scan filtered or unfiltered, nothing else
    narrow = B(p["dprobe"]) | B(p["ulist_read"])
    for name in "arc_mask prefilter split cml_read cml_write lines lm_write".split():
        assert not B(p[name])[narrow].any(), name
    assert np.isin(p["mode"][narrow] & 3, (0, 2)).all()
    assert not (B(p["alias"]) & ~B(p["dnb"])).any()
    assert not (B(p["dprobe"]) & ~(B(p["alias"]) & B(f["alias_active"]))).any()
    single = ~B(f["local"]) & (f["nloc"] == f["n_alloc"])
    s = B(p["split"])
    assert (B(p["prefilter"])[s] & ~B(p["early_exit"])[s] & single[s] & (f["acc_row"][s] > 0)).all()
    # the line masks the kernel reads are the ones the plan offers; where they came from
    assert not (B(p["k_lines"]) & ~B(p["lines"])).any()
    assert (B(p["k_lm_from_commits"]) == (B(p["k_lines"]) & B(f["lm_written"]))).all()
    assert (B(p["scan"] & 8) == (B(p["mode"] & 32) & ~push)).all()
    assert not (B(p["scan"] & 16) & ~B(f["lm_written"])).any()
    # records and line-mask writes never meet; one unfiltered / masked / prefiltered scan at most
    assert not (B(p["lm_write"]) & (B(p["cml_read"]) | B(p["cml_write"]))).any()
    assert ((B(p["unfiltered"]).astype(int) + B(p["arc_mask"]) + B(p["prefilter"])) <= 1).all()
    # the lazy buffers: a plan asks only for what it may use, so planning again
    # after a failed allocation never asks again
    assert not (B(p["need_park_slot"]) & ~B(f["can_park"])).any()
    assert not (B(p["need_ulist"]) & ~B(f["can_list"])).any()
    g = f.copy()
    g["can_park"] = 0
    q = plan_many(rp, g)
    assert not B(q["need_park_slot"]).any()
    g["can_list"] = 0
    q = plan_many(rp, g)
    assert not B(q["need_park_slot"]).any() and not B(q["need_ulist"]).any()
    # deterministic
    assert plan_many(rp, f).tobytes() == p.tobytes()


def _replay(rp, run):
    cfg, W = run["cfg"], max(1, 1 << int(np.ceil(np.log2(max(run["m"], 64) / 64))))
    churn = int(cfg["churn"])
    carry = dict(cml_written=0, lm_written=0, alias_active=0, ulist_valid=0, ul_cur=0, sate_since=-1)
    prev = dict(new_bits=0, receivers=0, next_arcs=0)
    held = 0
    got = []
    for r, rec in enumerate(run["rounds"]):
        assert rec["round"] == r
        inj = r < len(run["inj_arcs"])
        facts = dict(
            n=run["n"], n_alloc=run["n"], nloc=run["n"], nnz=run["nnz"], m=run["m"], words=W, round=r,
            prev_new_bits=prev["new_bits"], prev_receivers=prev["receivers"], prev_next_arcs=prev["next_arcs"],
            held_bits=held, inj_arcs=run["inj_arcs"][r] if inj else 0, inj_groups=run["inj_groups"][r] if inj else 0,
            last_inject_round=len(run["inj_arcs"]) - 1, local=0, liveness_active=churn, alive_on=churn, alive_now=churn,
            have_cml=int(cfg["compact_rows"] and W == 64), have_lm=int(W == 64), have_lmw=int(W == 64),
            have_ldone=int(W == 64), have_ld_cand=1, acc_row=run["n"] * (2 - (r & 1)),
            ld_env=int(run["env"].get("GP_LINE_DONE", -1)), lp_env=int(run["env"].get("GP_LINE_PACK", -1)),
            can_park=1, can_list=1, park_failed=0,
            # the one input the records do not carry: a list is read when it was short enough
            ulist_n=0 if rec["scan"] & 128 else run["n"],
            **carry, **{k: cfg[k] for k in CFG_I}, push_ratio=cfg["push_ratio"])
        p = plan(rp, **facts)
        got.append((p["mode_push"], p["scan"]))
        carry["cml_written"], carry["lm_written"] = p["cml_write"], p["lm_write"]
        carry["alias_active"] = int((carry["alias_active"] and (p["dprobe"] or p["mode_push"])) or rec["aliased"] > 0)
        carry["ulist_valid"] = p["ulist_emit"]
        carry["ul_cur"] ^= p["ulist_emit"]
        if p["sate"] and carry["sate_since"] < 0:
            carry["sate_since"] = r
        prev = {k: rec[k] for k in prev}
        held += rec["injected"] + rec["new_bits"]
    return got


@pytest.fixture(scope="module")
def trace():
    return json.load(open(TRACE))


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_replay(rp, trace, name):
    """The planner, fed each round's facts from the records before it and its
    own carry, chooses the recorded mode and scan of every round."""
    run = next(e for e in trace if e["name"] == name)
    want = [(r["mode"], r["scan"]) for r in run["rounds"]]
    assert _replay(rp, run) == want


def test_trace_reaches_its_rules(trace):
    """What each recorded run is in the fixture for."""
    scans = {e["name"]: [(r["mode"], r["scan"]) for r in e["rounds"]] for e in trace}
    a = [s for _, s in scans["a"]]
    for bit in (32, 8, 64, 128):   # degree-split, line masks, done probe, receiver list
        assert any(s & bit for s in a), bit
    assert any(s & 3 == 2 for _, s in scans["b"])          # an unfiltered pull under churn (parked rows)
    assert any(m == 1 for m, _ in scans["c"])              # a push round at W = 8
    assert any(s & 4 for _, s in scans["d"])               # records gathered
    assert scans["e"] == scans["a"]                        # the line rules change no record but row_bytes
