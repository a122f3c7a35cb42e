"""Every per-run record at once -- the spread curve, the traffic record, the
per-peer fresh deliveries and their curve, the per-link fresh deliveries, the
receipt delays and the delivery multiplicity -- at the row
widths, on the overlays and through the commit paths that the records' own test
files leave out.

One engine per case keeps all seven records.  Each is compared exactly with its
reference (load_ref, fresh_ref, fresh_curve_ref, link_ref, delay_ref, mult_ref)
evaluated on the oracle's first-receipt matrix, and every other output of the
run with the oracle's (check_run).  All comparisons are exact integers.

A. Widths.  k_fresh, k_fresh_curve and k_mult (and their hub kernels) are built
   for W = 1, 2, 4, 8, 16, 32, 64; their own files run W = 1, 2, 16, 64.  Here:
   m = 200, 500, 2000 (W = 4, 8, 32) under the five direction / scan modes,
   m = 65, 300, 1025, 2049 (rows that are mostly padding), hubs split at 64
   arcs read after every round, and one run cut into shards of W = 4, 8, 32, 32.
B. A raw in-CSR with self-loops and repeated arcs (raw_csr.py): a repeated arc
   is two deliverers, a self-loop counts in the load and in nothing fresh.
C. One case per round kind of the pull with the records on, each with its own
   assertion on the round stats that the kind ran: a commit path that stored a
   stale or partial frontier row would leave seen, first and digest right and
   the records wrong.  The store of the receivers' new rows each case reaches:

     finish_row (gp_device.h)        every per-receiver case's serial loop, the
                                     hubs' k_hub_final (test_hubs_between_rounds)
                                     and a degree-split round's touched
                                     receivers (test_degree_split)
     pair_finish (pull_groups.h)     test_compact_message_lists: k_expand_rec
                                     (prefilter 0), pre_pairs (prefilter 20);
                                     test_done_neighbours[W64] (dnb_pairs /
                                     gather_pairs)
     pre_quads (pull_groups.h)       test_degree_split[W64]
     dnb_quads (pull_groups.h)       test_done_neighbours[W64],
                                     test_sated_under_churn, test_line_done_pack
     group_finish (pull_groups.h)    test_degree_split[W32, W8-receiver],
                                     test_done_neighbours[W32, W16-late, W8-late]
     k_expand_flat (pull_flat.hip)   test_widths[pull-unfiltered, push,
                                     adaptive], test_degree_split[W8-flat]
     k_apply_lanes (push.hip)        test_widths[push, adaptive] (W = 4, 8, 32;
                                     a W = 64 push commits through k_apply's
                                     finish_row); with the spread curve on, the
                                     push gathers the senders' exact rows as well
"""
import functools

import numpy as np
import pytest

import delay_ref
import fresh_curve_ref
import fresh_ref
import link_ref
import load_ref
import mult_ref
import raw_csr
from test_gpu_curve import MODE_IDS, MODES, _alias_ref, _width_ref, check_curve, check_run, mode_cfg, overlay, run
from test_gpu_delay import check_bins, check_delay
from test_gpu_fresh import FORMS, check_fresh, set_form
from test_gpu_fresh_curve import check_fc
from test_gpu_link_fresh import check_link
from test_gpu_load import check_load
from test_gpu_mult import check_mult

pytestmark = pytest.mark.gpu

RECORDS = ("curve", "load", "fresh", "fresh_curve", "link_fresh", "delay", "mult")


def tracked(pkg, g, origin, inject, **cfg):
    """one engine with every record on"""
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    for rec in RECORDS:
        getattr(eng, "track_" + rec)()
    eng.reset()
    return eng


_EXP = {}


def expected(key, g, ref, inject, fc_words=None, **kw):
    """every record's reference, once per shape (fc_words: the 64-message words
    of the fresh-delivery curve to evaluate, a big shape's sample)"""
    if key not in _EXP:
        _EXP[key] = {"load": load_ref.totals(g, ref, **kw), "fresh": fresh_ref.totals(g, ref, **kw),
                     "fc": fresh_curve_ref.curve(g, ref, words=fc_words, **kw), "link": link_ref.record(g, ref, **kw),
                     "delay": delay_ref.totals(ref, inject), "mult": mult_ref.totals(g, ref, **kw)}
    return _EXP[key]


def check_records(pkg, eng, g, exp, r=None):
    """the six arc- and receipt-level records against `exp`: at the end of the
    run, or (r) as they stand after round r"""
    if r is None:
        load, fresh, fc, link = exp["load"], exp["fresh"], exp["fc"]["curve"], exp["link"]["link"]
        delay = (exp["delay"]["sum"], exp["delay"]["max"], exp["delay"]["seenpop"])
        mult = exp["mult"]
    else:
        load = dict(zip(("sent", "recv"), exp["load"]["per_round"][r]))
        fresh = dict(zip(("sent", "recv"), exp["fresh"]["per_round"][r]))
        fc, link = exp["fc"]["per_round"][r], exp["link"]["per_round"][r]
        delay = exp["delay"]["per_round"][r]
        mult = dict(zip(("hist", "sole_recv", "sole_sent"), exp["mult"]["per_round"][r]))
    check_load(eng, load)
    check_fresh(eng, fresh)
    check_fc(eng, fc, exp["fc"]["columns"])   # (sum link_fresh = sum fresh_curve below covers the other columns)
    lf, _ = check_link(eng, link)
    arrays = check_delay(eng, delay)
    check_bins(pkg, eng, np.diff(g.row_ptr), arrays)
    check_mult(pkg, eng, g, mult)
    check_sums(pkg, eng, lf)


def check_sums(pkg, eng, lf):
    """the row and column sums of DESIGN.md §2.4, on the engine's own outputs:
    sum_row link_fresh = fresh_recv, sum_{col = u} link_fresh = fresh_sent,
    mult_hist[1] = sum sole_recv = sum sole_sent, sum link_fresh = sum fresh_curve"""
    got = eng.graph()
    rp, col = np.asarray(got.row_ptr, np.int64), np.asarray(got.col, np.int64)
    lf = lf.astype(np.int64)
    by_row = np.concatenate([[0], np.cumsum(lf)])
    assert np.array_equal(by_row[rp[1:]] - by_row[rp[:-1]], eng.fresh_recv().astype(np.int64))
    by_col = np.bincount(col, weights=lf, minlength=eng.n).astype(np.int64)
    assert np.array_equal(by_col, eng.fresh_sent().astype(np.int64))
    hist = eng.mult_hist()
    assert int(hist[1]) == int(eng.sole_recv().astype(np.int64).sum()) == int(eng.sole_sent().astype(np.int64).sum())
    assert int(lf.sum()) == int(eng.fresh_curve().sum())
    assert (eng.fresh_sent() <= eng.load_sent()).all() and (eng.fresh_recv() <= eng.load_recv()).all()


def run_and_check(pkg, eng, g, exp, ref, inject, crashes=()):
    stats = run(eng, inject, crashes)
    check_records(pkg, eng, g, exp)
    check_curve(eng.curve(), ref, inject)
    check_run(eng, stats, ref)
    return stats


# -- A. widths ------------------------------------------------------------------

WIDTHS = {200: 4, 500: 8, 2000: 32}                 # the widths the three records' own files never run
PADDED = {65: 2, 300: 8, 1025: 32, 2049: 64}        # rows that are mostly padding: 2, 5, 17, 33 real words
# the 5-vertex overlay is a path of three vertices and two isolated ones: where
# _width_ref's origin of the last message is isolated, another seed of the origins
SEED5 = {300: 304, 1025: 1026, 2049: 2051}


@functools.lru_cache(maxsize=None)
def _shape(n, m):
    """_width_ref(n, m); at n = 5 with the origins' seed that meets the
    conditions of meaningful()"""
    if n != 5 or m not in SEED5:
        return _width_ref(n, m)
    import _gossip_pkg
    from oracle import lib
    pkg = _gossip_pkg.load()
    g = _width_ref(5, m)[0]
    origin = pkg.overlay.random_origins(g.n, m, seed=SEED5[m])
    inject = (np.arange(m) % 3).astype(np.int32)
    return g, origin, inject, lib.run(g, origin, inject, want_first=True)


def meaningful(n, m, g, ref, exp):
    """conditions on the oracle's outputs alone, before the engine is touched"""
    if n == 4099:   # receipts with every number of deliverers
        assert (exp["mult"]["hist"][1:17] > 0).all(), exp["mult"]["hist"]
    # the last real message was delivered and spread
    assert int(exp["fc"]["curve"][:, m - 1].sum()) > 0 and int(ref["coverage"][m - 1]) > 1
    if m in PADDED:   # a receipt in the last real word
        lo = 64 * ((m - 1) // 64)
        assert (ref["first"][:, lo:m] != 255).sum() > m - lo


CASES = [(n, m, mi, form) for n in (4099, 5) for m in sorted(WIDTHS) for mi in range(len(MODES))
         for form in (FORMS if n == 4099 else FORMS[1:])]
CASES += [(n, m, 4, form) for n in (4099, 5) for m in sorted(PADDED) for form in (FORMS if n == 4099 else FORMS[1:])]


@pytest.mark.parametrize("n,m,mi,form", CASES, ids=[f"{n}-{m}-{MODE_IDS[mi]}-{form}" for n, m, mi, form in CASES])
def test_widths(pkg, oracle, monkeypatch, n, m, mi, form):
    """W = 4, 8, 32 under the five modes (the pulls commit through finish_row
    and, at flat_max_words 16 / 32, k_expand_flat; the push through k_apply),
    and the padded rows under the default configuration (MODES[4])"""
    g, origin, inject, ref = _shape(n, m)
    exp = expected(("width", n, m), g, ref, inject)
    meaningful(n, m, g, ref, exp)
    set_form(monkeypatch, form)
    with tracked(pkg, g, origin, inject, **mode_cfg(MODES[mi])) as eng:
        assert eng.info()[3] == {**WIDTHS, **PADDED}[m]
        stats = run_and_check(pkg, eng, g, exp, ref, inject)
        if MODE_IDS[mi] == "push":
            assert all(s["mode"] == 1 for s in stats)
        if MODE_IDS[mi].startswith("pull"):
            assert all(s["mode"] == 0 for s in stats)


@pytest.mark.parametrize("m", sorted(WIDTHS))
def test_hubs_between_rounds(pkg, oracle, m):
    """hub_threshold=64: the hub kernels of the three records at RPI = 32, 16
    and 4 row slots, every record read after every round"""
    g, origin, inject, ref = _shape(4099, m)
    assert np.diff(g.row_ptr).max() > 4 * 64
    exp = expected(("width", 4099, m), g, ref, inject)
    meaningful(4099, m, g, ref, exp)
    with tracked(pkg, g, origin, inject, hub_threshold=64) as eng:
        assert eng.info()[3] == WIDTHS[m]
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            check_records(pkg, eng, g, exp, r)
        check_curve(eng.curve(), ref, inject)
        check_run(eng, stats, ref)


def test_message_shards(pkg, oracle):
    """The 4,096-message table of the 4099 shape cut at 256, 768 and 2816:
    blocks of W = 4, 8, 32 and 32 words, the last with 20 real ones.  Each
    record combines under its rule of DESIGN.md §2.4: the per-peer and per-link
    counts, the sole deliveries, the multiplicity histogram and the delay sums
    add, the delay maxima combine element-wise, the fresh-delivery curves
    concatenate."""
    g, origin, inject, ref = _shape(4099, 4096)
    exp = expected(("width", 4099, 4096), g, ref, inject)
    cuts = [0, 256, 768, 2816, 4096]
    add = {k: np.zeros(g.n, np.int64) for k in ("load_sent", "load_recv", "fresh_sent", "fresh_recv", "sole_sent",
                                                "sole_recv", "delay_sum")}
    link = np.zeros(g.nnz, np.int64)
    most = np.zeros(g.n, np.int64)
    hists, curves = [], []
    digest = np.zeros(g.n, np.uint64)
    for (lo, hi), words in zip(zip(cuts[:-1], cuts[1:]), (4, 8, 32, 32)):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            for rec in RECORDS:
                getattr(eng, "track_" + rec)()
            eng.reset()
            assert eng.info()[3] == words
            stats = run(eng, inject[lo:hi])
            for k in add:
                add[k] += getattr(eng, k)().astype(np.int64)
            lf = eng.link_fresh()
            assert lf.max() <= hi - lo
            link += lf
            most = np.maximum(most, eng.delay_max().astype(np.int64))
            hists.append(eng.mult_hist())
            part = eng.fresh_curve().astype(np.int64)
            assert part.shape == (len(stats) + 1, hi - lo)
            curves.append(np.pad(part, ((0, ref["rounds"] + 1 - part.shape[0]), (0, 0))))   # (a shard may stop earlier)
            check_sums(pkg, eng, lf)
            assert np.array_equal(eng.curve(), np.stack([(ref["first"][:, lo:hi] == r).sum(axis=0)
                                                         for r in range(len(stats) + 1)]).astype(np.uint64))
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
            digest ^= eng.digest()
    for rec, a, b in (("load", "sent", "recv"), ("fresh", "sent", "recv")):
        assert np.array_equal(add[rec + "_" + a], exp[rec][a]) and np.array_equal(add[rec + "_" + b], exp[rec][b]), rec
    assert np.array_equal(link, exp["link"]["link"])
    assert np.array_equal(add["sole_sent"], exp["mult"]["sole_sent"])
    assert np.array_equal(add["sole_recv"], exp["mult"]["sole_recv"])
    assert np.array_equal(pkg.fragility.combine(hists).astype(np.int64), exp["mult"]["hist"])
    assert np.array_equal(add["delay_sum"], exp["delay"]["sum"]) and np.array_equal(most, exp["delay"]["max"])
    assert np.array_equal(np.concatenate(curves, axis=1), exp["fc"]["curve"])
    assert np.array_equal(digest, ref["digest"])


# -- B. a raw CSR: self-loops, repeated arcs, unsorted in-lists ---------------------

RAW_WIDTHS = {100: 2, 2000: 32}


@functools.lru_cache(maxsize=None)
def _raw_ref(m, crash):
    """(g, origin, inject, crashes, ref) of the raw CSR; crash: the busiest
    sender and the busiest receiver go down in round 1"""
    import _gossip_pkg
    from oracle import lib
    pkg = _gossip_pkg.load()
    g = raw_csr.loops_and_repeats(pkg)
    origin = pkg.overlay.random_origins(g.n, m, seed=41)
    inject = (np.arange(m) % 3).astype(np.int32)
    crashes = []
    if crash:   # (the overlay is undirected, one vertex is both: the busiest of the others as well)
        recv = int(np.argmax(g.in_degree()))
        out = g.out_degree().copy()
        out[recv] = -1
        crashes = sorted([(recv, 1), (int(np.argmax(out)), 1)])
    return g, origin, inject, crashes, lib.run(g, origin, inject, crashes=crashes, want_first=True)


def raw_meaningful(pkg, oracle, m, g, origin, inject, ref, exp):
    """the raw CSR's record is not the record of its simple copy (no loop, every
    repeated arc once), although both runs hold the same first-receipt matrix"""
    s = raw_csr.simple_copy(pkg, g)
    assert s.nnz == g.nnz - 300 - 4000
    sref = oracle.run(s, origin, inject, want_first=True)
    assert np.array_equal(sref["first"], ref["first"])
    sexp = expected(("raw-simple", m), s, sref, inject)
    assert not np.array_equal(exp["fresh"]["sent"], sexp["fresh"]["sent"])
    assert int(exp["link"]["link"].sum()) > int(sexp["link"]["link"].sum())
    assert exp["mult"]["hist"][1] < sexp["mult"]["hist"][1] and exp["mult"]["hist"][2] != sexp["mult"]["hist"][2]
    src, dst, link = exp["link"]["src"], exp["link"]["dst"], exp["link"]["link"]
    # both copies of a repeated arc hold the same count, and it is not zero everywhere
    order = np.argsort(dst * g.n + src, kind="stable")
    key = (dst * g.n + src)[order]
    twin = np.nonzero(key[1:] == key[:-1])[0]
    assert twin.size >= 4000
    assert np.array_equal(link[order[twin]], link[order[twin + 1]]) and (link[order[twin]] > 0).any()
    # a self-loop carries every message of its vertex (load) and no news
    loop = src == dst
    assert int(loop.sum()) == 300 and not link[loop].any()
    v = dst[loop]
    assert (exp["load"]["recv"][v] - sexp["load"]["recv"][v] >= (ref["first"][v] != 255).sum(axis=1)).all()
    assert ((ref["first"][v] != 255).sum(axis=1) > 0).all()


@pytest.mark.parametrize("hub_threshold", [64, 1 << 30], ids=["split", "whole"])
@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("m", sorted(RAW_WIDTHS))
def test_raw_csr(pkg, oracle, m, mode, hub_threshold):
    """parallel arcs count separately in link_fresh, fresh_sent, fresh_recv and
    the multiplicity; k_link stages one live neighbour twice"""
    g, origin, inject, _, ref = _raw_ref(m, False)
    exp = expected(("raw", m), g, ref, inject)
    raw_meaningful(pkg, oracle, m, g, origin, inject, ref, exp)
    with tracked(pkg, g, origin, inject, hub_threshold=hub_threshold, **mode_cfg(mode)) as eng:
        assert eng.info()[3] == RAW_WIDTHS[m]
        got = eng.graph()
        assert np.array_equal(got.row_ptr, g.row_ptr) and np.array_equal(got.col, g.col)   # loaded as given
        run_and_check(pkg, eng, g, exp, ref, inject)


@pytest.mark.parametrize("m", sorted(RAW_WIDTHS))
def test_raw_csr_crashes(pkg, oracle, m):
    """the busiest sender and the busiest receiver crash in round 1"""
    g, origin, inject, crashes, ref = _raw_ref(m, True)
    exp = expected(("raw-crash", m), g, ref, inject, crashes=crashes)
    plain = expected(("raw", m), g, _raw_ref(m, False)[4], inject)
    assert not np.array_equal(exp["mult"]["hist"], plain["mult"]["hist"])
    with tracked(pkg, g, origin, inject, hub_threshold=64) as eng:
        run_and_check(pkg, eng, g, exp, ref, inject, crashes)


# -- C. commit paths, with the records on ---------------------------------------------

@functools.lru_cache(maxsize=None)
def _path_ref(n, dbar, gamma, seed, m, schedule, churn=None):
    """(g, origin, inject, kw, ref): a Chung-Lu overlay of the parity test of the
    same kind, at the size its case found"""
    import _gossip_pkg
    from oracle import lib
    pkg = _gossip_pkg.load()
    g = overlay(pkg, n, dbar, gamma, seed)
    origin = pkg.overlay.random_origins(g.n, m, seed=seed)
    inject = None if schedule is None else (np.arange(m) % schedule).astype(np.int32)
    kw = dict(churn=True, p_fail=churn[0], churn_seed=churn[1]) if churn else {}
    if (n, dbar, gamma, seed, m, schedule, churn) == (120_000, 12, 2.4, 41, 4096, None, None):
        return g, origin, inject, kw, _alias_ref(pkg)   # the ceiling: the shape the other record files share
    return g, origin, inject, kw, lib.run(g, origin, inject, want_first=True, **kw)


def path_case(pkg, shape, cfg):
    g, origin, inject, kw, ref = _path_ref(*shape)
    # (the curve's reference walks every set bit: over 20,000 vertices, three words of it)
    whole = shape[4] // 64   # the words that hold 64 messages
    fc_words = (0, whole // 2, whole - 1) if shape[0] > 20_000 else None
    exp = expected(("path",) + shape, g, ref, inject, fc_words=fc_words, **kw)
    if kw:
        cfg = dict(cfg, churn=1, p_fail=kw["p_fail"], churn_seed=kw["churn_seed"])
    with tracked(pkg, g, origin, inject, **cfg) as eng:
        stats = run_and_check(pkg, eng, g, exp, ref, inject)
        return stats, eng.info()[3]


SPLIT = dict(hub_threshold=512, push_ratio=1000.0, unfiltered_pct=90, arc_mask_permille=0, prefilter_pct=20,
             compact_rows=0, split_deg=8, split_max_permille=1000)   # test_gpu_parity.py::test_degree_split
SPLIT_CASES = {"W64": (8198, 2049, 16, 64), "W32": (4099, 1025, 16, 32), "W8-receiver": (4099, 257, 0, 8),
               "W8-flat": (4099, 257, 16, 8)}


@pytest.mark.parametrize("case", list(SPLIT_CASES))
def test_degree_split(pkg, oracle, case):
    """Degree-split rounds (scan bit 32): senders of in-degree < 8 push into the
    accumulator, whose touched receivers commit through finish_row; the others
    through pre_quads (W = 64), pre_groups (W = 32, and W = 8 at
    flat_max_words 0) or the flat kernel (W = 8 at flat_max_words 16).
    Chung-Lu(n, 10, 2.4, 61), inject rounds 0-1; the smallest n of the ladder
    4099, 8198, ... and the smallest m of the width: W = 64: 8198 x 2049 (at
    4099 round 0 reads line masks instead); W = 32: 4099 x 1025; W = 8:
    4099 x 257."""
    n, m, flat_max_words, words = SPLIT_CASES[case]
    stats, W = path_case(pkg, (n, 10, 2.4, 61, m, 2), dict(SPLIT, flat_max_words=flat_max_words))
    scans = [s["scan"] for s in stats]
    assert W == words
    assert any(x & 32 for x in scans), scans
    assert all((x & 3) == 3 for x in scans if x & 32), scans


def test_line_masks(pkg, oracle):
    """Line masks (scan bit 8) built by k_mklm in round 0 and written by round
    0's commits for round 1 (bit 16): finish_row's lm_next ballots beside its
    frontier row.  Chung-Lu(8198, 12, 2.4, 52) x 2049 messages, all injected in
    round 0 (at 4099 vertices round 1 is already unfiltered)."""
    stats, W = path_case(pkg, (8198, 12, 2.4, 52, 2049, None),
                         dict(hub_threshold=256, push_ratio=0.0, unfiltered_pct=90, flat_max_words=16,
                              arc_mask_permille=0, prefilter_pct=0, compact_rows=0))
    scans = [s["scan"] for s in stats]
    assert W == 64
    assert any(x & 8 for x in scans), scans
    assert any(x & 16 for x in scans), scans
    assert all(x & 8 for x in scans if x & 16), scans


@pytest.mark.parametrize("prefilter,n", [(0, 4099), (20, 65584)])
def test_compact_message_lists(pkg, oracle, prefilter, n):
    """Compact Message-Lists (scan bit 4): without the prefilter the flat record
    pull (k_expand_rec, pair_finish), with it the per-receiver loop (pre_pairs,
    finish_row with records).  Chung-Lu(n, 8, 2.5, 31) x 2049 messages, all
    injected in round 0, no hub splits.  prefilter 0: 4099 vertices; prefilter
    20: 65,584 (below that the record rounds have too many senders for the
    prefilter: scan 4, not 7)."""
    stats, W = path_case(pkg, (n, 8, 2.5, 31, 2049, None),
                         dict(push_ratio=0.0, prefilter_pct=prefilter, arc_mask_permille=0, compact_rows=1,
                              hub_threshold=1 << 30))
    assert W == 64
    assert any(s["scan"] & 4 for s in stats)
    assert any((s["scan"] & 3) == (3 if prefilter else 0) and s["scan"] & 4 for s in stats), [s["scan"] for s in stats]


DNB = dict(hub_threshold=4096, push_ratio=10.0, unfiltered_pct=90, flat_max_words=16, arc_mask_permille=10,
           prefilter_pct=20, compact_rows=1)   # test_gpu_parity.py::test_done_in_neighbours
DNB_CASES = {"W64": (41, 2049, DNB, 64), "W32": (41, 1025, DNB, 32),
             # test_narrow_late_rounds_per_receiver: every round a filtered pull
             "W16-late": (43, 513, dict(DNB, push_ratio=0.0, unfiltered_pct=0, arc_mask_permille=0), 16),
             "W8-late": (43, 257, dict(DNB, push_ratio=0.0, unfiltered_pct=0, arc_mask_permille=0), 8)}


@pytest.mark.parametrize("case", list(DNB_CASES))
def test_done_neighbours(pkg, oracle, case):
    """Done-neighbour receivers (done_nb > 0): they take cmask & ~seen without
    gathering a row and still owe the record their new bits -- dnb_quads and
    gather_pairs at W = 64, dnb_groups / gather_groups at W = 32 and, in the
    thin late rounds that leave the flat kernel, at W = 16 and 8.
    Chung-Lu(4099, 12, 2.5, seed) x 2049, 1025, 513 and 257 messages, all
    injected in round 0: the first rung of the ladder has them at every width."""
    seed, m, cfg, words = DNB_CASES[case]
    stats, W = path_case(pkg, (4099, 12, 2.5, seed, m, None), cfg)
    assert W == words
    dnb = [s["done_nb"] for s in stats]
    assert sum(dnb) > 0, dnb
    for s in stats:
        assert s["done_nb"] == 0 or (s["mode"] == 0 and s["done_nb"] <= s["vertices_visited"])


def test_sated_under_churn(pkg, oracle):
    """Under churn the done bitmap is the sated marks: once a round has marked
    them, receivers with a sated in-neighbour take cmask & F_r & ~seen
    (done_nb > 0 with crashes in the run).  Chung-Lu(4099, 12, 2.4, 31) x 2049
    messages in round 0, p_fail 0.02, every round a filtered pull of the
    per-receiver kernel."""
    stats, W = path_case(pkg, (4099, 12, 2.4, 31, 2049, None, (0.02, 7)),
                         dict(hub_threshold=256, push_ratio=0.0, unfiltered_pct=0, flat_max_words=0,
                              arc_mask_permille=0))
    assert W == 64
    assert sum(s["crashed"] for s in stats) > 0 and all(s["mode"] == 0 for s in stats)
    assert sum(s["done_nb"] for s in stats) > 0, [s["done_nb"] for s in stats]


def test_line_done_pack(pkg, oracle, monkeypatch):
    """GP_LINE_DONE=1 GP_LINE_PACK=1 (read at gp_create): the unfiltered
    early-exit pulls seed their targets from a top in-neighbour's complete
    lines and gather packed.  The gather's work counters of an unfiltered round
    differ from the run with both off, so the packed path ran, and both runs
    keep every record.  Chung-Lu(4099, 8, 2.5, 5) x 2049 messages in round 0,
    every round a pull, unfiltered from 1 % senders, no hub splits."""
    shape = (4099, 8, 2.5, 5, 2049, None)
    cfg = dict(push_ratio=0.0, unfiltered_pct=1, hub_threshold=1 << 30)
    monkeypatch.setenv("GP_LINE_DONE_MIN_DEG", "16")
    runs = {}
    for v in ("1", "0"):
        monkeypatch.setenv("GP_LINE_DONE", v)
        monkeypatch.setenv("GP_LINE_PACK", v)
        runs[v], W = path_case(pkg, shape, cfg)
        assert W == 64
    moved = [a["round"] for a, b in zip(runs["1"], runs["0"])
             if a["scan"] == 2 and (a["rows_gathered"], a["row_bytes"]) != (b["rows_gathered"], b["row_bytes"])]
    assert moved, "no unfiltered round's row_bytes or rows_gathered moved"
    for a, b in zip(runs["1"], runs["0"]):
        assert (a["mode"], a["scan"]) == (b["mode"], b["scan"])
