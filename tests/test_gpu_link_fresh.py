"""Per-link fresh deliveries (csrc/link.hip, gp_track_link_fresh, GP_LINK_FRESH,
gp_read_link_hist) against the CPU oracle.

link_fresh[j] is the first receipts arc j of the in-CSR delivered (sender
col[j], receiver the row of j): the news of the reference's arrival logs
(Peer.py:206, Peer.py:286) grouped by the connection it came over.  Every case
compares link_fresh() exactly with tests/link_ref.py, which evaluates the
first-receipt formula of DESIGN.md §2.4 on the oracle's outputs alone,
link_hist() exactly with the bincount of the array read, and checks that every
other output of the tracked run equals the oracle's as before.

Shapes are the smallest that reach each path: 4,099 vertices (no multiple of a
wave's 64 owners) and 5 (fewer than one wave), every row width, the five
direction / scan modes (every commit path must store the receivers' new rows),
the 5-vertex path that fills the u16 counts to 4,096, hubs split over items
(item boundaries inside dwords of the record) and long rows walked chunk by
chunk by the main kernel (the compaction's position mapping), churn and
explicit crashes, directed overlays, aliased Message-Lists, message shards,
all records at once, and the lifecycle.
"""
import numpy as np
import pytest

import directed_shapes as ds
import fresh_curve_ref
import fresh_ref
import link_ref
import load_ref
from test_gpu_curve import MODE_IDS, MODES, _alias_ref, _width_ref, check_curve, check_run, mode_cfg, overlay, run
from test_gpu_fresh import CHURN, _churn_ref, _crash_shapes, _hub_ref, _outputs, _same, _status

pytestmark = pytest.mark.gpu

BINS = 4097


def tracked(pkg, g, origin, inject, out_csr=None, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g, out_csr=out_csr) if out_csr is not None else eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.track_link_fresh()
    eng.reset()
    return eng


def check_link(eng, exp):
    """link_fresh() against the expected int64 [nnz]; link_hist() against the array read"""
    lf = eng.link_fresh()
    assert lf.dtype == np.uint16 and lf.shape == exp.shape
    bad = np.nonzero(lf.astype(np.int64) != exp)[0]
    assert bad.size == 0, (bad[:8], lf[bad[:8]], exp[bad[:8]])
    h = eng.link_hist()
    assert h.dtype == np.uint64 and h.shape == (BINS,)
    assert np.array_equal(h, np.bincount(lf, minlength=BINS).astype(np.uint64))
    return lf, h


_EXP = {}


def expected(key, g, ref, **kw):
    """link_ref.record, once per shape"""
    if key not in _EXP:
        _EXP[key] = link_ref.record(g, ref, **kw)
    return _EXP[key]


# -- sizes, widths, modes -----------------------------------------------------

WIDTHS = {1: 1, 100: 2, 200: 4, 500: 8, 1000: 16, 2000: 32, 4096: 64}


@pytest.mark.parametrize("m", sorted(WIDTHS))
@pytest.mark.parametrize("n", [4099, 5])
def test_widths(pkg, oracle, n, m):
    g, origin, inject, ref = _width_ref(n, m)
    exp = expected(("width", n, m), g, ref)
    if n == 4099 and m >= 100:
        assert (exp["link"] == 0).any() and (exp["link"] > 1).any()
    with tracked(pkg, g, origin, inject, **mode_cfg(MODES[0])) as eng:
        assert eng.info()[3] == WIDTHS[m]
        stats = run(eng, inject)
        check_link(eng, exp["link"])
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [100, 4096])
def test_modes(pkg, oracle, m, mode):
    g, origin, inject, ref = _width_ref(4099, m)
    exp = expected(("width", 4099, m), g, ref)
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        lf, _ = check_link(eng, exp["link"])
        _, _, uv, vu = pkg.links.undirected(g, lf)
        assert ((uv > 0) & (vu > 0)).any()   # some link has news in both directions
        check_run(eng, stats, ref)


def test_saturation(pkg, oracle):
    """the path 0-1-2-3-4 with 4,096 messages at vertex 0: the u16 bound, attained"""
    g = link_ref.path(pkg, 5)
    origin = np.zeros(4096, np.int32)
    ref = oracle.run(g, origin, None, want_first=True)
    exp = link_ref.record(g, ref)
    away = exp["src"] < exp["dst"]
    assert (exp["link"][away] == 4096).all() and (exp["link"][~away] == 0).all()
    with tracked(pkg, g, origin, None) as eng:
        stats = run(eng, None)
        _, h = check_link(eng, exp["link"])
        assert h[0] == 4 and h[4096] == 4 and int(h.sum()) == 8
        check_run(eng, stats, ref)


@pytest.mark.parametrize("m", [100, 4096])
def test_read_between_rounds(pkg, oracle, m):
    g, origin, inject, ref = _width_ref(4099, m)
    exp = expected(("width", 4099, m), g, ref)
    with tracked(pkg, g, origin, inject) as eng:
        _, h = check_link(eng, np.zeros(g.nnz, np.int64))   # zero before round 0
        assert h[0] == g.nnz
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            check_link(eng, exp["per_round"][r])
            check_link(eng, exp["per_round"][r])   # a read changes nothing
        check_run(eng, stats, ref)


# -- hubs ---------------------------------------------------------------------

@pytest.mark.parametrize("hub_threshold", [64, 1 << 30], ids=["split", "whole"])
def test_hubs(pkg, oracle, hub_threshold):
    """hub_threshold=64: k_link_hub walks the items of every vertex above 64
    arcs, and item boundaries fall inside dwords of the record; 1 << 30: nothing
    is split and the main kernel walks the long rows, many chunks per owner."""
    g, origin, ref = _hub_ref()
    assert np.diff(g.row_ptr).max() > 1000
    exp = expected("hub", g, ref)
    with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
        stats = run(eng, None)
        check_link(eng, exp["link"])
        check_run(eng, stats, ref)


# -- liveness -----------------------------------------------------------------

@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("m", [100, 1000])
def test_churn(pkg, oracle, m, mode):
    g, origin, inject, ref = _churn_ref(m)
    tot = {k: sum(s[k] for s in ref["stats"]) for k in ("crashed", "removals", "lost")}
    assert tot["crashed"] > 0 and tot["removals"] > 0 and tot["lost"] > 0
    exp = expected(("churn", m), g, ref, **CHURN)
    with tracked(pkg, g, origin, inject, churn=1, p_fail=0.02, churn_seed=5, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_link(eng, exp["link"])
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("which", ["after-receipt", "top-hub"])
def test_explicit_crashes(pkg, oracle, which, mode):
    """A crash in the round right after a receipt drops that frontier: the
    sender's stale row must not be read, so its out-arcs get nothing of that
    receipt, and its in-arcs keep what they delivered."""
    g, origin, inject, plain = _width_ref(4099, 100)
    crashes = _crash_shapes(plain, g)[which]
    ref = ds.CachedOracle(oracle).run(g, origin, inject, crashes=crashes, want_first=True)
    exp = expected(("crash", which), g, ref, crashes=crashes)
    if which == "after-receipt":
        vs = [v for v, _ in crashes]
        plain_exp = expected(("width", 4099, 100), g, plain)
        out_arcs, in_arcs = np.isin(exp["src"], vs), np.isin(exp["dst"], vs)
        assert int(exp["link"][out_arcs].sum()) < int(plain_exp["link"][out_arcs].sum())
        assert int(exp["link"][in_arcs].sum()) > 0
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject, crashes)
        check_link(eng, exp["link"])
        check_run(eng, stats, ref)


# -- directed -----------------------------------------------------------------

@pytest.mark.parametrize("crash", [False, True], ids=["plain", "crash"])
@pytest.mark.parametrize("shape", ["down", "up", "first3"])
def test_directed(pkg, oracle, shape, crash):
    """in-degree != out-degree: the pass walks the in-CSR whatever the overlay,
    hubs of the in-CSR through their items"""
    co = ds.CachedOracle(oracle)
    if shape == "first3":
        g = ds.first3(pkg, 3000)
        origin = pkg.overlay.random_origins(g.n, 300, seed=3)
    else:
        g = ds.oriented_chung_lu(pkg, co, 20_000, 8, 2.2, 11, shape)
        origin = pkg.overlay.random_origins(g.n, 256, seed=11)
    assert not np.array_equal(g.in_degree(), g.out_degree())
    crashes = []
    if crash:   # the busiest sender and the busiest receiver
        crashes = sorted({(int(np.argmax(g.out_degree())), 1), (int(np.argmax(g.in_degree())), 1)})
    ref = co.run(g, origin, None, crashes=crashes, want_first=True)
    exp = expected(("directed", shape, crash), g, ref, crashes=crashes)
    assert int(exp["link"].sum()) > 0
    for hub_threshold in (64, 1 << 30):
        with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
            stats = run(eng, None, crashes)
            check_link(eng, exp["link"])
            check_run(eng, stats, ref)


def test_directed_explicit_out_csr(pkg, oracle):
    """an out-CSR handed to gp_load_graph with every row's entries scrambled:
    the record stays in the order of the in-CSR as loaded"""
    co = ds.CachedOracle(oracle)
    g = ds.oriented_chung_lu(pkg, co, 3000, 8, 2.3, 5, "coin")
    orp, ocol = co.transpose(g.n, g.row_ptr, g.col)
    row = np.repeat(np.arange(g.n), np.diff(orp))
    scrambled = np.ascontiguousarray(ocol[np.lexsort((np.random.default_rng(5).random(ocol.size), row))])
    assert not np.array_equal(scrambled, ocol)
    origin = pkg.overlay.random_origins(g.n, 300, seed=5)
    inject = (np.arange(300) % 4).astype(np.int32)
    crashes = [(int(np.argmax(g.in_degree() + g.out_degree())), 1)]
    ref = co.run(g, origin, inject, crashes=crashes, want_first=True)
    exp = expected("out-csr", g, ref, crashes=crashes)
    assert int(exp["link"].sum()) > 0
    with tracked(pkg, g, origin, inject, out_csr=(orp.copy(), scrambled), hub_threshold=64, **mode_cfg(MODES[4])) as eng:
        got = eng.graph()
        assert np.array_equal(got.row_ptr, g.row_ptr) and np.array_equal(got.col, g.col)
        stats = run(eng, inject, crashes)
        check_link(eng, exp["link"])
        check_run(eng, stats, ref)


# -- aliased Message-Lists and receiver lists ----------------------------------

def test_aliases_and_receiver_lists(pkg, oracle):
    """The shape of test_aliased_message_lists (W = 64): receivers that complete
    commit an alias of their component row and no row of their own -- their new
    bits must still be stored as a frontier row."""
    g = overlay(pkg, 120_000, 12, 2.4, 41)
    origin = pkg.overlay.random_origins(g.n, 4096, seed=41)
    ref = _alias_ref(pkg)
    exp = expected("alias", g, ref)
    with tracked(pkg, g, origin, None, push_ratio=0.0, unfiltered_pct=0, hub_threshold=1 << 30,
                 arc_mask_permille=0, compact_rows=0) as eng:
        stats = run(eng, None)
        assert sum(s["aliased"] for s in stats) > 0
        assert any(s["scan"] & 128 for s in stats)
        check_link(eng, exp["link"])
        check_run(eng, stats, ref)


# -- message shards -----------------------------------------------------------

def test_message_shards_add_up(pkg, oracle):
    """two contexts with the word-aligned halves of one table: their arrays add
    element by element to the whole run's; their histograms do not"""
    g, origin, inject, ref = _width_ref(4099, 4096)
    exp = expected(("width", 4099, 4096), g, ref)
    total = np.zeros(g.nnz, np.int64)
    hists = np.zeros(BINS, np.uint64)
    digest = np.zeros(g.n, np.uint64)
    for lo, hi in ((0, 2048), (2048, 4096)):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.track_link_fresh()
            eng.reset()
            run(eng, inject[lo:hi])
            lf = eng.link_fresh()
            assert lf.max() <= hi - lo
            h = eng.link_hist()
            assert np.array_equal(h, np.bincount(lf, minlength=BINS).astype(np.uint64))
            total += lf
            hists += h
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
            digest ^= eng.digest()
    assert np.array_equal(total, exp["link"])
    whole = np.bincount(exp["link"], minlength=BINS).astype(np.uint64)
    assert int(hists.sum()) == 2 * int(whole.sum()) and not np.array_equal(hists, whole)
    assert np.array_equal(digest, ref["digest"])


# -- with the other records, and beside an untracked run -------------------------

@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_all_records_at_once(pkg, oracle, churn):
    """the spread curve, the traffic record, the per-peer fresh deliveries and
    their curve beside the per-link record: each equals its own reference, and
    the per-link record folds into the per-peer and per-message ones exactly"""
    g, origin, inject, ref = _churn_ref(100) if churn else _width_ref(4099, 1000)
    kw = CHURN if churn else {}
    cfg = dict(churn=1, p_fail=0.02, churn_seed=5) if churn else {}
    exp = expected(("churn", 100) if churn else ("width", 4099, 1000), g, ref, **kw)
    with pkg.GossipEngine(0, **cfg) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        for rec in ("curve", "load", "fresh", "fresh_curve", "link_fresh"):
            getattr(eng, "track_" + rec)()
        eng.reset()
        stats = run(eng, inject)
        lf, _ = check_link(eng, exp["link"])
        check_curve(eng.curve(), ref, inject)
        load = load_ref.totals(g, ref, **kw)
        assert np.array_equal(eng.load_sent().astype(np.int64), load["sent"])
        assert np.array_equal(eng.load_recv().astype(np.int64), load["recv"])
        fresh = fresh_ref.totals(g, ref, **kw)
        sent, recv = eng.fresh_sent().astype(np.int64), eng.fresh_recv().astype(np.int64)
        assert np.array_equal(sent, fresh["sent"]) and np.array_equal(recv, fresh["recv"])
        fc = eng.fresh_curve()
        assert np.array_equal(fc.astype(np.int64), fresh_curve_ref.curve(g, ref, **kw)["curve"])
        # on the engine's own outputs
        fs, fr = pkg.links.fold_peers(eng.graph(), lf)
        assert np.array_equal(fs, sent) and np.array_equal(fr, recv)
        assert int(lf.astype(np.int64).sum()) == int(fc.sum())
        check_run(eng, stats, ref)


@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_round_stats_are_the_untracked_runs(pkg, oracle, churn):
    """gp_round_stats of a run with gp_track_link_fresh alone: the untracked
    run's, work counters included (timings aside), and every other output"""
    g, origin, inject, ref = _churn_ref(100) if churn else _width_ref(4099, 1000)
    kw = CHURN if churn else {}
    cfg = dict(churn=1, p_fail=0.02, churn_seed=5) if churn else {}
    exp = expected(("churn", 100) if churn else ("width", 4099, 1000), g, ref, **kw)
    outs = []
    for on in (False, True):
        with pkg.GossipEngine(0, **cfg) as eng:
            eng.load_graph(g)
            eng.set_messages(origin, inject)
            if on:
                eng.track_link_fresh()
            eng.reset()
            outs.append(_outputs(pkg, eng, inject))
            if on:
                check_link(eng, exp["link"])
    assert outs[1]["frontier"] == pkg._lib.GP_ENOTRACK   # tracking does not make GP_FRONTIER readable
    _same(outs[0], outs[1], work_counters=True)
    assert np.array_equal(outs[1]["digest"], ref["digest"])


# -- lifecycle ----------------------------------------------------------------

def test_errors_and_lifecycle(pkg, oracle):
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = expected(("width", 4099, 100), g, ref)
    lib = pkg._lib
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        assert _status(pkg, eng.link_fresh) == lib.GP_ENOTRACK     # off by default
        assert _status(pkg, eng.link_hist) == lib.GP_ENOTRACK
        eng.track_link_fresh()
        assert _status(pkg, eng.link_fresh) == lib.GP_ENOTRACK     # takes effect at the next reset
        assert _status(pkg, eng.link_hist) == lib.GP_ENOTRACK
        eng.reset()
        short = np.full(g.nnz - 1, 77, np.uint16)                   # a wrong byte count: refused, nothing written
        assert eng._lib.gp_read(eng._ctx, lib.LINK_FRESH, short.ctypes.data, short.nbytes) == lib.GP_EINVAL
        assert (short == 77).all()
        big = np.full(g.nnz + 1, 77, np.uint16)
        assert eng._lib.gp_read(eng._ctx, lib.LINK_FRESH, big.ctypes.data, big.nbytes) == lib.GP_EINVAL
        assert (big == 77).all()
        for bins in (4096, 4098, 0):                                # a wrong bin count
            hb = np.full(4098, 77, np.uint64)
            assert eng._lib.gp_read_link_hist(eng._ctx, hb.ctypes.data, bins) == lib.GP_EINVAL
            assert (hb == 77).all()
        stats = run(eng, inject)
        check_link(eng, exp["link"])
        check_run(eng, stats, ref)
        eng.reset()                                                 # a second run starts from zero
        check_link(eng, np.zeros(g.nnz, np.int64))
        for _ in range(3):
            eng.round()
        check_link(eng, exp["per_round"][2])
        eng.track_link_fresh(False)                                 # off again: at the next reset
        check_link(eng, exp["per_round"][2])
        eng.reset()                                                 # (which frees the array)
        assert _status(pkg, eng.link_fresh) == lib.GP_ENOTRACK
        assert _status(pkg, eng.link_hist) == lib.GP_ENOTRACK
        stats = run(eng, inject)                                    # and the untracked run is the oracle's
        check_run(eng, stats, ref)
    with tracked(pkg, g, origin, inject) as eng:
        blob0 = eng.checkpoint()
        stats = [eng.round() for _ in range(3)]
        blob3 = eng.checkpoint()
        with tracked(pkg, g, origin, inject) as other:
            other.restore(blob3)                                    # past round 0: the record is not in the blob
            assert _status(pkg, other.link_fresh) == lib.GP_ESTATE
            assert _status(pkg, other.link_hist) == lib.GP_ESTATE
            more = run(other, inject)
            assert _status(pkg, other.link_fresh) == lib.GP_ESTATE
            check_run(other, stats + more, ref)                     # the restored run itself is exact
            other.reset()
            run(other, inject)
            check_link(other, exp["link"])
            other.restore(blob0)                                    # a blob of round 0 has counted nothing yet
            run(other, inject)
            check_link(other, exp["link"])


def test_second_overlay_resizes_the_record(pkg, oracle):
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = expected(("width", 4099, 100), g, ref)
    p = link_ref.path(pkg, 5)
    porigin = np.zeros(70, np.int32)
    pref = oracle.run(p, porigin, None, want_first=True)
    pexp = link_ref.record(p, pref)
    assert p.nnz != g.nnz
    with tracked(pkg, g, origin, inject) as eng:
        run(eng, inject)
        check_link(eng, exp["link"])
        eng.load_graph(p)                                           # tracking stays asked for
        eng.set_messages(porigin, None)
        eng.reset()
        assert eng.link_fresh().shape == (p.nnz,)
        stats = run(eng, None)
        check_link(eng, pexp["link"])
        check_run(eng, stats, pref)
        eng.load_graph(g)                                           # and back
        eng.set_messages(origin, inject)
        eng.reset()
        stats = run(eng, inject)
        check_link(eng, exp["link"])
        check_run(eng, stats, ref)


def test_partitioned_context_keeps_no_record(pkg, oracle):
    g, origin, inject, _ = _width_ref(4099, 100)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.track_link_fresh()
        eng.reset()
        assert _status(pkg, eng.link_fresh) == pkg._lib.GP_ENOTRACK
        assert _status(pkg, eng.link_hist) == pkg._lib.GP_ENOTRACK
