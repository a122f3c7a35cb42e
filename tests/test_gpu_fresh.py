"""Per-peer fresh deliveries (csrc/fresh.hip, gp_track_fresh, GP_FRESH_SENT /
GP_FRESH_RECV) against the CPU oracle.

fresh_sent[u] is the sends of peer u that delivered a first receipt and
fresh_recv[v] the arrivals at v of a message it did not hold: the lines of the
reference's arrival logs (Peer.py:206, Peer.py:286) that were news.  Every case
compares fresh_sent() / fresh_recv() exactly with tests/fresh_ref.py, which
evaluates the first-receipt formula of DESIGN.md §2.4 on the oracle's outputs
alone, and checks that every other output of the tracked run equals the
oracle's as before.

Shapes are the smallest that reach each path: 4,099 vertices (no multiple of a
wave's 64 owners) and 5 (fewer than one wave), every row width, the five
direction / scan modes (every commit path must store the receivers' new rows),
hubs split over items and long rows walked by the main kernel, both forms of
the pass (one gather that scatters the senders' side, the default and the
directed overlays' only form; one gather per role, GP_FRESH_GATHER=1 on
undirected overlays), churn and explicit crashes,
directed overlays, aliased Message-Lists, message shards, and the lifecycle.
The u64 accumulators cannot overflow a u32 at these sizes (a hub's round sum
needs 2^20 arcs x 4096 messages): csrc/fresh.hip argues them where they are.
"""
import functools

import numpy as np
import pytest

import directed_shapes as ds
import fresh_ref
import load_ref
from test_gpu_curve import (MODE_IDS, MODES, STAT_KEYS, _alias_ref, _width_ref, check_curve, check_run, mode_cfg,
                            overlay, run)

pytestmark = pytest.mark.gpu

FORMS = ["gather", "scatter"]


def set_form(monkeypatch, form):
    """before the engine is created: GP_FRESH_GATHER is read at gp_create"""
    if form == "gather":
        monkeypatch.setenv("GP_FRESH_GATHER", "1")
    else:
        monkeypatch.delenv("GP_FRESH_GATHER", raising=False)


def tracked(pkg, g, origin, inject, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.track_fresh()
    eng.reset()
    return eng


def check_fresh(eng, exp):
    sent, recv = eng.fresh_sent(), eng.fresh_recv()
    assert sent.dtype == recv.dtype == np.uint64 and sent.shape == recv.shape == (eng.n,)
    assert np.array_equal(recv.astype(np.int64), exp["recv"]), np.nonzero(recv.astype(np.int64) != exp["recv"])[0][:8]
    assert np.array_equal(sent.astype(np.int64), exp["sent"]), np.nonzero(sent.astype(np.int64) != exp["sent"])[0][:8]


_EXP = {}


def expected(key, g, ref, **kw):
    """fresh_ref.totals, once per shape"""
    if key not in _EXP:
        _EXP[key] = fresh_ref.totals(g, ref, **kw)
    return _EXP[key]


# -- sizes, widths, modes -----------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [1, 100, 1000, 4096])
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_modes(pkg, oracle, monkeypatch, n, m, mode):
    g, origin, inject, ref = _width_ref(n, m)
    exp = expected(("width", n, m), g, ref)
    assert int(exp["sent"].sum()) == int(exp["recv"].sum()) >= sum(s["new_bits"] for s in ref["stats"])
    set_form(monkeypatch, "scatter")
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_fresh(eng, exp)
        check_fresh(eng, exp)   # a read changes nothing
        check_run(eng, stats, ref)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", [100, 4096])
def test_read_between_rounds(pkg, oracle, monkeypatch, m, form):
    g, origin, inject, ref = _width_ref(4099, m)
    exp = expected(("width", 4099, m), g, ref)
    set_form(monkeypatch, form)
    with tracked(pkg, g, origin, inject) as eng:
        assert not eng.fresh_sent().any() and not eng.fresh_recv().any()
        stats, prev = [], 0
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            s, v = exp["per_round"][r]
            check_fresh(eng, {"sent": s, "recv": v})
            assert int(v.sum()) - prev >= stats[-1]["new_bits"]
            prev = int(v.sum())
        check_run(eng, stats, ref)


# -- hubs ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hub_ref():
    import _gossip_pkg
    from oracle import lib
    pkg = _gossip_pkg.load()
    rp, col = lib.chung_lu(20_000, 8, 2.2, 11)
    g = pkg.CSR(20_000, rp, col, False)
    origin = pkg.overlay.random_origins(g.n, 256, seed=11)
    return g, origin, lib.run(g, origin, None, want_first=True)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hub_threshold", [64, 1 << 30], ids=["split", "whole"])
def test_hubs(pkg, oracle, monkeypatch, hub_threshold, form):
    """hub_threshold=64: k_fresh_hub walks the items of every vertex above 64
    arcs, as receiver and as sender; 1 << 30: nothing is split and the main
    kernel walks the long rows."""
    g, origin, ref = _hub_ref()
    assert np.diff(g.row_ptr).max() > 1000
    exp = expected("hub", g, ref)
    set_form(monkeypatch, form)
    with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
        stats = run(eng, None)
        check_fresh(eng, exp)
        check_run(eng, stats, ref)


# -- liveness -----------------------------------------------------------------

CHURN = dict(churn=True, p_fail=0.02, churn_seed=5)


@functools.lru_cache(maxsize=None)
def _churn_ref(m):
    import _gossip_pkg
    from oracle import lib
    pkg = _gossip_pkg.load()
    g = overlay(pkg, 4099, 8, 2.2, 7)
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 7).astype(np.int32)
    return g, origin, inject, lib.run(g, origin, inject, want_first=True, **CHURN)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("m", [100, 1000])
def test_churn(pkg, oracle, monkeypatch, m, mode):
    g, origin, inject, ref = _churn_ref(m)
    tot = {k: sum(s[k] for s in ref["stats"]) for k in ("crashed", "removals", "lost", "new_bits")}
    assert tot["crashed"] > 0 and tot["removals"] > 0 and tot["lost"] > 0
    exp = expected(("churn", m), g, ref, **CHURN)
    load = load_ref.totals(g, ref, **CHURN)
    assert int(exp["sent"].sum()) == int(exp["recv"].sum()) >= tot["new_bits"]
    assert (exp["sent"] <= load["sent"]).all() and (exp["recv"] <= load["recv"]).all()
    set_form(monkeypatch, "scatter")
    with tracked(pkg, g, origin, inject, churn=1, p_fail=0.02, churn_seed=5, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_fresh(eng, exp)
        check_run(eng, stats, ref)
        # fresh_recv >= the first receipts that arrived (the messages lost at a down origin never existed)
        lost = ref["first"][origin, np.arange(m)] == 255
        own = np.bincount(origin[~lost], minlength=g.n)
        assert (eng.fresh_recv().astype(np.int64) >= eng.seenpop().astype(np.int64) - own).all()


def _crash_shapes(ref, g):
    got2 = np.nonzero((ref["first"] == 2).any(axis=1))[0][:20]
    assert got2.size == 20
    hub = int(np.argmax(np.diff(g.row_ptr)))
    return {"after-receipt": [(int(v), 2) for v in got2], "top-hub": [(hub, 2)]}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("which", ["after-receipt", "top-hub"])
def test_explicit_crashes(pkg, oracle, monkeypatch, which, mode, form):
    """A crash in the round right after a receipt -- the round the vertex would
    have sent in -- drops that frontier: k_churn zeroes its count, its frontier
    row is stale and must not be read, and what it received still counts as
    received.  A crash of the top hub takes the busiest receiver and sender
    out."""
    g, origin, inject, plain = _width_ref(4099, 100)
    crashes = _crash_shapes(plain, g)[which]
    ref = ds.CachedOracle(oracle).run(g, origin, inject, crashes=crashes, want_first=True)
    exp = expected(("crash", which), g, ref, crashes=crashes)
    if which == "after-receipt":
        vs = [v for v, _ in crashes]
        assert (ref["first"][vs] == 2).any()
        plain_exp = expected(("width", 4099, 100), g, plain)
        assert int(exp["sent"][vs].sum()) < int(plain_exp["sent"][vs].sum())   # the dropped frontiers delivered nothing
        assert int(exp["recv"][vs].sum()) > 0                                   # their receipts happened
    set_form(monkeypatch, form)
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject, crashes)
        check_fresh(eng, exp)
        check_run(eng, stats, ref)


# -- directed -----------------------------------------------------------------

@pytest.mark.parametrize("crash", [False, True], ids=["plain", "crash"])
@pytest.mark.parametrize("shape", ["down", "up", "first3"])
def test_directed(pkg, oracle, monkeypatch, shape, crash):
    """in-degree != out-degree: the receiver pass walks the in-CSR and adds the
    senders' side by atomics (hubs of the in-CSR through their items)"""
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
    assert int(exp["sent"].sum()) > 0
    set_form(monkeypatch, "gather")   # (a directed overlay scatters whatever the lever says)
    for hub_threshold in (64, 1 << 30):
        with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
            stats = run(eng, None, crashes)
            check_fresh(eng, exp)
            check_run(eng, stats, ref)


# -- aliased Message-Lists and receiver lists ----------------------------------

def test_aliases_and_receiver_lists(pkg, oracle, monkeypatch):
    """The shape of test_aliased_message_lists (W = 64): receivers that complete
    commit an alias of their component row and no row of their own -- their new
    bits must still be stored as a frontier row."""
    g = overlay(pkg, 120_000, 12, 2.4, 41)
    origin = pkg.overlay.random_origins(g.n, 4096, seed=41)
    ref = _alias_ref(pkg)
    exp = expected("alias", g, ref)
    set_form(monkeypatch, "scatter")
    with tracked(pkg, g, origin, None, push_ratio=0.0, unfiltered_pct=0, hub_threshold=1 << 30,
                 arc_mask_permille=0, compact_rows=0) as eng:
        stats = run(eng, None)
        assert sum(s["aliased"] for s in stats) > 0
        assert any(s["scan"] & 128 for s in stats)
        check_fresh(eng, exp)
        check_run(eng, stats, ref)


# -- message shards -----------------------------------------------------------

@pytest.mark.parametrize("blocks", [2, 4])
def test_message_shards_add_up(pkg, oracle, monkeypatch, blocks):
    g, origin, inject, ref = _width_ref(4099, 4096)
    exp = expected(("width", 4099, 4096), g, ref)
    set_form(monkeypatch, "scatter")
    sent = np.zeros(g.n, np.uint64)
    recv = np.zeros(g.n, np.uint64)
    digest = np.zeros(g.n, np.uint64)
    cuts = [0, 1024, 4096] if blocks == 2 else [0, 1024, 2048, 3072, 4096]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.track_fresh()
            eng.reset()
            run(eng, inject[lo:hi])
            sent += eng.fresh_sent()
            recv += eng.fresh_recv()
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
            digest ^= eng.digest()
    assert np.array_equal(sent.astype(np.int64), exp["sent"])
    assert np.array_equal(recv.astype(np.int64), exp["recv"])
    assert np.array_equal(digest, ref["digest"])


# -- tracking changes nothing else ----------------------------------------------

def _outputs(pkg, eng, inject):
    """every output of a run but the timings: counters of every round, seen,
    digest, coverage, forwards (or the status that refuses them), reports"""
    stats, reports = [], []
    last = int(np.max(inject))
    while not stats or stats[-1]["new_bits"] or stats[-1]["round"] < last:
        stats.append(eng.round())
        rows, _ = eng.reports()   # (of the round just run, unordered)
        reports.append(rows[np.lexsort(rows.T[::-1])])
    eng.finalize()
    out = {"stats": [{k: v for k, v in s.items() if not k.endswith("_ms")} for s in stats],
           "seen": eng.seen(), "digest": eng.digest(), "coverage": eng.coverage(),
           "reports": np.concatenate(reports)}
    for name in ("forwards", "frontier"):
        try:
            out[name] = getattr(eng, name)()
        except pkg.GossipError as e:
            out[name] = e.status
    return out


def _same(a, b, work_counters):
    assert a.keys() == b.keys()
    assert len(a["stats"]) == len(b["stats"])
    for x, y in zip(a["stats"], b["stats"]):
        assert set(STAT_KEYS) <= set(x)
        for k in (x if work_counters else STAT_KEYS):
            assert x[k] == y[k], (k, x["round"], x[k], y[k])
    for k in a:
        if k != "stats":
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_tracking_changes_nothing_else(pkg, oracle, monkeypatch, churn):
    """an untracked run, a run with gp_track_fresh, and one with the spread curve
    and the traffic record beside it: identical outputs and counters (with
    gp_track_fresh alone the work counters too, timings aside), and all three
    records correct together"""
    g, origin, inject, ref = _churn_ref(100) if churn else _width_ref(4099, 1000)
    kw = CHURN if churn else {}
    cfg = dict(churn=1, p_fail=0.02, churn_seed=5) if churn else {}
    exp = expected(("churn", 100) if churn else ("width", 4099, 1000), g, ref, **kw)
    set_form(monkeypatch, "scatter")
    outs = []
    for records in ((), ("fresh",), ("fresh", "curve", "load")):
        with pkg.GossipEngine(0, **cfg) as eng:
            eng.load_graph(g)
            eng.set_messages(origin, inject)
            for rec in records:
                getattr(eng, "track_" + rec)()
            eng.reset()
            outs.append(_outputs(pkg, eng, inject))
            if "fresh" in records:
                check_fresh(eng, exp)
            if "curve" in records:
                check_curve(eng.curve(), ref, inject)
            if "load" in records:
                load = load_ref.totals(g, ref, **kw)
                assert np.array_equal(eng.load_sent().astype(np.int64), load["sent"])
                assert np.array_equal(eng.load_recv().astype(np.int64), load["recv"])
                assert (eng.fresh_sent() <= eng.load_sent()).all() and (eng.fresh_recv() <= eng.load_recv()).all()
    # tracking makes neither GP_FRONTIER nor (under churn) GP_FORWARDS readable
    assert outs[0]["frontier"] == pkg._lib.GP_ENOTRACK
    _same(outs[0], outs[1], work_counters=True)
    # (the spread curve's frontier rows also feed the push, which moves its work counters: the exact ones)
    _same(outs[0], outs[2], work_counters=False)
    assert np.array_equal(outs[1]["seen"], ref["seen"][:, :outs[1]["seen"].shape[1]])
    assert np.array_equal(outs[1]["digest"], ref["digest"])


# -- lifecycle ----------------------------------------------------------------

def _status(pkg, fn):
    with pytest.raises(pkg.GossipError) as e:
        fn()
    return e.value.status


def test_errors_and_lifecycle(pkg, oracle, monkeypatch):
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = expected(("width", 4099, 100), g, ref)
    lib = pkg._lib
    set_form(monkeypatch, "scatter")
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        assert _status(pkg, eng.fresh_sent) == lib.GP_ENOTRACK     # not tracked
        eng.track_fresh()
        assert _status(pkg, eng.fresh_recv) == lib.GP_ENOTRACK     # takes effect at the next reset
        eng.reset()
        buf = np.full(g.n - 1, 77, np.uint64)                       # a short buffer: refused, nothing written
        assert eng._lib.gp_read(eng._ctx, lib.FRESH_SENT, buf.ctypes.data, buf.nbytes) == lib.GP_EINVAL
        assert (buf == 77).all()
        big = np.full(g.n + 1, 77, np.uint64)
        assert eng._lib.gp_read(eng._ctx, lib.FRESH_RECV, big.ctypes.data, big.nbytes) == lib.GP_EINVAL
        assert (big == 77).all()
        stats = run(eng, inject)
        check_fresh(eng, exp)
        check_run(eng, stats, ref)
        eng.reset()                                                 # a second run starts from zero
        assert not eng.fresh_sent().any() and not eng.fresh_recv().any()
        stats = [eng.round() for _ in range(3)]
        check_fresh(eng, dict(zip(("sent", "recv"), exp["per_round"][2])))
        eng.track_fresh(False)                                      # off again: at the next reset
        check_fresh(eng, dict(zip(("sent", "recv"), exp["per_round"][2])))
        eng.reset()
        assert _status(pkg, eng.fresh_sent) == lib.GP_ENOTRACK
        assert _status(pkg, eng.fresh_recv) == lib.GP_ENOTRACK
        stats = run(eng, inject)                                    # and the untracked run is the oracle's
        check_run(eng, stats, ref)
    # a run restored past round 0: its totals are not in the blob
    with tracked(pkg, g, origin, inject) as eng:
        blob0 = eng.checkpoint()
        stats = [eng.round() for _ in range(3)]
        blob3 = eng.checkpoint()
        with tracked(pkg, g, origin, inject) as other:
            other.restore(blob3)
            assert _status(pkg, other.fresh_sent) == lib.GP_ESTATE
            more = run(other, inject)
            assert _status(pkg, other.fresh_recv) == lib.GP_ESTATE
            check_run(other, stats + more, ref)                     # the restored run itself is exact
            other.reset()
            run(other, inject)
            check_fresh(other, exp)
            other.restore(blob0)                                    # a blob of round 0 has counted nothing yet
            run(other, inject)
            check_fresh(other, exp)


def test_partitioned_context_keeps_no_fresh(pkg, oracle):
    g, origin, inject, _ = _width_ref(4099, 100)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.track_fresh()
        eng.reset()
        assert _status(pkg, eng.fresh_sent) == pkg._lib.GP_ENOTRACK
        assert _status(pkg, eng.fresh_recv) == pkg._lib.GP_ENOTRACK
