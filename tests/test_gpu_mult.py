"""Delivery multiplicity (csrc/mult.hip, gp_track_mult, gp_read_mult_hist,
GP_SOLE_SENT / GP_SOLE_RECV, gp_read_sole_bins) against the CPU oracle.

mult_hist[c] counts the first receipts that c in-neighbours delivered in the
round they were news, sole_recv[v] the receipts of v with one deliverer and
sole_sent[u] the receipts u alone delivered: the arrival lines of one message
at one peer in one round (Peer.py:206, Peer.py:286), counted.  Every case
compares all four outputs exactly with tests/mult_ref.py, which evaluates the
first-receipt formula of DESIGN.md §2.4 on the oracle's outputs alone, and
checks that every other output of the tracked run equals the oracle's as
before.

The cases mirror tests/test_gpu_fresh.py one by one, with its shapes: 4,099
vertices (no multiple of a wave's 64 receivers) and 5 (fewer than one wave),
every row width, the five direction / scan modes (every commit path must store
the receivers' new rows), hubs split over items -- whose counters must be
merged before a count means anything -- and long rows walked by the main
kernel, churn and explicit crashes, directed overlays, aliased Message-Lists,
message shards, and the lifecycle.
"""
import numpy as np
import pytest

import directed_shapes as ds
import fresh_ref
import mult_ref
from test_gpu_curve import MODE_IDS, MODES, _alias_ref, _width_ref, check_run, mode_cfg, overlay, run
from test_gpu_fresh import CHURN, _churn_ref, _crash_shapes, _hub_ref, _outputs, _same, _status

pytestmark = pytest.mark.gpu


def tracked(pkg, g, origin, inject, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.track_mult()
    eng.reset()
    return eng


def check_mult(pkg, eng, g, exp):
    """all four outputs against the expected record (hist, sole_recv, sole_sent)"""
    hist, recv, sent, table = eng.mult_hist(), eng.sole_recv(), eng.sole_sent(), eng.sole_bins()
    assert hist.dtype == np.uint64 and hist.shape == (17,)
    assert recv.dtype == np.uint32 and sent.dtype == np.uint64 and recv.shape == sent.shape == (eng.n,)
    assert table.dtype == np.uint64 and table.shape == (32, 4)
    assert np.array_equal(hist.astype(np.int64), exp["hist"]), (hist.tolist(), exp["hist"].tolist())
    assert np.array_equal(recv.astype(np.int64), exp["sole_recv"]), np.nonzero(recv != exp["sole_recv"])[0][:8]
    assert np.array_equal(sent.astype(np.int64), exp["sole_sent"]), np.nonzero(sent.astype(np.int64) != exp["sole_sent"])[0][:8]
    seenpop = eng.seenpop()
    twin = pkg.fragility.bins(g.in_degree(), seenpop, exp["sole_recv"], exp["sole_sent"])
    assert np.array_equal(table, twin), np.argwhere(table != twin)[:8]
    assert int(table[:, 2].sum()) == int(table[:, 3].sum()) == int(exp["hist"][1])


def record(exp, r=None):
    if r is None:
        return exp
    return dict(zip(("hist", "sole_recv", "sole_sent"), exp["per_round"][r]))


_EXP = {}


def expected(key, g, ref, **kw):
    """mult_ref.totals, once per shape"""
    if key not in _EXP:
        _EXP[key] = mult_ref.totals(g, ref, **kw)
    return _EXP[key]


# -- sizes, widths, modes -----------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [1, 100, 1000, 4096])
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_modes(pkg, oracle, n, m, mode):
    g, origin, inject, ref = _width_ref(n, m)
    exp = expected(("width", n, m), g, ref)
    assert int(exp["hist"][1:].sum()) == sum(s["new_bits"] for s in ref["stats"])
    assert int(exp["hist"].sum()) == int(ref["coverage"].sum())
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_mult(pkg, eng, g, exp)
        check_mult(pkg, eng, g, exp)   # a read changes nothing
        check_run(eng, stats, ref)
        assert np.array_equal(eng.sole_bins(), mult_ref.table(g, eng.seenpop(), exp))   # (a loop over the vertices)


@pytest.mark.parametrize("m", [100, 4096])
def test_read_between_rounds(pkg, oracle, m):
    g, origin, inject, ref = _width_ref(4099, m)
    exp = expected(("width", 4099, m), g, ref)
    with tracked(pkg, g, origin, inject) as eng:
        assert not eng.sole_sent().any() and not eng.sole_recv().any() and not eng.mult_hist().any()
        assert not eng.sole_bins()[:, 1:].any() and int(eng.sole_bins()[:, 0].sum()) == g.n
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            check_mult(pkg, eng, g, record(exp, r))
            check_mult(pkg, eng, g, record(exp, r))   # a read changes nothing
            assert int(exp["per_round"][r][0][1:].sum()) == sum(s["new_bits"] for s in stats)
        check_run(eng, stats, ref)


# -- hubs ---------------------------------------------------------------------

@pytest.mark.parametrize("hub_threshold", [64, 1 << 30], ids=["split", "whole"])
def test_hubs(pkg, oracle, hub_threshold):
    """hub_threshold=64: the receivers above 64 arcs are counted item by item
    and their counters merged (k_mult_hub, k_mult_hub_final, k_mult_hub_sole);
    1 << 30: nothing is split and the main kernel walks the long rows."""
    g, origin, ref = _hub_ref()
    assert np.diff(g.row_ptr).max() > 1000
    exp = expected("hub", g, ref, chunk=64)
    # before the engine is touched: the split receivers have receipts in every bin, and
    # receipts whose 2 .. 15 deliverers lie in different items
    big = exp["big_hist"]
    assert big[1] == 18129 and big[16] == 9436 and (big[2:16] > 0).all()
    assert exp["cross"] == 17809
    g100, _, _, ref100 = _width_ref(4099, 100)
    small = expected(("width", 4099, 100, "chunk"), g100, ref100, chunk=64)
    assert (small["big_hist"][1], small["big_hist"][16], small["cross"]) == (1619, 378, 1331)
    with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
        stats = run(eng, None)
        check_mult(pkg, eng, g, exp)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("m", [100, 1000])
def test_hubs_every_width_between_rounds(pkg, oracle, m):
    """the 4099-vertex shape with its hubs split, read after every round"""
    g, origin, inject, ref = _width_ref(4099, m)
    assert np.diff(g.row_ptr).max() > 4 * 64
    exp = expected(("width", 4099, m), g, ref)
    with tracked(pkg, g, origin, inject, hub_threshold=64) as eng:
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            check_mult(pkg, eng, g, record(exp, r))
        check_run(eng, stats, ref)


# -- liveness -----------------------------------------------------------------

@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("m", [100, 1000])
def test_churn(pkg, oracle, m, mode):
    g, origin, inject, ref = _churn_ref(m)
    tot = {k: sum(s[k] for s in ref["stats"]) for k in ("crashed", "removals", "lost", "new_bits", "injected")}
    assert tot["crashed"] > 0 and tot["removals"] > 0 and tot["lost"] > 0
    exp = expected(("churn", m), g, ref, **CHURN)
    assert int(exp["hist"][1:].sum()) == tot["new_bits"] and int(exp["hist"][0]) == tot["injected"]
    with tracked(pkg, g, origin, inject, churn=1, p_fail=0.02, churn_seed=5, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_mult(pkg, eng, g, exp)
        check_run(eng, stats, ref)
        # sole_recv <= the first receipts that arrived (the messages lost at a down origin never existed)
        lost = ref["first"][origin, np.arange(m)] == 255
        own = np.bincount(origin[~lost], minlength=g.n)
        assert (eng.sole_recv().astype(np.int64) <= eng.seenpop().astype(np.int64) - own).all()


@pytest.mark.parametrize("hub_threshold", [64, 1 << 30], ids=["split", "whole"])
@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("which", ["after-receipt", "top-hub"])
def test_explicit_crashes(pkg, oracle, which, mode, hub_threshold):
    """A crash in the round right after a receipt -- the round the vertex would
    have sent in -- drops that frontier: k_churn zeroes its count, its frontier
    row is stale and must not be read, so it is nobody's deliverer, and what it
    received still counts as received.  A crash of the top hub takes the busiest
    receiver and sender out."""
    g, origin, inject, plain = _width_ref(4099, 100)
    crashes = _crash_shapes(plain, g)[which]
    ref = ds.CachedOracle(oracle).run(g, origin, inject, crashes=crashes, want_first=True)
    exp = expected(("crash", which), g, ref, crashes=crashes)
    plain_exp = expected(("width", 4099, 100), g, plain)
    assert not np.array_equal(exp["hist"], plain_exp["hist"])
    if which == "after-receipt":
        vs = [v for v, _ in crashes]
        assert (ref["first"][vs] == 2).any()
        assert int(exp["sole_recv"][vs].sum()) > 0                             # their receipts happened
    with tracked(pkg, g, origin, inject, hub_threshold=hub_threshold, **mode_cfg(mode)) as eng:
        stats = run(eng, inject, crashes)
        check_mult(pkg, eng, g, exp)
        check_run(eng, stats, ref)


# -- directed -----------------------------------------------------------------

@pytest.mark.parametrize("crash", [False, True], ids=["plain", "crash"])
@pytest.mark.parametrize("shape", ["down", "up", "first3"])
def test_directed(pkg, oracle, shape, crash):
    """in-degree != out-degree: the pass walks the in-CSR alone and adds the
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
    assert int(exp["sole_sent"].sum()) > 0
    assert shape == "first3" or int(exp["hist"][2:].sum()) > 0   # (3000 first3 peers, 300 messages: every receipt is sole)
    for hub_threshold in (64, 1 << 30):
        with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
            stats = run(eng, None, crashes)
            check_mult(pkg, eng, g, exp)
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
        check_mult(pkg, eng, g, exp)
        check_run(eng, stats, ref)


# -- message shards -----------------------------------------------------------

@pytest.mark.parametrize("blocks", [2, 4])
def test_message_shards_add_up(pkg, oracle, blocks):
    g, origin, inject, ref = _width_ref(4099, 4096)
    exp = expected(("width", 4099, 4096), g, ref)
    sent = np.zeros(g.n, np.uint64)
    recv = np.zeros(g.n, np.uint64)
    hists, tables = [], []
    digest = np.zeros(g.n, np.uint64)
    cuts = [0, 1024, 4096] if blocks == 2 else [0, 1024, 2048, 3072, 4096]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.track_mult()
            eng.reset()
            run(eng, inject[lo:hi])
            sent += eng.sole_sent()
            recv += eng.sole_recv()
            hists.append(eng.mult_hist())
            tables.append(eng.sole_bins())
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
            assert int(hists[-1].sum()) == int(ref["coverage"][lo:hi].sum())
            digest ^= eng.digest()
    assert np.array_equal(sent.astype(np.int64), exp["sole_sent"])
    assert np.array_equal(recv.astype(np.int64), exp["sole_recv"])
    assert np.array_equal(pkg.fragility.combine(hists).astype(np.int64), exp["hist"])
    assert np.array_equal(sum(t[:, 1:] for t in tables), pkg.fragility.bins(
        g.in_degree(), (ref["first"] != 255).sum(axis=1), exp["sole_recv"], exp["sole_sent"])[:, 1:])
    assert np.array_equal(digest, ref["digest"])


# -- identities on the device ---------------------------------------------------

@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_identities_on_the_device(pkg, oracle, churn):
    g, origin, inject, ref = _churn_ref(1000) if churn else _width_ref(4099, 1000)
    cfg = dict(churn=1, p_fail=0.02, churn_seed=5) if churn else {}
    with pkg.GossipEngine(0, hub_threshold=64, **cfg) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.track_mult()
        eng.track_fresh()
        eng.reset()
        stats = run(eng, inject)
        hist, sr, ss = eng.mult_hist().astype(np.int64), eng.sole_recv().astype(np.int64), eng.sole_sent().astype(np.int64)
        fr, fs = eng.fresh_recv().astype(np.int64), eng.fresh_sent().astype(np.int64)
        table = eng.sole_bins()
        seenpop = eng.seenpop().astype(np.int64)
        eng.finalize()
        assert int(hist.sum()) == int(eng.coverage().sum())
        assert int(hist[1:].sum()) == sum(s["new_bits"] for s in stats)
        assert int(hist[0]) == sum(s["injected"] for s in stats)
        assert int(hist[1]) == int(sr.sum()) == int(ss.sum()) > 0
        injected = ref["first"][origin, np.arange(len(origin))] != 255
        assert (sr <= seenpop - np.bincount(origin[injected], minlength=g.n)).all()
        assert (sr <= fr).all() and (ss <= fs).all()
        assert sum(c * int(hist[c]) for c in range(1, 17)) <= int(fr.sum())
        assert hist[16] > 0 and hist[2:16].all()
        assert np.array_equal(table, pkg.fragility.bins(g.in_degree(), seenpop, sr, ss))
        fexp = fresh_ref.totals(g, ref, **(CHURN if churn else {}))
        assert np.array_equal(fr, fexp["recv"]) and np.array_equal(fs, fexp["sent"])   # both records, together
        rows = pkg.fragility.by_degree(table)
        assert sum(x["peers"] for x in rows) == g.n
        assert pkg.fragility.sole_share(hist) == int(hist[1]) / int(hist[1:].sum())
        assert pkg.fragility.at_least(hist, 2) == int(hist[2:].sum())


# -- tracking changes nothing else ----------------------------------------------

@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_tracking_changes_nothing_else(pkg, oracle, churn):
    """an untracked run and a run with gp_track_mult: identical outputs and
    counters, the work counters included (timings aside)"""
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
                eng.track_mult()
            eng.reset()
            outs.append(_outputs(pkg, eng, inject))
            if on:
                check_mult(pkg, eng, g, exp)
    # tracking makes neither GP_FRONTIER nor (under churn) GP_FORWARDS readable
    assert outs[0]["frontier"] == outs[1]["frontier"] == pkg._lib.GP_ENOTRACK
    _same(outs[0], outs[1], work_counters=True)
    assert np.array_equal(outs[1]["seen"], ref["seen"][:, :outs[1]["seen"].shape[1]])
    assert np.array_equal(outs[1]["digest"], ref["digest"])


# -- lifecycle ----------------------------------------------------------------

def test_errors_and_lifecycle(pkg, oracle):
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = expected(("width", 4099, 100), g, ref)
    lib = pkg._lib
    reads = ("sole_sent", "sole_recv", "mult_hist", "sole_bins")
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        for name in reads:                                          # off by default
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        eng.track_mult()
        for name in reads:                                          # takes effect at the next reset
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        eng.reset()
        buf = np.full(g.n - 1, 77, np.uint64)                       # a short buffer: refused, nothing written
        assert eng._lib.gp_read(eng._ctx, lib.SOLE_SENT, buf.ctypes.data, buf.nbytes) == lib.GP_EINVAL
        assert (buf == 77).all()
        big = np.full(g.n + 1, 77, np.uint32)
        assert eng._lib.gp_read(eng._ctx, lib.SOLE_RECV, big.ctypes.data, big.nbytes) == lib.GP_EINVAL
        assert (big == 77).all()
        wrong = np.full(g.n, 77, np.uint32)                         # the other array's width
        assert eng._lib.gp_read(eng._ctx, lib.SOLE_SENT, wrong.ctypes.data, wrong.nbytes) == lib.GP_EINVAL
        assert (wrong == 77).all()
        h = np.full(32 * 4, 77, np.uint64)
        for bins in (16, 18, 0):
            assert eng._lib.gp_read_mult_hist(eng._ctx, h.ctypes.data, bins) == lib.GP_EINVAL
        for bins in (31, 33, 17):
            assert eng._lib.gp_read_sole_bins(eng._ctx, h.ctypes.data, bins) == lib.GP_EINVAL
        assert (h == 77).all()
        assert eng._lib.gp_read_mult_hist(eng._ctx, None, 17) == lib.GP_EINVAL
        assert eng._lib.gp_read_sole_bins(eng._ctx, None, 32) == lib.GP_EINVAL
        assert eng._lib.gp_track_mult(None, 1) == lib.GP_EINVAL
        stats = run(eng, inject)
        check_mult(pkg, eng, g, exp)
        check_run(eng, stats, ref)
        eng.reset()                                                 # a second run starts from zero
        assert not eng.sole_sent().any() and not eng.sole_recv().any() and not eng.mult_hist().any()
        stats = [eng.round() for _ in range(3)]
        check_mult(pkg, eng, g, record(exp, 2))
        eng.track_mult(False)                                       # off again: at the next reset
        check_mult(pkg, eng, g, record(exp, 2))
        eng.reset()
        for name in reads:
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        stats = run(eng, inject)                                    # and the untracked run is the oracle's
        check_run(eng, stats, ref)
        # another overlay and another message table re-size the record and the hubs' scratch
        g2, origin2, inject2, ref2 = _width_ref(5, 1000)
        eng.track_mult()
        eng.load_graph(g2)
        eng.set_messages(origin2, inject2)
        eng.reset()
        stats = run(eng, inject2)
        check_mult(pkg, eng, g2, expected(("width", 5, 1000), g2, ref2))
        check_run(eng, stats, ref2)
    with pkg.GossipEngine(0, hub_threshold=64) as eng:             # ... with hubs: 5 -> 4099 vertices, W = 16 -> 2
        g2, origin2, inject2, ref2 = _width_ref(5, 1000)
        eng.load_graph(g2)
        eng.set_messages(origin2, inject2)
        eng.track_mult()
        eng.reset()
        eng.round()
        check_mult(pkg, eng, g2, record(expected(("width", 5, 1000), g2, ref2), 0))
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        stats = run(eng, inject)
        check_mult(pkg, eng, g, exp)
        check_run(eng, stats, ref)
    # a run restored past round 0: its record is not in the blob
    with tracked(pkg, g, origin, inject) as eng:
        blob0 = eng.checkpoint()
        stats = [eng.round() for _ in range(3)]
        blob3 = eng.checkpoint()
        with tracked(pkg, g, origin, inject) as other:
            other.restore(blob3)
            for name in reads:
                assert _status(pkg, getattr(other, name)) == lib.GP_ESTATE
            more = run(other, inject)
            assert _status(pkg, other.sole_recv) == lib.GP_ESTATE
            check_run(other, stats + more, ref)                     # the restored run itself is exact
            other.reset()
            run(other, inject)
            check_mult(pkg, other, g, exp)
            other.restore(blob0)                                    # a blob of round 0 has counted nothing yet
            run(other, inject)
            check_mult(pkg, other, g, exp)


def test_partitioned_context_keeps_no_mult(pkg, oracle):
    g, origin, inject, _ = _width_ref(4099, 100)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.track_mult()
        eng.reset()
        for name in ("sole_sent", "sole_recv", "mult_hist", "sole_bins"):
            assert _status(pkg, getattr(eng, name)) == pkg._lib.GP_ENOTRACK
