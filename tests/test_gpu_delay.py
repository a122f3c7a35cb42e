"""Per-peer receipt delays (csrc/delay.hip, gp_track_delay, GP_DELAY_SUM /
GP_DELAY_MAX, gp_read_delay_bins) against the CPU oracle.

delay_sum[v] and delay_max[v] are the sum and the maximum of first[v][k] -
inject_round[k] over the messages v holds: the time column of the reference's
arrival logs (Peer.py:206, Peer.py:286) grouped by the receiving peer.  Every
case compares both arrays and seenpop() exactly with tests/delay_ref.py, which
evaluates the formula of DESIGN.md §2.4 on the oracle's first-receipt matrix
alone, delay_bins() exactly with latency.bins of the arrays read and with
delay_ref.bins, and checks that every other output of the tracked run equals
the oracle's as before.  No tolerance anywhere.

Shapes are the smallest that reach each path: 4,099 vertices (no multiple of a
wave's 64) and 5 (fewer than one wave), every row width with partial last
words, the five direction / scan modes on a table with several inject rounds
(the row pass) and on one with a single inject round (the pass over the
per-vertex counts alone, which relies on every commit path storing |new_r(v)|),
inject rounds with every bit 0-7 set, hubs committed by k_hub_final, churn and
a crash right after a receipt, aliased Message-Lists and receiver lists,
directed overlays, message shards, a vertex partition, and the lifecycle.
"""
import functools

import numpy as np
import pytest

import delay_ref
import directed_shapes as ds
from test_gpu_curve import MODE_IDS, MODES, STAT_KEYS, _alias_ref, _width_ref, check_run, mode_cfg, overlay, run
from test_gpu_fresh import CHURN, _churn_ref, _status

pytestmark = pytest.mark.gpu

WIDTH_MS = [1, 64, 100, 512, 1000, 2048, 4096]
WORDS = {1: 1, 64: 1, 100: 2, 512: 8, 1000: 16, 2048: 32, 4096: 64}


def tracked(pkg, g, origin, inject, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.track_delay()
    eng.reset()
    return eng


def check_delay(eng, exp):
    """delay_sum(), delay_max() and seenpop() against (sum, max, seenpop)"""
    s, mx, sp = eng.delay_sum(), eng.delay_max(), eng.seenpop()
    assert s.dtype == np.uint32 and mx.dtype == np.uint8 and s.shape == mx.shape == exp[0].shape
    for name, got, want in (("sum", s, exp[0]), ("max", mx, exp[1]), ("seenpop", sp, exp[2])):
        bad = np.nonzero(got.astype(np.int64) != want)[0]
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])
    return s, mx, sp


def check_bins(pkg, eng, deg, arrays, want=None):
    t = eng.delay_bins()
    assert t.dtype == np.uint64 and t.shape == (32, 5)
    s, mx, sp = arrays
    assert np.array_equal(t, pkg.latency.bins(deg, sp, s, mx))
    if want is not None:
        assert np.array_equal(t, want)
    return t


def final(exp):
    return exp["sum"], exp["max"], exp["seenpop"]


@functools.lru_cache(maxsize=None)
def _exp(n, m, uniform):
    """(g, origin, inject, ref, delay_ref.totals) of _width_ref's shape; uniform:
    the same overlay and origins with every message injected in round 0"""
    g, origin, inject, ref = _width_ref(n, m)
    if uniform:
        from oracle import lib
        inject, ref = None, lib.run(g, origin, None, want_first=True)
    return g, origin, inject, ref, delay_ref.totals(ref, inject)


# -- sizes, widths, modes -------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", WIDTH_MS)
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_modes_rows(pkg, oracle, n, m, mode):
    """inject = k % 3: the row pass (k_delay<W>)"""
    g, origin, inject, ref, exp = _exp(n, m, False)
    if n == 4099 and m >= 100:
        assert len(set(exp["max"].tolist())) >= 6 and (np.diff(g.row_ptr) == 0).sum() > 100
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        assert eng.info()[3] == WORDS[m]
        stats = run(eng, inject)
        check_delay(eng, final(exp))
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", WIDTH_MS)
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_modes_uniform(pkg, oracle, n, m, mode):
    """every message injected in round 0: the pass over the guard words alone
    (k_delay_uniform) -- exact iff every commit path of the mode stores the
    exact |new_r(v)|"""
    g, origin, inject, ref, exp = _exp(n, m, True)
    with tracked(pkg, g, origin, None, **mode_cfg(mode)) as eng:
        stats = run(eng, None)
        s, mx, _ = check_delay(eng, final(exp))
        # one inject round: the sum is the receipts weighted by their round
        assert int(s.astype(np.int64).sum()) == sum((r + 1) * st["new_bits"] for r, st in enumerate(stats))
        check_run(eng, stats, ref)


def test_uniform_table_keeps_no_frontier_rows(pkg, oracle, monkeypatch):
    """a checkpoint holds the frontier rows a context keeps: tracking a table
    with one inject round adds none, a table with several (or GP_DELAY_ROWS=1)
    adds them"""
    g, origin, inject, _, _ = _exp(4099, 100, False)

    def blob_bytes(inj, track):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_messages(origin, inj)
            eng.track_delay(track)
            eng.reset()
            return eng.checkpoint().size

    rows = g.n * 2 * 8   # [n][W = 2] u64
    assert blob_bytes(None, True) == blob_bytes(None, False)
    assert blob_bytes(inject, True) == blob_bytes(inject, False) + rows
    monkeypatch.setenv("GP_DELAY_ROWS", "1")
    assert blob_bytes(None, True) == blob_bytes(None, False) + rows


@pytest.mark.parametrize("mode", [MODES[0], MODES[4]], ids=["pull", "adaptive"])
def test_one_inject_round_and_one_message_moved(pkg, oracle, mode):
    """every inject round = 2 (uniform path, nothing happens in rounds 0 and 1),
    then the same table with one message moved to round 0 (the row pass)"""
    g, origin, _, _ = _width_ref(4099, 100)
    for moved in (False, True):
        inject = np.full(100, 2, np.int32)
        if moved:
            inject[17] = 0
        ref = oracle.run(g, origin, inject, want_first=True)
        exp = delay_ref.totals(ref, inject)
        with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
            stats = run(eng, inject)
            check_delay(eng, final(exp))
            check_run(eng, stats, ref)


# -- high planes ----------------------------------------------------------------

def test_inject_rounds_up_to_200(pkg, oracle):
    """inject = 37 k % 201: every plane 0-7 holds messages, about 210 rounds"""
    g, origin, _, _ = _width_ref(4099, 100)
    inject = ((37 * np.arange(100)) % 201).astype(np.int32)
    assert all(((inject >> b) & 1).any() for b in range(8))
    ref = oracle.run(g, origin, inject, want_first=True)
    assert ref["rounds"] > 200
    exp = delay_ref.totals(ref, inject)
    with tracked(pkg, g, origin, inject) as eng:
        stats = run(eng, inject)
        check_delay(eng, final(exp))
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
def test_c1_schedule_and_reset(pkg, oracle, mode):
    """test_injections_and_reset's c1 schedule (inject up to 45, 10 messages per
    origin), and a second run after reset(): nothing stale survives it"""
    g = overlay(pkg, 4099)
    origin, inject, _ = pkg.peer.c1_schedule(10)
    origin, inject = np.array(origin, np.int32) * 400 + 3, np.array(inject, np.int32)
    assert inject.max() == 45
    ref = ds.CachedOracle(oracle).run(g, origin, inject, want_first=True)
    exp = delay_ref.totals(ref, inject)
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        first_run = check_delay(eng, final(exp))
        check_run(eng, stats, ref)
        eng.reset()
        assert not eng.delay_sum().any() and not eng.delay_max().any()
        run(eng, inject)
        for a, b in zip(check_delay(eng, final(exp)), first_run):
            assert np.array_equal(a, b)


# -- hubs -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
@pytest.mark.parametrize("m", [100, 4096])
def test_hub_commits_feed_the_record(pkg, oracle, m, uniform, mode):
    """hub_threshold=64: the receivers k_hub_final commits are counted too"""
    g, origin, inject, ref, exp = _exp(4099, m, uniform)
    assert np.diff(g.row_ptr).max() > 4 * 64
    with tracked(pkg, g, origin, inject, hub_threshold=64, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_delay(eng, final(exp))
        check_run(eng, stats, ref)


# -- liveness -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _churn_uniform_ref(m):
    from oracle import lib
    g, origin, _, _ = _churn_ref(m)
    return lib.run(g, origin, None, want_first=True, **CHURN)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
@pytest.mark.parametrize("m", [100, 1000])
def test_churn(pkg, oracle, m, uniform, mode):
    g, origin, inject, ref = _churn_ref(m)
    if uniform:
        inject, ref = None, _churn_uniform_ref(m)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0
    exp = delay_ref.totals(ref, inject)
    with tracked(pkg, g, origin, inject, churn=1, p_fail=0.02, churn_seed=5, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        arrays = check_delay(eng, final(exp))
        check_bins(pkg, eng, np.diff(g.row_ptr), arrays, delay_ref.bins(g, ref, inject))
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
def test_crash_right_after_receipt(pkg, oracle, uniform, mode):
    """20 vertices with a first receipt in round 2 crash in round 2: k_churn
    zeroes their frontier counts before they send; what they received still
    counts as received, with its delay"""
    g, origin, inject, plain, _ = _exp(4099, 100, uniform)
    picked = np.nonzero((plain["first"] == 2).any(axis=1))[0][:20]
    assert picked.size == 20
    crashes = [(int(v), 2) for v in picked]
    ref = ds.CachedOracle(oracle).run(g, origin, inject, crashes=crashes, want_first=True)
    assert (ref["first"][picked] == 2).any() and not np.array_equal(ref["forwards"], plain["forwards"])
    exp = delay_ref.totals(ref, inject)
    assert (exp["sum"][picked] > 0).any()
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject, crashes)
        check_delay(eng, final(exp))
        check_run(eng, stats, ref)


# -- aliased Message-Lists and receiver lists -------------------------------------

@functools.lru_cache(maxsize=None)
def _alias_exp(pkg):
    return delay_ref.totals(_alias_ref(pkg), None)


@pytest.mark.parametrize("mode", ["pull", "adaptive"])
@pytest.mark.parametrize("path", ["uniform", "rows"])
def test_aliases_and_receiver_lists(pkg, oracle, monkeypatch, path, mode):
    """The shape of test_aliased_message_lists (W = 64): receivers that complete
    commit an alias of their component row and no row of their own, and the
    last pulls take their receivers from a list -- their counts and their new
    rows must still be stored.  The table has one inject round; GP_DELAY_ROWS=1
    runs the row pass on it."""
    push_ratio, unfiltered_pct, hub = {"pull": (0.0, 0, 1 << 30), "adaptive": (10.0, 90, 4096)}[mode]
    g = overlay(pkg, 120_000, 12, 2.4, 41)
    origin = pkg.overlay.random_origins(g.n, 4096, seed=41)
    ref, exp = _alias_ref(pkg), _alias_exp(pkg)
    if path == "rows":
        monkeypatch.setenv("GP_DELAY_ROWS", "1")
    with tracked(pkg, g, origin, None, push_ratio=push_ratio, unfiltered_pct=unfiltered_pct, hub_threshold=hub,
                 arc_mask_permille=0, compact_rows=0) as eng:
        stats = run(eng, None)
        assert sum(s["aliased"] for s in stats) > 0
        assert any(s["scan"] & 64 for s in stats)
        assert any(s["scan"] & 128 for s in stats)
        arrays = check_delay(eng, final(exp))
        check_bins(pkg, eng, np.diff(g.row_ptr), arrays)
        check_run(eng, stats, ref)


# -- directed overlays ------------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
def test_directed(pkg, oracle, uniform):
    """in-degree != out-degree: the delays follow the arcs' direction, and the
    bins use the in-list length"""
    co = ds.CachedOracle(oracle)
    g = ds.oriented_chung_lu(pkg, co, 20_000, 8, 2.2, 11, "down")
    assert not np.array_equal(g.in_degree(), g.out_degree())
    origin = pkg.overlay.random_origins(g.n, 256, seed=11)
    inject = None if uniform else (np.arange(256) % 4).astype(np.int32)
    ref = co.run(g, origin, inject, want_first=True)
    exp = delay_ref.totals(ref, inject)
    assert int(exp["sum"].sum()) > 0
    with tracked(pkg, g, origin, inject, hub_threshold=64) as eng:
        stats = run(eng, inject)
        arrays = check_delay(eng, final(exp))
        check_bins(pkg, eng, g.in_degree(), arrays, delay_ref.bins(g, ref, inject))
        check_run(eng, stats, ref)


# -- reads between rounds ---------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
@pytest.mark.parametrize("m", [100, 4096])
def test_read_between_rounds(pkg, oracle, m, uniform):
    g, origin, inject, ref, exp = _exp(4099, m, uniform)
    zero = np.zeros(g.n, np.int64)
    with tracked(pkg, g, origin, inject) as eng:
        check_delay(eng, (zero, zero, zero))   # nothing before round 0
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            want = exp["per_round"][r]
            check_delay(eng, want)
            before = eng.delay_bins()
            check_delay(eng, want)             # a read changes nothing
            assert np.array_equal(eng.delay_bins(), before)
        check_delay(eng, final(exp))
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_stopping_after_two_rounds(pkg, oracle, mode):
    g, origin, inject, ref, exp = _exp(4099, 1000, False)
    cut = delay_ref.totals(ref, inject, rounds=2)
    assert 0 < int(cut["sum"].sum()) < int(exp["sum"].sum())
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = [eng.round(), eng.round()]
        arrays = check_delay(eng, final(cut))
        check_bins(pkg, eng, np.diff(g.row_ptr), arrays, delay_ref.bins(g, ref, inject, rounds=2))
        while not (stats[-1]["new_bits"] == 0 and stats[-1]["round"] >= 2):
            stats.append(eng.round())
        check_delay(eng, final(exp))
        check_run(eng, stats, ref)


# -- message shards ---------------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
def test_message_shards(pkg, oracle, uniform):
    """two contexts with the word-aligned halves of the 4,096-message table:
    each holds its own messages' terms (planes of its own table), the sums add
    to the single-context result and the maxima combine element-wise"""
    g, origin, inject, ref, exp = _exp(4099, 4096, uniform)
    total = np.zeros(g.n, np.int64)
    most = np.zeros(g.n, np.int64)
    tables = []
    for lo, hi in ((0, 2048), (2048, 4096)):
        inj = None if inject is None else inject[lo:hi]
        part = delay_ref.totals({"first": ref["first"][:, lo:hi], "rounds": ref["rounds"]}, inj)
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.track_delay()
            eng.reset()
            run(eng, inj)
            s, mx, sp = check_delay(eng, final(part))
            tables.append(check_bins(pkg, eng, np.diff(g.row_ptr), (s, mx, sp)))
            total += s
            most = np.maximum(most, mx)
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
    assert np.array_equal(total, exp["sum"]) and np.array_equal(most, exp["max"])
    whole = delay_ref.bins(g, ref, inject)
    both = pkg.latency.combine(tables, disjoint=False)
    assert np.array_equal(both[:, [0, 2, 3, 4]], whole[:, [0, 2, 3, 4]])


# -- vertex partition -------------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_partition(pkg, oracle, churn, uniform):
    """Three contexts of a vertex partition on one GPU: each keeps the record
    of its owned vertices; the slices concatenate to the oracle's, the tables
    add up (the maxima combine) to the whole overlay's."""
    g = pkg.overlay.barabasi_albert(3001, 2, seed=8)
    origin = pkg.overlay.random_origins(g.n, 200, seed=8)
    inject = np.zeros(200, np.int32) if uniform else (np.arange(200) % 4).astype(np.int32)
    kw = dict(churn=True, p_fail=0.02, churn_seed=3) if churn else {}
    cfg = dict(churn=1, p_fail=0.02, churn_seed=3, track_msg_forwards=1) if churn else {}
    ref = oracle.run(g, origin, inject, want_first=True, **kw)
    exp = delay_ref.totals(ref, inject)
    engs = []
    for k in range(3):
        e = pkg.GossipEngine(0, **cfg)
        e.load_graph(g)
        e.set_partition(k, 3)
        e.set_messages(origin, inject)
        e.track_delay()
        e.reset()
        engs.append(e)
    stats = pkg.GossipEngine.run_group(engs)
    assert len(stats) == ref["rounds"]
    for a, b in zip(stats, ref["stats"]):
        for k in STAT_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    deg = np.diff(g.row_ptr)
    tables, sums, maxes = [], [], []
    for e in engs:
        lo, hi = e.partition()
        arrays = check_delay(e, tuple(x[lo:hi] for x in final(exp)))
        tables.append(check_bins(pkg, e, deg[lo:hi], arrays, delay_ref.bins(g, ref, inject, lo=lo, hi=hi)))
        sums.append(arrays[0])
        maxes.append(arrays[1])
    assert np.array_equal(np.concatenate(sums), exp["sum"]) and np.array_equal(np.concatenate(maxes), exp["max"])
    assert np.array_equal(pkg.latency.combine(tables), delay_ref.bins(g, ref, inject))
    for e in engs:
        e.close()


# -- bins -------------------------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
@pytest.mark.parametrize("n,m", [(4099, 100), (4099, 4096), (5, 100)])
def test_bins(pkg, oracle, n, m, uniform):
    g, origin, inject, ref, exp = _exp(n, m, uniform)
    want = delay_ref.bins(g, ref, inject)
    if n == 4099:
        assert (want[:10, 0] > 0).all() and not want[10:].any()   # degrees 0 .. 913: bins 0-9
        assert want[0, 1] < want[0, 0]                             # the degree-0 vertices are never reached
    with tracked(pkg, g, origin, inject) as eng:
        zero = np.zeros(g.n, np.int64)
        check_bins(pkg, eng, np.diff(g.row_ptr), (zero, zero, zero))   # peers alone before round 0
        run(eng, inject)
        t = check_bins(pkg, eng, np.diff(g.row_ptr), check_delay(eng, final(exp)), want)
        assert int(t[:, 0].sum()) == g.n and int(t[:, 3].sum()) == int(exp["sum"].sum())
        if n == 4099:   # hubs hear early, leaves late
            rows = pkg.latency.by_degree(t)
            assert rows[-1]["mean_delay"] < rows[1]["mean_delay"]


def test_identity_with_the_spread_curve(pkg, oracle):
    g, origin, inject, ref, exp = _exp(4099, 1000, False)
    with tracked(pkg, g, origin, inject) as eng:
        eng.track_curve()
        eng.reset()
        for r in range(ref["rounds"]):
            eng.round()
            assert int(eng.delay_sum().astype(np.int64).sum()) == pkg.latency.total_delay(eng.curve(), inject)
        check_delay(eng, final(exp))
        hist = pkg.latency.delay_hist(eng.curve(), inject)
        assert int(np.nonzero(hist)[0].max()) == int(eng.delay_max().max())


# -- lifecycle --------------------------------------------------------------------

def test_errors_and_lifecycle(pkg, oracle):
    g, origin, inject, ref, exp = _exp(4099, 100, False)
    lib = pkg._lib
    reads = ("delay_sum", "delay_max", "delay_bins")
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        for name in reads:                                          # off by default
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        eng.track_delay()
        for name in reads:                                          # takes effect at the next reset
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        eng.reset()
        for what, dtype in ((lib.DELAY_SUM, np.uint32), (lib.DELAY_MAX, np.uint8)):
            for size in (g.n - 1, g.n + 1):                         # a wrong byte count: refused, nothing written
                buf = np.full(size, 77, dtype)
                assert eng._lib.gp_read(eng._ctx, what, buf.ctypes.data, buf.nbytes) == lib.GP_EINVAL
                assert (buf == 77).all()
        for bins in (31, 33, 0):                                    # a wrong bin count
            tb = np.full((33, 5), 77, np.uint64)
            assert eng._lib.gp_read_delay_bins(eng._ctx, tb.ctypes.data, bins) == lib.GP_EINVAL
            assert (tb == 77).all()
        assert eng._lib.gp_read_delay_bins(eng._ctx, None, 32) == lib.GP_EINVAL   # a null argument
        assert eng._lib.gp_track_delay(None, 1) == lib.GP_EINVAL
        stats = run(eng, inject)
        check_delay(eng, final(exp))
        check_run(eng, stats, ref)
        eng.reset()                                                 # a second run starts from zero
        for _ in range(3):
            eng.round()
        check_delay(eng, exp["per_round"][2])
        eng.track_delay(False)                                      # off again: at the next reset
        check_delay(eng, exp["per_round"][2])
        eng.reset()                                                 # (which frees the record)
        for name in reads:
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        stats = run(eng, inject)                                    # and the untracked run is the oracle's
        check_run(eng, stats, ref)
    with tracked(pkg, g, origin, inject) as eng:
        blob0 = eng.checkpoint()
        stats = [eng.round() for _ in range(3)]
        blob3 = eng.checkpoint()
        with tracked(pkg, g, origin, inject) as other:
            other.restore(blob3)                                    # past round 0: the record is not in the blob
            for name in reads:
                assert _status(pkg, getattr(other, name)) == lib.GP_ESTATE
            more = run(other, inject)
            assert _status(pkg, other.delay_sum) == lib.GP_ESTATE
            check_run(other, stats + more, ref)                     # the restored run itself is exact
            other.reset()
            run(other, inject)
            check_delay(other, final(exp))
            other.restore(blob0)                                    # a blob of round 0 has counted nothing yet
            run(other, inject)
            check_delay(other, final(exp))


def test_table_change_switches_the_path(pkg, oracle):
    """one context, tracking left on: a table with one inject round, then one
    with several (the reset makes the frontier rows), then the first again"""
    g, origin, inject, ref, exp = _exp(4099, 100, False)
    _, _, _, uref, uexp = _exp(4099, 100, True)
    with tracked(pkg, g, origin, None) as eng:
        for inj, r, e in ((None, uref, uexp), (inject, ref, exp), (None, uref, uexp)):
            eng.set_messages(origin, inj)
            eng.reset()
            stats = run(eng, inj)
            check_delay(eng, final(e))
            check_run(eng, stats, r)
