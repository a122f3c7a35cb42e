"""Per-peer delay distributions (csrc/delay_dist.hip, gp_track_delay_dist,
GP_DELAY_DIST, gp_read_delay_dist_bins) against the CPU oracle.

delay_dist[v][d] counts the messages v holds whose delay first[v][k] -
inject_round[k], capped at 15, is d: the time column of the reference's arrival
logs (Peer.py:206, Peer.py:286) grouped by the receiving peer and kept per
value, so that medians and tails can be read.  Every case compares the array
and seenpop() exactly with tests/delay_dist_ref.py, which evaluates the formula
of DESIGN.md §2.4 on the oracle's first-receipt matrix alone,
delay_dist_bins() exactly with delay_dist_ref.bins and with latency.dist_bins of
the array read, and checks that every other output of the tracked run equals
the oracle's as before.  No tolerance anywhere.

Shapes are test_gpu_delay.py's, the smallest that reach each path: 4,099
vertices (no multiple of a wave's 64) and 5 (fewer than one wave), every row
width with partial last words, the five direction / scan modes on a table with
several inject rounds (the row pass) and on one with a single inject round (the
pass over the per-vertex counts alone), a window that slides over 210 rounds, a
path long enough to fill the saturated column, hubs committed by k_hub_final,
churn and a crash right after a receipt, aliased Message-Lists and receiver
lists, a directed overlay, message shards, vertex partitions, and the lifecycle.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import delay_dist_ref
import delay_ref
import directed_shapes as ds
import raw_csr
from test_gpu_curve import MODE_IDS, MODES, STAT_KEYS, _alias_ref, _width_ref, check_run, mode_cfg, overlay, run
from test_gpu_delay import WIDTH_MS, WORDS, _churn_uniform_ref, _exp as _delay_exp, check_delay
from test_gpu_fresh import CHURN, _churn_ref, _status

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tracked(pkg, g, origin, inject, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.track_delay_dist()
    eng.reset()
    return eng


def check_dist(pkg, eng, g, want, lo=0, hi=None, ref_bins=True):
    """delay_dist(), seenpop() and delay_dist_bins() against want = (dist [n][16],
    seenpop [n]) of the whole overlay; [lo, hi): the context's owned slice"""
    hi = int(g.n) if hi is None else hi
    dist, sp = (np.asarray(x)[lo:hi] for x in want)
    d, got_sp, t = eng.delay_dist(), eng.seenpop(), eng.delay_dist_bins()
    assert d.dtype == np.uint16 and d.shape == (hi - lo, 16)
    assert t.dtype == np.uint64 and t.shape == (32, 16)
    bad = np.nonzero((d.astype(np.int64) != dist).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], d[bad[:4]], dist[bad[:4]])
    assert np.array_equal(got_sp.astype(np.int64), sp)
    assert np.array_equal(d.astype(np.int64).sum(axis=1), got_sp.astype(np.int64))   # column 0 closes every row
    deg = np.diff(np.asarray(g.row_ptr, np.int64))[lo:hi]
    assert np.array_equal(t, pkg.latency.dist_bins(deg, d))
    if ref_bins:
        assert np.array_equal(t, delay_dist_ref.bins(g, want[0], lo=lo, hi=hi))
    return d, got_sp, t


def final(exp):
    return exp["dist"], exp["seenpop"]


@functools.lru_cache(maxsize=None)
def _exp(n, m, uniform):
    """test_gpu_delay._exp's shape with the distributions' reference"""
    g, origin, inject, ref, _ = _delay_exp(n, m, uniform)
    return g, origin, inject, ref, delay_dist_ref.totals(ref, inject)


# -- sizes, widths, modes -------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", WIDTH_MS)
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_modes_rows(pkg, oracle, n, m, mode):
    """inject = k % 3: the row pass (k_delay_dist<W>), three masks per word"""
    g, origin, inject, ref, exp = _exp(n, m, False)
    if n == 4099 and m >= 100:
        assert (exp["dist"].sum(axis=0)[:7] > 0).all() and int(exp["dist"][:, 0].sum()) == m
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        assert eng.info()[3] == WORDS[m]
        stats = run(eng, inject)
        check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", WIDTH_MS)
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_modes_uniform(pkg, oracle, n, m, mode):
    """every message injected in round 0: the pass over the guard words alone
    (k_delay_dist_uniform)"""
    g, origin, inject, ref, exp = _exp(n, m, True)
    with tracked(pkg, g, origin, None, **mode_cfg(mode)) as eng:
        stats = run(eng, None)
        d, _, _ = check_dist(pkg, eng, g, final(exp))
        # one inject round: column r + 1 is round r's new bits
        cols = d.astype(np.int64).sum(axis=0)
        for r, st in enumerate(stats[:14]):
            assert int(cols[r + 1]) == st["new_bits"]
        check_run(eng, stats, ref)


@pytest.mark.parametrize("m", [100, 4096])
def test_uniform_table_by_rows(pkg, oracle, monkeypatch, m):
    """GP_DELAY_ROWS=1: the row pass on a table with one inject round gives the
    guard-word pass's record"""
    g, origin, _, ref, exp = _exp(4099, m, True)
    with tracked(pkg, g, origin, None) as eng:
        run(eng, None)
        plain = check_dist(pkg, eng, g, final(exp))
    monkeypatch.setenv("GP_DELAY_ROWS", "1")
    with tracked(pkg, g, origin, None) as eng:
        stats = run(eng, None)
        forced = check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)
    for a, b in zip(plain, forced):
        assert np.array_equal(a, b)


def test_uniform_table_keeps_no_frontier_rows(pkg, oracle, monkeypatch):
    """a checkpoint holds the frontier rows a context keeps: tracking a table
    with one inject round adds none, a table with several (or GP_DELAY_ROWS=1)
    adds them -- whichever of the two delay records asks"""
    g, origin, inject, _, _ = _exp(4099, 100, False)

    def blob_bytes(inj, dist, delay=False):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_messages(origin, inj)
            eng.track_delay_dist(dist)
            eng.track_delay(delay)
            eng.reset()
            return eng.checkpoint().size

    rows = g.n * 2 * 8   # [n][W = 2] u64
    assert blob_bytes(None, True) == blob_bytes(None, False)
    assert blob_bytes(inject, True) == blob_bytes(inject, False) + rows
    assert blob_bytes(inject, True, True) == blob_bytes(inject, True)   # (one set of rows for both)
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
        exp = delay_dist_ref.totals(ref, inject)
        with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
            stats = run(eng, inject)
            check_dist(pkg, eng, g, final(exp))
            check_run(eng, stats, ref)


# -- a sliding window -------------------------------------------------------------

def test_inject_rounds_up_to_200(pkg, oracle):
    """inject = 37 k % 201: every plane 0-7 holds messages, the window slides
    over about 210 rounds, and inject rounds older than the window are present
    in most of them"""
    g, origin, _, _ = _width_ref(4099, 100)
    inject = ((37 * np.arange(100)) % 201).astype(np.int32)
    assert all(((inject >> b) & 1).any() for b in range(8))
    ref = oracle.run(g, origin, inject, want_first=True)
    assert ref["rounds"] > 200
    exp = delay_dist_ref.totals(ref, inject)
    assert (exp["dist"].sum(axis=0)[:6] > 0).all()
    with tracked(pkg, g, origin, inject) as eng:
        stats = run(eng, inject)
        check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)


# -- the saturated column ---------------------------------------------------------

def path_csr(pkg, n):
    """the path 0 - 1 - ... - n - 1 as a raw in-CSR"""
    a = np.arange(n - 1, dtype=np.int64)
    rp, col = raw_csr._csr(n, np.concatenate([a, a + 1]), np.concatenate([a + 1, a]))
    return pkg.CSR(n, rp, col, False)


@pytest.mark.parametrize("m", [100, 4096])
@pytest.mark.parametrize("rounds_injected", [1, 2], ids=["uniform", "rows"])
def test_path_fills_the_last_column(pkg, oracle, rounds_injected, m):
    """24 peers in a row, every message injected at peer 0: peer v hears a
    message v rounds after its start, so columns 1 .. 14 hold one peer each and
    column 15 the last 9 hops -- through the guard-word pass (one inject round)
    and through the row pass (two: the remainder that needs no mask)"""
    g = path_csr(pkg, 24)
    origin = np.zeros(m, np.int32)
    inject = None if rounds_injected == 1 else (np.arange(m) % 2).astype(np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    exp = delay_dist_ref.totals(ref, inject)
    want = np.zeros((24, 16), np.int64)
    for v in range(24):
        want[v, min(v, 15)] = m
    assert np.array_equal(exp["dist"], want)
    with tracked(pkg, g, origin, inject) as eng:
        eng.track_delay()
        eng.reset()
        stats = run(eng, inject)
        d, sp, t = check_dist(pkg, eng, g, final(exp))
        assert d.sum(axis=0).tolist() == [m] * 15 + [9 * m] and d.max() == m
        s, mx = eng.delay_sum(), eng.delay_max()
        assert mx.tolist() == list(range(24)) and s.tolist() == [m * v for v in range(24)]
        pkg.latency.dist_check(d, sp, s, mx)                      # <= and >= 15 where saturated
        q, sat = pkg.latency.dist_quantile(d, 0.5, flag=True)
        assert q.tolist() == [min(v, 15) for v in range(24)] and sat.tolist() == [v >= 15 for v in range(24)]
        check_run(eng, stats, ref)


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
        check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)


# -- liveness -------------------------------------------------------------------

@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
@pytest.mark.parametrize("m", [100, 1000])
def test_churn(pkg, oracle, m, uniform, mode):
    g, origin, inject, ref = _churn_ref(m)
    if uniform:
        inject, ref = None, _churn_uniform_ref(m)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0
    exp = delay_dist_ref.totals(ref, inject)
    with tracked(pkg, g, origin, inject, churn=1, p_fail=0.02, churn_seed=5, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
def test_crash_right_after_receipt(pkg, oracle, uniform, mode):
    """20 vertices with a first receipt in round 2 crash in round 2: k_churn
    zeroes their frontier counts before they send; what they received still
    counts as received, in its delay's column"""
    g, origin, inject, plain, _ = _exp(4099, 100, uniform)
    picked = np.nonzero((plain["first"] == 2).any(axis=1))[0][:20]
    assert picked.size == 20
    crashes = [(int(v), 2) for v in picked]
    ref = ds.CachedOracle(oracle).run(g, origin, inject, crashes=crashes, want_first=True)
    assert (ref["first"][picked] == 2).any() and not np.array_equal(ref["forwards"], plain["forwards"])
    exp = delay_dist_ref.totals(ref, inject)
    assert (exp["dist"][picked, 1:3].sum(axis=1) > 0).any()
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject, crashes)
        check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)


# -- aliased Message-Lists and receiver lists -------------------------------------

@functools.lru_cache(maxsize=None)
def _alias_exp(pkg):
    return delay_dist_ref.totals(_alias_ref(pkg), None)


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
        check_dist(pkg, eng, g, final(exp), ref_bins=False)   # (120,000 rows: the numpy twin alone)
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
    exp = delay_dist_ref.totals(ref, inject)
    with tracked(pkg, g, origin, inject, hub_threshold=64) as eng:
        stats = run(eng, inject)
        _, _, t = check_dist(pkg, eng, g, final(exp))
        assert np.array_equal(t, pkg.latency.dist_bins(g.in_degree(), exp["dist"].astype(np.uint16)))
        check_run(eng, stats, ref)


# -- reads between rounds ---------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
@pytest.mark.parametrize("m", [100, 4096])
def test_read_between_rounds(pkg, oracle, m, uniform):
    g, origin, inject, ref, exp = _exp(4099, m, uniform)
    zero = (np.zeros((g.n, 16), np.int64), np.zeros(g.n, np.int64))
    with tracked(pkg, g, origin, inject) as eng:
        check_dist(pkg, eng, g, zero)   # nothing before round 0
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            want = exp["per_round"][r]
            first_read = check_dist(pkg, eng, g, want, ref_bins=r < 3)
            again = check_dist(pkg, eng, g, want, ref_bins=False)   # a read changes nothing
            for a, b in zip(first_read, again):
                assert np.array_equal(a, b)
        check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_stopping_after_two_rounds(pkg, oracle, mode):
    g, origin, inject, ref, exp = _exp(4099, 1000, False)
    cut = delay_dist_ref.totals(ref, inject, rounds=2)
    assert 0 < int(cut["dist"].sum()) < int(exp["dist"].sum())
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = [eng.round(), eng.round()]
        check_dist(pkg, eng, g, final(cut))
        while not (stats[-1]["new_bits"] == 0 and stats[-1]["round"] >= 2):
            stats.append(eng.round())
        check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)


# -- message shards ---------------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
def test_message_shards(pkg, oracle, uniform):
    """two contexts with the word-aligned halves of the 4,096-message table:
    each holds its own messages' receipts (planes and presence set of its own
    table), and the arrays add element by element to the single-context result"""
    g, origin, inject, ref, exp = _exp(4099, 4096, uniform)
    parts, tables = [], []
    for lo, hi in ((0, 2048), (2048, 4096)):
        inj = None if inject is None else inject[lo:hi]
        part = delay_dist_ref.totals({"first": ref["first"][:, lo:hi], "rounds": ref["rounds"]}, inj)
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.track_delay_dist()
            eng.reset()
            run(eng, inj)
            d, _, t = check_dist(pkg, eng, g, final(part))
            parts.append(d)
            tables.append(t)
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
    assert np.array_equal(pkg.latency.dist_combine(parts), exp["dist"])
    assert np.array_equal(pkg.latency.dist_combine(tables), delay_dist_ref.bins(g, exp["dist"]).astype(np.int64))


# -- vertex partition -------------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_partition(pkg, oracle, churn, uniform):
    """Three contexts of a vertex partition on one GPU: each keeps the record
    of its owned vertices; the slices concatenate to the oracle's, the tables
    add up to the whole overlay's."""
    g = pkg.overlay.barabasi_albert(3001, 2, seed=8)
    origin = pkg.overlay.random_origins(g.n, 200, seed=8)
    inject = np.zeros(200, np.int32) if uniform else (np.arange(200) % 4).astype(np.int32)
    kw = dict(churn=True, p_fail=0.02, churn_seed=3) if churn else {}
    cfg = dict(churn=1, p_fail=0.02, churn_seed=3, track_msg_forwards=1) if churn else {}
    ref = oracle.run(g, origin, inject, want_first=True, **kw)
    exp = delay_dist_ref.totals(ref, inject)
    engs = []
    for k in range(3):
        e = pkg.GossipEngine(0, **cfg)
        e.load_graph(g)
        e.set_partition(k, 3)
        e.set_messages(origin, inject)
        e.track_delay_dist()
        e.reset()
        engs.append(e)
    stats = pkg.GossipEngine.run_group(engs)
    assert len(stats) == ref["rounds"]
    for a, b in zip(stats, ref["stats"]):
        for k in STAT_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    slices, tables = [], []
    for e in engs:
        lo, hi = e.partition()
        d, _, t = check_dist(pkg, e, g, final(exp), lo=lo, hi=hi)
        slices.append(d)
        tables.append(t)
    assert np.array_equal(np.concatenate(slices), exp["dist"])
    assert np.array_equal(pkg.latency.dist_combine(tables), delay_dist_ref.bins(g, exp["dist"]).astype(np.int64))
    for e in engs:
        e.close()


def test_partition_over_the_rccl_stand_in(pkg):
    """P = 2 ranks as threads of a child process that loads the engine built
    against the in-process RCCL stand-in (tests/delay_dist_standin_driver.py):
    the owned slices concatenate to the single-rank array"""
    import importlib
    sys.path.insert(0, os.path.dirname(pkg._lib.__file__))
    try:
        path = importlib.import_module("build_lib").STANDIN_LIB
    finally:
        sys.path.pop(0)
    assert os.path.exists(path)
    env = dict(os.environ, GOSSIP_HIP_LIB=path, GP_STANDIN_ASYNC="1")
    env.pop("GP_STANDIN_CORRUPT", None)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "delay_dist_standin_driver.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-6000:]
    assert "delay_dist cases ok: 2" in r.stdout


# -- the identities ---------------------------------------------------------------

@pytest.mark.parametrize("uniform", [False, True], ids=["rows", "uniform"])
def test_identities_with_the_other_records(pkg, oracle, uniform):
    """with track_delay and track_curve on, after every round: the weighted row
    sums and largest columns are delay_sum and delay_max, the column sums are
    the curve's receipts per delay, the table's row sums are delay_bins'
    receipts"""
    g, origin, inject, ref, exp = _exp(4099, 1000, uniform)
    old = delay_ref.totals(ref, inject)
    with tracked(pkg, g, origin, inject) as eng:
        eng.track_delay()
        eng.track_curve()
        eng.reset()
        for r in range(ref["rounds"]):
            eng.round()
            d, sp, s, mx = eng.delay_dist(), eng.seenpop(), eng.delay_sum(), eng.delay_max()
            pkg.latency.dist_check(d, sp, s, mx)
            d = d.astype(np.int64)
            assert not d[:, 15].any()   # (this overlay's largest delay is below 15: every identity is an equality)
            assert np.array_equal((d * np.arange(16)).sum(axis=1), s.astype(np.int64))
            assert np.array_equal(np.where(d > 0, np.arange(16)[None, :], 0).max(axis=1), mx.astype(np.int64))
            hist = pkg.latency.delay_hist(eng.curve(), inject).astype(np.int64)
            hist = np.concatenate([hist, np.zeros(max(0, 16 - hist.size), np.int64)])
            cols = d.sum(axis=0)
            assert np.array_equal(cols[:15], hist[:15]) and int(cols[15]) == int(hist[15:].sum())
            assert np.array_equal(eng.delay_dist_bins().sum(axis=1), eng.delay_bins()[:, 2])
        check_dist(pkg, eng, g, final(exp))
        check_delay(eng, (old["sum"], old["max"], old["seenpop"]))   # the other record is untouched


# -- lifecycle --------------------------------------------------------------------

def test_errors_and_lifecycle(pkg, oracle):
    g, origin, inject, ref, exp = _exp(4099, 100, False)
    lib = pkg._lib
    reads = ("delay_dist", "delay_dist_bins")
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        for name in reads:                                          # off by default
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        eng.track_delay()
        eng.reset()
        for name in reads:                                          # the other delay record does not turn it on
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        eng.track_delay(False)
        eng.track_delay_dist()
        for name in reads:                                          # takes effect at the next reset
            assert _status(pkg, getattr(eng, name)) == lib.GP_ENOTRACK
        eng.reset()
        assert _status(pkg, eng.delay_sum) == lib.GP_ENOTRACK       # ... nor this one the other
        for rows in (g.n - 1, g.n + 1):                             # a wrong byte count: refused, nothing written
            buf = np.full((rows, 16), 77, np.uint16)
            assert eng._lib.gp_read(eng._ctx, lib.DELAY_DIST, buf.ctypes.data, buf.nbytes) == lib.GP_EINVAL
            assert (buf == 77).all()
        buf = np.full((g.n, 8), 77, np.uint16)
        assert eng._lib.gp_read(eng._ctx, lib.DELAY_DIST, buf.ctypes.data, buf.nbytes) == lib.GP_EINVAL
        for bins in (31, 33, 0, 16):                                # a wrong bin count
            tb = np.full((33, 16), 77, np.uint64)
            assert eng._lib.gp_read_delay_dist_bins(eng._ctx, tb.ctypes.data, bins) == lib.GP_EINVAL
            assert (tb == 77).all()
        assert eng._lib.gp_read_delay_dist_bins(eng._ctx, None, 32) == lib.GP_EINVAL   # a null argument
        assert eng._lib.gp_track_delay_dist(None, 1) == lib.GP_EINVAL
        stats = run(eng, inject)
        first_run = check_dist(pkg, eng, g, final(exp))
        check_run(eng, stats, ref)
        eng.reset()                                                 # cleared: a second run starts from zero
        assert not eng.delay_dist().any() and not eng.delay_dist_bins().any()
        run(eng, inject)
        for a, b in zip(check_dist(pkg, eng, g, final(exp)), first_run):
            assert np.array_equal(a, b)                             # ... and is identical
        eng.reset()
        for _ in range(3):
            eng.round()
        check_dist(pkg, eng, g, exp["per_round"][2])
        eng.track_delay_dist(False)                                 # off again: at the next reset
        check_dist(pkg, eng, g, exp["per_round"][2])
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
            assert _status(pkg, other.delay_dist) == lib.GP_ESTATE
            check_run(other, stats + more, ref)                     # the restored run itself is exact
            other.reset()
            run(other, inject)
            check_dist(pkg, other, g, final(exp))
            other.restore(blob0)                                    # a blob of round 0 has counted nothing yet
            run(other, inject)
            check_dist(pkg, other, g, final(exp))


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
            check_dist(pkg, eng, g, final(e))
            check_run(eng, stats, r)
