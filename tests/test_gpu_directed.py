"""Directed overlays at sizes that reach the hub, liveness and late-round
paths of the HIP engine, bit-exact against the CPU oracle (which
test_oracle_directed.py pins to the per-peer harness on directed input).

The device code that branches on the direction -- the push and the push half
of a degree-split round walk the out-CSR, k_detect / k_det_big_* cross from a
candidate's in-list into its out-list, components are weak components,
deg_out / deg_live are out-degrees -- and the rules argued for symmetric
overlays (component targets, done in-neighbours, sated vertices, aliased
Message-Lists, complete lines) run here where in- and out-degree differ: on
oriented Chung-Lu overlays (directed_shapes.py: coin, down, up), the reference's
as-run first-3 overlay (Seed.py:127-129, Peer.py:402) at 3000 peers, and a
two-tier overlay whose weak component holds messages that never reach a quarter
of it.  Every case compares what _compare of test_gpu_parity.py compares; where
a case names a path it also asserts from the round stats that the path ran.
"""
import numpy as np
import pytest

import directed_shapes as ds
from test_gpu_parity import ALIAS_MODES, MODE_IDS, MODES, STAT_KEYS, _compare, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def co(oracle):
    """The oracle with its runs cached: the modes of a case share one."""
    return ds.CachedOracle(oracle)


def _mode_kw(mode):
    push_ratio, unfiltered_pct, flat_max_words, arc_mask = mode
    return dict(push_ratio=push_ratio, unfiltered_pct=unfiltered_pct, flat_max_words=flat_max_words,
                arc_mask_permille=arc_mask)


def _total(r, key):
    return sum(s[key] for s in r["stats"])


def _coin(pkg, oracle):
    g = ds.oriented_chung_lu(pkg, oracle, 30_000, 12, 2.1, 17, "coin")
    din, dout = g.in_degree(), g.out_degree()
    assert int(((din + dout > 2048) & (din <= 2048)).sum()) >= 3 and int((dout > 512).sum()) >= 4
    return g


# -- a. the as-run overlay at 3000 peers -------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_first3_at_scale(pkg, co, mode):
    """Three receivers with 2999 / 2998 / 2997 in-links and 0 / 1 / 2 out-links,
    everyone else with in-degree 0: the three crash, and every peer up reports
    a detected one over its out-link (k_det_big_*: more than 2048 links).

    Crashes at rounds 1, 2, 3: the run ends with round 3 (last injection, all
    receivers down), and a crash at round r is detected at round r + 2, so
    only peer 0 is ever reported: 2822 reports, one big candidate.  The same
    with crashes at rounds 0, 1, 1 has all three detected inside the run
    (rounds 2, 3, 3), and only there can the reports exceed 2 * 2048."""
    g = ds.first3(pkg, 3000)
    assert g.in_degree()[:3].min() > 2048 and not g.in_degree()[3:].any()
    origin = pkg.overlay.random_origins(g.n, 300, seed=3)
    inject = (np.arange(300) % 4).astype(np.int32)
    kw = dict(hub_threshold=64, churn=True, p_fail=0.02, churn_seed=3, **_mode_kw(mode))
    late = _compare(pkg, co, g, origin, inject, crashes=[(0, 1), (1, 2), (2, 3)], **kw)
    assert _total(late, "reports") > 2048
    late["eng"].close()
    r = _compare(pkg, co, g, origin, inject, crashes=[(0, 0), (1, 1), (2, 1)], **kw)
    assert _total(r, "reports") > 2 * 2048
    assert {d for d, _, _ in r["ref"]["reports"].tolist()} >= {0, 1, 2}
    if mode[0] == 1e-12:
        assert all(s["mode"] == 1 for s in r["stats"])
    r["eng"].close()


# -- b. candidates that cross DET_BIG through their out-list -----------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_coin_liveness_big_candidates(pkg, co, mode):
    """The six vertices with the most heartbeat links crash at rounds 1-3; at
    least three of them have in-degree <= 2048 < in + out, so k_det_big_* has
    to cross from the in-list into the out-list (j == din[c]) mid-candidate."""
    g = _coin(pkg, co)
    din, dout = g.in_degree(), g.out_degree()
    top = np.argsort(-(din + dout), kind="stable")[:6]
    assert (din[top] + dout[top] > 2048).all() and int((din[top] <= 2048).sum()) >= 3
    origin = pkg.overlay.random_origins(g.n, 256, seed=17)
    inject = (np.arange(256) % 3).astype(np.int32)
    crashes = [(int(h), 1 + i % 3) for i, h in enumerate(top)]
    r = _compare(pkg, co, g, origin, inject, crashes=crashes, hub_threshold=64, churn=True, p_fail=0.02,
                 churn_seed=23, **_mode_kw(mode))
    ref = r["ref"]   # the bounds are the oracle's own
    assert sum(s["removals"] for s in ref["stats"]) >= 6 and _total(r, "removals") >= 6
    assert sum(s["reports"] for s in ref["stats"]) > 6 * 2048 and _total(r, "reports") > 6 * 2048
    r["eng"].close()


# -- c. hubs that only send / only receive -----------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [1000, 4096])
@pytest.mark.parametrize("kind", ["down", "up"])
def test_one_way_hubs(pkg, co, kind, m, mode):
    """down: 14 vertices of out-degree > 512 and in-degree <= 35 (k_push_big
    walks the out-CSR; its senders are no hubs of the in-CSR); up: 151
    receivers above 64 in-arcs split over waves, 11,966 vertices nobody sends
    to.  Without churn and with it."""
    g = ds.oriented_chung_lu(pkg, co, 20_000, 8, 2.2, 11, kind)
    din, dout = g.in_degree(), g.out_degree()
    if kind == "down":
        assert int((dout > 512).sum()) >= 4 and din.max() <= 64
    else:
        assert int((din > 64).sum()) >= 100 and (din == 0).any() and dout.max() <= 64
    origin = pkg.overlay.random_origins(g.n, m, seed=11)
    for kw in ({}, dict(churn=True, p_fail=0.02, churn_seed=11)):
        r = _compare(pkg, co, g, origin, first=(m == 1000), hub_threshold=64, **_mode_kw(mode), **kw)
        if kind == "down" and mode[0] == 1e-12:
            assert all(s["mode"] == 1 for s in r["stats"])
        if kw:
            assert _total(r, "removals") > 0
        r["eng"].close()


# -- d. row widths ------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [1, 64, 65, 300, 1000, 2048, 4096])
def test_directed_widths(pkg, co, m, mode):
    g = ds.oriented_chung_lu(pkg, co, 3000, 8, 2.3, m, "coin")
    assert not np.array_equal(g.in_degree(), g.out_degree())
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 5).astype(np.int32)
    _compare(pkg, co, g, origin, inject, first=True, **_mode_kw(mode))["eng"].close()


# -- e-g, i, j. the two-tier overlay -----------------------------------------

def _two_tier(pkg, oracle, m, schedule="round0", spread_order=False):
    g, A, B = ds.two_tier(pkg, oracle)
    assert 3 * A.size < g.n and A.size > 1000 and B.size > A.size
    origin = ds.two_tier_origins(g, A, B, m, 7)
    mA, mB = ds.two_tier_counts(origin, A, B)
    assert mA > 0 and mB > 0 and mA + mB < m
    inject = None if schedule == "round0" else (np.arange(m) % 3).astype(np.int32)
    if spread_order:
        p = pkg.overlay.spread_order(pkg.overlay.spread_keys(g.row_ptr, g.col, origin, 3), inject)
        origin, inject = origin[p], (None if inject is None else inject[p])
    return g, A, B, origin, inject


def _check_two_tier_end(ref, origin, A, B):
    """Without liveness A's giant ends with exactly its own messages and B's
    with both giants': the weak component's target is out of A's reach."""
    row_a, row_b = ds.two_tier_masks(origin, A, B, ref["seen"].shape[1])
    assert (ref["seen"][A] == row_a).all() and (ref["seen"][B] == row_b).all()
    held = ds.held_before_round(ref)
    assert (held * 2 >= ref["seen"].shape[0] * origin.size).any()


@pytest.mark.parametrize("schedule", ["round0", "spread"])
@pytest.mark.parametrize("m", [4096, 2048])
@pytest.mark.parametrize("alias_mode", list(ALIAS_MODES))
def test_two_tier_late_rounds(pkg, co, alias_mode, m, schedule):
    """Early-exit rounds above half held on an overlay where a quarter of the
    vertices never complete: done in-neighbours, aliased Message-Lists (W = 64)
    and receiver lists that A's giant never leaves."""
    push_ratio, unfiltered_pct, hub = ALIAS_MODES[alias_mode]
    g, A, B, origin, inject = _two_tier(pkg, co, m, schedule)
    r = _compare(pkg, co, g, origin, inject, first=(m == 2048), push_ratio=push_ratio,
                 unfiltered_pct=unfiltered_pct, hub_threshold=hub, arc_mask_permille=0, compact_rows=0)
    _check_two_tier_end(r["ref"], origin, A, B)
    st = r["stats"]
    print([(s["round"], s["mode"], s["scan"], s["aliased"], s["done_nb"]) for s in st])
    if m == 4096:
        assert sum(s["aliased"] for s in st) > 0
        assert any(s["scan"] & 64 for s in st)
        if alias_mode == "pull":
            assert any(s["scan"] & 128 for s in st)
        for s in st:   # A never completes
            assert s["aliased"] <= B.size, s
    elif push_ratio == 0.0:   # W = 32 above flat_max_words: done in-neighbours in every pull above half held
        assert sum(s["done_nb"] for s in st) > 0
    r["eng"].close()


@pytest.mark.parametrize("m,flat_max_words", [(1000, 16), (512, 0)])
def test_two_tier_narrow_rows(pkg, co, m, flat_max_words):
    """W = 16 on the flat kernel throughout: the thin-round condition (under
    n*m/16 bits missing) cannot hold while A's giant lacks B's messages -- 19 %
    of the bits, asserted in test_oracle_directed.py -- so no done-neighbour
    round exists for it and done_nb is not asserted; W = 8 above
    flat_max_words takes the per-receiver kernel's serial loop."""
    g, A, B, origin, inject = _two_tier(pkg, co, m)
    r = _compare(pkg, co, g, origin, inject, push_ratio=0.0, flat_max_words=flat_max_words)
    _check_two_tier_end(r["ref"], origin, A, B)
    print([(s["round"], s["scan"], s["done_nb"]) for s in r["stats"]])
    if flat_max_words == 0:
        assert sum(s["done_nb"] for s in r["stats"]) > 0
    for s in r["stats"]:
        assert s["done_nb"] == 0 or (s["mode"] == 0 and s["done_nb"] <= s["vertices_visited"])
    r["eng"].close()


def test_two_tier_line_rule(pkg, co, monkeypatch):
    """The complete-line rule forced on against off: a top
    in-neighbour in A's giant holds lines whole that are not its receiver's
    whole target.  Both runs equal the oracle; the rule only drops loads."""
    g, A, B, origin, inject = _two_tier(pkg, co, 4096, spread_order=True)
    kw = dict(first=False, push_ratio=0.0, unfiltered_pct=1, hub_threshold=int(g.in_degree().max()) + 1,
              arc_mask_permille=0, compact_rows=0)
    monkeypatch.setenv("GP_LINE_DONE_MIN_DEG", "16")
    monkeypatch.setenv("GP_LINE_DONE", "1")
    on = _compare(pkg, co, g, origin, inject, **kw)
    on["eng"].close()
    monkeypatch.setenv("GP_LINE_DONE", "0")
    off = _compare(pkg, co, g, origin, inject, **kw)
    off["eng"].close()
    _check_two_tier_end(on["ref"], origin, A, B)
    print([(a["round"], a["scan"], a["row_bytes"], b["row_bytes"], a["rows_gathered"], b["rows_gathered"])
           for a, b in zip(on["stats"], off["stats"])])
    for a, b in zip(on["stats"], off["stats"]):
        assert a["row_bytes"] <= b["row_bytes"], a["round"]
        assert a["rows_gathered"] <= b["rows_gathered"], a["round"]


@pytest.mark.parametrize("push_ratio", [0.0, 10.0], ids=["pull", "adaptive"])
@pytest.mark.parametrize("track_fwd", [0, 1])
def test_two_tier_under_churn(pkg, co, push_ratio, track_fwd):
    """Sated vertices and receiver lists under liveness: A's giant can never
    hold the alive messages of B's, so it is never sated and stays listed."""
    g, A, B, origin, inject = _two_tier(pkg, co, 4096)
    r = _compare(pkg, co, g, origin, inject, first=False, push_ratio=push_ratio, compact_rows=0,
                 arc_mask_permille=0, track_fwd=track_fwd, churn=True, p_fail=0.01, churn_seed=9)
    print([(s["round"], s["mode"], s["scan"]) for s in r["stats"]])
    assert any(s["scan"] & 128 for s in r["stats"])
    assert _total(r, "removals") > 0
    r["eng"].close()


def test_two_tier_parked_rows(pkg, co):
    g, A, B, origin, inject = _two_tier(pkg, co, 4096)
    r = _compare(pkg, co, g, origin, inject, first=False, push_ratio=0.0, unfiltered_pct=1, compact_rows=0,
                 arc_mask_permille=0, churn=True, p_fail=0.01, churn_seed=9)
    scans = [s["scan"] for s in r["stats"]]
    assert sum(1 for x in scans if x & 3 == 2) >= 3, scans
    r["eng"].close()


# -- h. sparse-round paths on coin -------------------------------------------

SPARSE = {}
for _sd in (8, 128):
    for _m, _f in ((512, 0), (512, 16), (2048, 16)):
        SPARSE[f"split{_sd}-m{_m}-flat{_f}"] = dict(
            m=_m, bit=(32,), inject=2, first=False, hub_threshold=64, push_ratio=1000.0, unfiltered_pct=90,
            flat_max_words=_f, arc_mask_permille=0, prefilter_pct=20, compact_rows=0, split_deg=_sd,
            split_max_permille=1000)
SPARSE["line-masks"] = dict(m=4096, bit=(8, 16), inject=0, first=False, hub_threshold=64, push_ratio=0.0,
                            unfiltered_pct=90, flat_max_words=16, arc_mask_permille=0, prefilter_pct=0,
                            compact_rows=0)
for _p in (0, 20):
    SPARSE[f"records-prefilter{_p}"] = dict(m=4096, bit=(4,), inject=0, first=bool(_p), hub_threshold=1 << 30,
                                            push_ratio=0.0, prefilter_pct=_p, arc_mask_permille=0, compact_rows=1)
SPARSE["summary"] = dict(m=256, bit=(), inject=6, first=True, push_ratio=0.0, flat_max_words=0, arc_mask_permille=0,
                         prefilter_pct=20, compact_rows=0, summary_min_n=1)


@pytest.mark.parametrize("path", list(SPARSE))
def test_directed_sparse_round_paths(pkg, co, path):
    """Degree-split rounds (scan bit 32: senders filtered by in-degree through
    rp_in / prehi, their arcs pushed along the out-CSR -- the one place where
    both degrees of a vertex matter at once), line masks (8: read, 16: from
    the commits), compact records (4) and summary probes on coin 30,000, where
    4,527 vertices have no in-arc and 4,530 no out-arc."""
    kw = dict(SPARSE[path])
    m, bits, k = kw.pop("m"), kw.pop("bit"), kw.pop("inject")
    g = _coin(pkg, co)
    assert kw["hub_threshold"] > g.in_degree().max() if path.startswith("records") else True
    origin = pkg.overlay.random_origins(g.n, m, seed=17)
    inject = (np.arange(m) % k).astype(np.int32) if k else None
    r = _compare(pkg, co, g, origin, inject, **kw)
    scans = [s["scan"] for s in r["stats"]]
    print(path, [(s["round"], s["mode"], s["scan"], s["active"]) for s in r["stats"]])
    for b in bits:
        assert any(x & b for x in scans), (b, scans)
    if path.startswith("split"):
        assert all((x & 3) == 3 for x in scans if x & 32), scans
    if path == "summary":   # the summary path runs in filtered pull rounds with <= n/256 senders
        assert any(s["mode"] == 0 and s["scan"] != 2 and s["active"] * 256 <= g.n for s in r["stats"])
    r["eng"].close()


# -- i. checkpoints and message shards ---------------------------------------

def test_directed_checkpoint(pkg, co, tmp_path):
    """Two-tier under churn: saved after round 3, loaded into a fresh context;
    both contexts run on to quiescence and equal the oracle's uninterrupted run."""
    stop, m = 3, 4096
    g, A, B, origin, inject = _two_tier(pkg, co, m)
    kw = dict(churn=True, p_fail=0.01, churn_seed=13)
    cfg = dict(track_first=0, track_digest=1, track_msg_forwards=1, churn=1, p_fail=0.01, churn_seed=13)
    ref = co.run(g, origin, inject, want_first=False, **kw)
    assert ref["rounds"] > stop + 2

    def tail(eng):
        stats, reports = [], []
        while True:
            st = eng.round()
            stats.append(st)
            reports.extend(map(tuple, eng.reports()[0].tolist()))
            if st["new_bits"] == 0:
                return stats, reports

    def check(eng, stats, reports):
        assert len(stats) == ref["rounds"] - stop
        for a, b in zip(stats, ref["stats"][stop:]):
            for k in STAT_KEYS:
                assert a[k] == b[k], (k, a["round"], a[k], b[k])
        eng.finalize()
        assert np.array_equal(eng.seen(), ref["seen"][:, :eng.words])
        assert np.array_equal(eng.digest(), ref["digest"])
        assert np.array_equal(eng.coverage(), ref["coverage"])
        assert np.array_equal(eng.forwards(), ref["forwards"])
        assert sorted(reports) == sorted(tuple(x) for x in ref["reports"].tolist() if x[2] >= stop)

    with _engine(pkg, g, origin, inject, **cfg) as a:
        for _ in range(stop):
            a.round()
        path = tmp_path / "ck.npy"
        a.save_checkpoint(path)
        with _engine(pkg, g, origin, inject, **cfg) as b:
            b.load_checkpoint(path)
            check(b, *tail(b))
        check(a, *tail(a))


def test_directed_message_shards(pkg, co):
    """Two message shards on coin: digests XOR to the whole run's, coverage /
    forwards / first columns concatenate, and the whole run is the oracle's."""
    g = _coin(pkg, co)
    m = 1024
    origin = pkg.overlay.random_origins(g.n, m, seed=13)
    inject = (np.arange(m) % 3).astype(np.int32)

    def run(lo, hi):
        with pkg.GossipEngine(0, track_first=1, track_digest=1, hub_threshold=64) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.reset()
            stats = eng.run()
            eng.finalize()
            return stats, eng.first(), eng.digest(), eng.coverage(), eng.forwards()

    whole = run(0, m)
    parts = [run(*pkg.dist.message_shard(m, 2, r)) for r in range(2)]
    ref = co.run(g, origin, inject, want_first=True)
    assert len(whole[0]) == ref["rounds"]
    for i, s in enumerate(whole[0]):
        for k in STAT_KEYS:
            assert s[k] == ref["stats"][i][k], (k, i)
        for k in ("new_bits", "sends", "injected"):
            assert s[k] == sum(p[0][i][k] if i < len(p[0]) else 0 for p in parts), (k, i)
    assert np.array_equal(whole[1], ref["first"]) and np.array_equal(whole[2], ref["digest"])
    assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1), whole[1])
    assert np.array_equal(parts[0][2] ^ parts[1][2], whole[2])
    assert np.array_equal(np.concatenate([p[3] for p in parts]), whole[3])
    assert np.array_equal(np.concatenate([p[4] for p in parts]), whole[4])
    assert np.array_equal(whole[3], ref["coverage"]) and np.array_equal(whole[4], ref["forwards"])


# -- j. small ones -------------------------------------------------------------

def test_partition_refuses_directed_overlay(pkg, co):
    g = ds.oriented_chung_lu(pkg, co, 3000, 8, 2.3, 5, "coin")
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        with pytest.raises(pkg.GossipError, match="undirected"):
            eng.set_partition(0, 2)


@pytest.mark.parametrize("hops", [1, 2, 3])
def test_spread_keys_match_host_directed(pkg, co, hops):
    """gp_spread_keys reads the in-CSR, as overlay.spread_keys does: hubs by
    links, vertices without in-arcs, repeated origins."""
    g = _coin(pkg, co)
    din, dout = g.in_degree(), g.out_degree()
    origin = pkg.overlay.random_origins(g.n, 3000, seed=44).copy()
    origin[:5] = np.argsort(-(din + dout), kind="stable")[:5]
    origin[5] = np.nonzero(din == 0)[0][0]
    origin[6] = origin[7]
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        assert np.array_equal(eng.spread_keys(origin, hops), pkg.overlay.spread_keys(g.row_ptr, g.col, origin, hops))


def test_two_tier_reset_and_second_run(pkg, co):
    """A second and third run on one context (aliases, done bitmap, receiver
    lists of the first still in memory) repeat the first."""
    g, A, B, origin, inject = _two_tier(pkg, co, 4096, "spread")
    r = _compare(pkg, co, g, origin, inject, first=False, push_ratio=0.0, unfiltered_pct=0,
                 hub_threshold=1 << 30, arc_mask_permille=0, compact_rows=0)
    eng, ref = r["eng"], r["ref"]
    assert sum(s["aliased"] for s in r["stats"]) > 0
    for _ in range(2):
        eng.reset()
        stats = eng.run()
        assert [s["new_bits"] for s in stats] == [s["new_bits"] for s in ref["stats"]]
        assert [s["aliased"] for s in stats] == [s["aliased"] for s in r["stats"]]
        assert np.array_equal(eng.digest(), ref["digest"])
        assert np.array_equal(eng.seen(), ref["seen"])
    eng.close()


# -- the out-CSR argument of gp_load_graph ------------------------------------

def _out_csr(oracle, g, shuffle_seed=None):
    orp, ocol = oracle.transpose(g.n, g.row_ptr, g.col)
    if shuffle_seed is not None:   # each out-row's entries in random order
        row = np.repeat(np.arange(g.n), np.diff(orp))
        ocol = ocol[np.lexsort((np.random.default_rng(shuffle_seed).random(ocol.size), row))]
    return orp.copy(), np.ascontiguousarray(ocol)


class _PkgWithOutCsr:
    """pkg whose engines load every overlay with the given out-CSR."""

    def __init__(self, pkg, out_csr):
        self._pkg = pkg

        class Engine(pkg.GossipEngine):
            def load_graph(self, csr):
                super().load_graph(csr, out_csr=out_csr)
        self.GossipEngine = Engine

    def __getattr__(self, name):
        return getattr(self._pkg, name)


@pytest.mark.parametrize("mode", [MODES[3], MODES[4]], ids=["push", "adaptive"])
def test_explicit_out_csr(pkg, co, mode):
    """An out-CSR handed to gp_load_graph (the oracle's transpose, each row
    shuffled) runs as the engine's own transpose does and as the oracle."""
    g = ds.oriented_chung_lu(pkg, co, 3000, 8, 2.3, 5, "coin")
    orp, ocol = _out_csr(co, g, shuffle_seed=5)
    plain = _out_csr(co, g)[1]
    assert not np.array_equal(ocol, plain) and np.array_equal(np.sort(ocol), np.sort(plain))
    origin = pkg.overlay.random_origins(g.n, 300, seed=5)
    inject = (np.arange(300) % 4).astype(np.int32)
    din, dout = g.in_degree(), g.out_degree()
    crashes = [(int(np.argmax(din + dout)), 1)]
    kw = dict(crashes=crashes, hub_threshold=64, churn=True, p_fail=0.02, churn_seed=5, **_mode_kw(mode))
    given = _compare(_PkgWithOutCsr(pkg, (orp, ocol)), co, g, origin, inject, **kw)
    own = _compare(pkg, co, g, origin, inject, **kw)
    assert _total(given, "reports") > 0 and _total(given, "sends") > 0
    if mode[0] == 1e-12:
        assert all(s["mode"] == 1 for s in given["stats"])
    for a, b in zip(given["stats"], own["stats"]):
        for k in STAT_KEYS + ("mode", "scan"):
            assert a[k] == b[k], (k, a["round"])
    assert np.array_equal(given["eng"].seen(), own["eng"].seen())
    assert np.array_equal(given["eng"].deg_live(), own["eng"].deg_live())
    given["eng"].close()
    own["eng"].close()


@pytest.mark.parametrize("fault", ["non-monotone", "id-out-of-range", "negative-id", "wrong-degrees", "bad-ends"])
def test_bad_out_csr_refused(pkg, co, fault):
    """gp_load_graph validates a given out-CSR before anything is uploaded."""
    g = ds.oriented_chung_lu(pkg, co, 3000, 8, 2.3, 5, "coin")
    orp, ocol = _out_csr(co, g)
    i = 1 + int(np.nonzero(np.diff(orp)[1:-1] > 0)[0][0])   # 1 <= i < n - 1, out-degree > 0
    if fault == "non-monotone":
        orp[i] = orp[i + 1] + 1
        assert orp[i] <= orp[-1]
    elif fault == "id-out-of-range":
        ocol[ocol.size // 2] = g.n
    elif fault == "negative-id":
        ocol[0] = -1
    elif fault == "wrong-degrees":   # one arc moved from vertex i to vertex i - 1: still monotone, ids untouched
        orp[i] += 1
        assert (np.diff(orp) >= 0).all()
    else:
        orp[-1] -= 1
    with pkg.GossipEngine(0) as eng:
        with pytest.raises(pkg.GossipError):
            eng.load_graph(g, out_csr=(orp, ocol))
