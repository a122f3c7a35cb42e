"""How a pull round is scheduled must not change what it computes.

The hub chunks (k_hub_partial) run on the context's side stream beside the
round's main pull kernel, joined before k_hub_final (csrc/pull.hip
launch_expand_w), and k_expand's blocks are launched in the order of
csrc/block_order.h, long in-lists first.  These tests run overlays with many
hubs through every kind of pull round, repeatedly in one context, under churn,
on the flat kernel and in two contexts side by side, and overlays whose
heaviest block is the last, the only one, or none at all -- bit-exact against
the CPU oracle through the comparisons of tests/test_gpu_parity.py::_compare:
counters, Message-Lists, first receipts, digests, coverage, forwards, reports.
A missing fork or join shows as a cycle that differs.  The reference's send
loop and Message-List dedup: Peer.py:402-404, Peer.py:175-216.
"""
import json

import numpy as np
import pytest

import round_trace

pytestmark = pytest.mark.gpu

STAT_KEYS = ("injected", "lost", "new_bits", "receivers", "sends", "active", "crashed",
             "reports", "removals", "dup_reports")


def _cfg(first=True, track_fwd=0, churn=False, p_fail=0.0, churn_seed=0, **kw):
    cfg = dict(track_first=int(first), track_digest=1, track_msg_forwards=int(track_fwd), churn=int(churn),
               p_fail=p_fail, churn_seed=churn_seed, hub_threshold=64, push_ratio=0.0, unfiltered_pct=90,
               flat_max_words=16, arc_mask_permille=0, prefilter_pct=20, compact_rows=0)
    cfg.update(kw)
    return cfg


def _step(eng, stats, reports):
    st = eng.round()
    stats.append(st)
    rep, nrep = eng.reports()
    assert nrep == len(rep)
    reports.extend(map(tuple, rep.tolist()))
    return st


def _cycle(eng, last=0):
    """reset -> run -> finalize; the rounds' stats and the dead-node reports"""
    eng.reset()
    stats, reports = [], []
    for r in range(254):
        if _step(eng, stats, reports)["new_bits"] == 0 and r >= last:
            break
    eng.finalize()
    return stats, reports


def _check(pkg, eng, stats, reports, ref, first=True, fwd=True):
    assert len(stats) == ref["rounds"]
    for a, b in zip(stats, ref["stats"]):
        for k in STAT_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    W = eng.words
    for s in stats:
        assert s["row_bytes"] <= (8 * W + (8 if s["scan"] & 4 else 0)) * s["rows_gathered"], s
    assert np.array_equal(eng.seen(), ref["seen"][:, :W])
    if first:
        assert np.array_equal(eng.first(), ref["first"])
    assert np.array_equal(eng.digest(), ref["digest"])
    assert np.array_equal(eng.coverage(), ref["coverage"])
    if fwd:
        assert np.array_equal(eng.forwards(), ref["forwards"])
    else:
        with pytest.raises(pkg.GossipError):
            eng.forwards()
    assert sorted(reports) == sorted(map(tuple, ref["reports"].tolist()))


N_WIDE = 60_000


@pytest.fixture(scope="module")
def wide(pkg, oracle):
    """60,000 vertices, about 10 % of them hubs at hub_threshold = 64, 4096
    messages: 8 at each of 512 origins, so that round 0's senders are under
    split_max_permille of the vertices and the run starts with a degree-split
    round as C4 does."""
    rp, col = oracle.chung_lu(N_WIDE, 12, 2.4, 43)
    g = pkg.CSR(N_WIDE, rp, col, False)
    assert (np.diff(rp) > 64).sum() > 500
    origin = np.repeat(pkg.overlay.random_origins(g.n, 512, seed=43), 8).astype(np.int32)
    return g, origin


@pytest.fixture(scope="module")
def wide_ref(oracle, wide):
    g, origin = wide
    return oracle.run(g, origin, want_first=True)


def test_hubs_in_every_kind_of_round_repeated(pkg, wide, wide_ref):
    g, origin = wide
    with pkg.GossipEngine(0, **_cfg()) as eng:
        eng.load_graph(g)
        eng.set_messages(origin)
        assert eng.words == 64
        runs = []
        for cycle in range(3):
            stats, reports = _cycle(eng)
            print("cycle", cycle, [(s["scan"], s["aliased"], s["done_nb"]) for s in stats])
            _check(pkg, eng, stats, reports, wide_ref)
            runs.append([{k: s[k] for k in STAT_KEYS + ("scan", "mode", "aliased")} for s in stats])
        assert runs[0] == runs[1] == runs[2]
        st = stats
    nm = g.n * len(origin)
    assert all(s["mode"] == 0 for s in st)
    assert any(s["scan"] & 32 for s in st), "no degree-split round"
    assert any(s["scan"] & 8 for s in st), "no line-mask round"
    # unfiltered, early exit by the dense-frontier rule of round_plan.h (last
    # round's new bits >= n * m / 16), before any alias: no done probe
    assert any((s["scan"] & 3) == 2 and not s["scan"] & 64 and p["new_bits"] * 16 >= nm
               for p, s in zip(st, st[1:])), "no unfiltered early-exit round"
    assert any(s["aliased"] > 0 for s in st), "no aliasing round"
    assert any(s["scan"] & 64 for s in st), "no done-probe round"
    assert any(s["scan"] & 128 for s in st), "no list round"


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_rounds_as_recorded(pkg, wide, name):
    """The round's plan is a pure function (csrc/round_plan.h) since the runs
    of tests/golden/round_plan_trace.json were recorded, with the library of
    the commit before: the same runs (tests/round_trace.py: this overlay plain,
    under churn, at W = 8 with the default push_ratio, with compact records)
    give every round's record again -- mode, scan, every counter, all but the
    timings.  (The work counters too: on this overlay they repeated exactly in
    every recording, the parent's and this tree's.)"""
    g, origin = wide
    assert round_trace.BASE == _cfg() and round_trace.N_WIDE == N_WIDE
    want = next(e for e in json.load(open(round_trace.FIXTURE)) if e["name"] == name)
    got = json.loads(json.dumps(round_trace.record(pkg, g, origin, name)))
    assert sorted(got) == sorted(want)
    for k in want:
        if k != "rounds":
            assert got[k] == want[k], k
    assert len(got["rounds"]) == len(want["rounds"])
    for a, b in zip(got["rounds"], want["rounds"]):
        assert a == b, (a["round"], {k: (a[k], b[k]) for k in b if a[k] != b[k]})


def test_hubs_under_churn(pkg, oracle, wide):
    """k_park before the fork, the alive variants with hubs."""
    g, origin = wide
    ref = oracle.run(g, origin, want_first=True, churn=True, p_fail=0.01, churn_seed=5)
    with pkg.GossipEngine(0, **_cfg(churn=True, p_fail=0.01, churn_seed=5)) as eng:
        eng.load_graph(g)
        eng.set_messages(origin)
        stats, reports = _cycle(eng)
        _check(pkg, eng, stats, reports, ref, fwd=False)
        assert any((s["scan"] & 3) == 2 for s in stats), "no unfiltered pull (k_park) under churn"
        assert sum(s["crashed"] for s in stats) > 0


def test_hubs_with_the_flat_kernel(pkg, oracle):
    """Narrow rows: the hub chunks beside k_expand_flat (W = 4)."""
    rp, col = oracle.chung_lu(20_000, 8, 2.2, 11)
    g = pkg.CSR(20_000, rp, col, False)
    origin = pkg.overlay.random_origins(g.n, 256, seed=11)
    ref = oracle.run(g, origin, want_first=True)
    with pkg.GossipEngine(0, **_cfg(flat_max_words=16)) as eng:
        eng.load_graph(g)
        eng.set_messages(origin)
        assert eng.words == 4
        for _ in range(2):
            stats, reports = _cycle(eng)
            _check(pkg, eng, stats, reports, ref)


def test_two_contexts_take_turns(pkg, oracle):
    """Each context has its own side stream: two on one device, advanced round
    by round in turn, both with hubs."""
    rp, col = oracle.chung_lu(20_000, 8, 2.2, 11)
    g = pkg.CSR(20_000, rp, col, False)
    origins = [pkg.overlay.random_origins(g.n, 4096, seed=s) for s in (21, 22)]
    refs = [oracle.run(g, o, want_first=True) for o in origins]
    engs = [pkg.GossipEngine(0, **_cfg()) for _ in origins]
    try:
        for e, o in zip(engs, origins):
            e.load_graph(g)
            e.set_messages(o)
            e.reset()
        out = [([], []) for _ in engs]
        live = [True, True]
        for r in range(254):
            for k, e in enumerate(engs):
                if live[k] and _step(e, *out[k])["new_bits"] == 0:
                    live[k] = False
            if not any(live):
                break
        for e, (stats, reports), ref in zip(engs, out, refs):
            e.finalize()
            _check(pkg, e, stats, reports, ref)
    finally:
        for e in engs:
            e.close()


def _heavy_last(pkg, oracle):
    """64 * 1000 + 37 vertices; the vertex of highest in-degree, above the
    block order's cut of 1024, has the last id: the last, partial block is the
    first one launched."""
    n = 64 * 1000 + 37
    rp, col = oracle.chung_lu(n, 8, 2.2, 13)
    src, dst = pkg.CSR(n, rp, col, False).arcs()
    extra = np.arange(1500, dtype=np.int64) * 40 + 3   # a floor under the top degree
    src = np.concatenate([src, np.full(extra.size, n - 1, np.int64)])
    dst = np.concatenate([dst, extra])
    g = pkg.CSR.from_arcs(n, src, dst, False)
    top = int(np.argmax(g.in_degree()))
    perm = np.arange(n, dtype=np.int64)
    perm[top], perm[n - 1] = n - 1, top
    src, dst = g.arcs()
    g = pkg.CSR.from_arcs(n, perm[src], perm[dst], False)
    deg = g.in_degree()
    assert deg[n - 1] == deg.max() and deg[n - 1] > 1024
    return g


def _single_block(pkg, oracle):
    rng = np.random.default_rng(5)
    return pkg.CSR.from_edges(40, rng.integers(0, 40, size=(120, 2)))


def _ring(pkg, oracle):
    n = 300   # equal degrees: the block order is the identity
    return pkg.CSR.from_edges(n, [(i, (i + 1) % n) for i in range(n)])


@pytest.mark.parametrize("m", [64, 4096], ids=["W1", "W64"])
@pytest.mark.parametrize("make", [_heavy_last, _single_block, _ring], ids=["heavy-last-block", "one-block", "ring"])
def test_block_order_edge_cases(pkg, oracle, make, m):
    """hub_threshold out of reach: the heavy vertices stay in k_expand
    (flat_max_words = 0: at W = 1 too)."""
    g = make(pkg, oracle)
    first = g.n * m <= 1 << 24
    origin = pkg.overlay.random_origins(g.n, m, seed=m + g.n)
    ref = oracle.run(g, origin, want_first=first)
    with pkg.GossipEngine(0, **_cfg(first=first, hub_threshold=1 << 30, flat_max_words=0)) as eng:
        eng.load_graph(g)
        eng.set_messages(origin)
        assert eng.words == (1 if m == 64 else 64)
        stats, reports = _cycle(eng)
        _check(pkg, eng, stats, reports, ref, first=first)
