"""Complete lines of a top in-neighbour: the per-line
done-neighbour rule of the W = 64 early-exit pulls, against the CPU oracle and
against the same run with the rule off.

The rule only drops row loads: a receiver whose first two gather-order
in-neighbours held a 128-B line of their Message-List whole at the start of
the round takes that line of its target and fetches it from nobody.  So every
output and every protocol counter -- the reference's send loop over every link
(Peer.py:402-404) and its Message-List dedup (Peer.py:175-216) -- must stay bit
for bit what the oracle computes, and only the work counters may move, down.

Shape: Chung-Lu 200,000 x mean degree 8, gamma 2.5, 4096 messages (W = 64)
in spread order.
Unless a case says otherwise the rule is forced on (GP_LINE_DONE=1) with a
minimum candidate degree of 16, every round pulls (push_ratio 0), unfiltered
from 1 % senders, and no vertex is a hub (hub_threshold above the maximum
degree), so that the work counters do not depend on wave timing.  The default
gate needs more than 2^19 vertices at W = 64; tests/test_full_size.py runs the
bench configuration there.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DBAR, GAMMA, M = 200_000, 8, 2.5, 4096
STAT_KEYS = ("injected", "lost", "new_bits", "receivers", "sends", "active", "crashed",
             "reports", "removals", "dup_reports")
_cache = {}


def _overlay(pkg, oracle, kind):
    """'one': the Chung-Lu overlay; 'two': a 150,000- and a 50,000-vertex
    Chung-Lu overlay side by side (no arc between them)."""
    if ("g", kind) not in _cache:
        if kind == "one":
            rp, col = oracle.chung_lu(N, DBAR, GAMMA, 5)
            g = pkg.CSR(N, rp, col, False)
        else:
            na, nb = 150_000, 50_000
            rpa, cola = oracle.chung_lu(na, DBAR, GAMMA, 6)
            rpb, colb = oracle.chung_lu(nb, DBAR, GAMMA, 7)
            rp = np.concatenate([rpa, rpa[-1] + rpb[1:]]).astype(np.int64)
            col = np.concatenate([cola, colb + na]).astype(np.int32)
            g = pkg.CSR(na + nb, rp, col, False)
        _cache[("g", kind)] = g
    return _cache[("g", kind)]


def _messages(pkg, g, staggered=False):
    """The message table in spread order, as the bench runs it (by inject
    round, then by the 3-hop spread key): the fast messages share line 0, which
    the big vertices hold whole while most bits are still missing."""
    origin = pkg.overlay.random_origins(g.n, M, seed=5)
    inject = (np.arange(M) % 3).astype(np.int32) if staggered else None
    p = pkg.overlay.spread_order(pkg.overlay.spread_keys(g.row_ptr, g.col, origin, 3), inject)
    return origin[p], (inject[p] if staggered else None)


def _reference(oracle, key, g, origin, inject, **kw):
    """One oracle run per case family, shared and never modified."""
    if ("ref", key) not in _cache:
        ref = oracle.run(g, origin, inject, nthreads=16, **kw)
        for a in ("seen", "digest", "coverage", "forwards"):
            ref[a].setflags(write=False)
        _cache[("ref", key)] = ref
    return _cache[("ref", key)]


def _run(pkg, monkeypatch, g, origin, inject, line_done, min_deg=16, hub_threshold=None, runs=1, **cfg):
    """The engine's run(s) to quiescence with GP_LINE_DONE / GP_LINE_DONE_MIN_DEG
    set as given (None: unset) when the context is created."""
    for name, val in (("GP_LINE_DONE", line_done), ("GP_LINE_DONE_MIN_DEG", min_deg)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    if hub_threshold is None:
        hub_threshold = int(np.diff(g.row_ptr).max()) + 1
    cfg = dict(dict(track_first=0, track_digest=1, push_ratio=0.0, unfiltered_pct=1, hub_threshold=hub_threshold), **cfg)
    out = []
    with pkg.GossipEngine(0, **cfg) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        for _ in range(runs):
            eng.reset()
            stats = eng.run()
            eng.finalize()
            out.append(dict(stats=stats, seen=eng.seen(), digest=eng.digest(), coverage=eng.coverage(),
                            forwards=eng.forwards()))
    return out if runs > 1 else out[0]


def _check_oracle(run, ref):
    assert len(run["stats"]) == ref["rounds"]
    for a, b in zip(run["stats"], ref["stats"]):
        for k in STAT_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    assert np.array_equal(run["seen"], ref["seen"])
    assert np.array_equal(run["digest"], ref["digest"])
    assert np.array_equal(run["coverage"], ref["coverage"])
    assert np.array_equal(run["forwards"], ref["forwards"])


def _work(run):
    return [(s["round"], s["scan"], s["row_bytes"], s["rows_gathered"], s["arcs_scanned"], s["rows_written"],
             s["aliased"], s["done_nb"]) for s in run["stats"]]


def _check_on_off(on, off):
    """Same protocol, same outputs; the rule only drops loads, and drops some.

    row_bytes and rows_gathered never rise, and row_bytes falls in at least
    one round (base case: round 3 541.0 -> 374.2 MB, round 4 241.2 -> 192.1 MB,
    round 5 44.05 -> 43.75 MB).  rows_gathered stays equal at this shape and
    cannot fall: it counts the rows of every batch in which some lane still
    loads, so it only falls where the complete lines cover a receiver's whole
    target, and the oracle's first-receipt matrix has no such receiver here in
    any round, at minimum degree 16 or 1 (a neighbour holding lines 0-2 whole
    holds line 3 too and is a done in-neighbour already).  At C4 size it falls
    (profiles/LEDGER.md, "Complete lines of a top in-neighbour"), and
    test_receivers_covered_whole builds an overlay where it must, and asserts
    it strictly."""
    print("on :", _work(on))
    print("off:", _work(off))
    assert len(on["stats"]) == len(off["stats"])
    fired = False
    for a, b in zip(on["stats"], off["stats"]):
        for k in STAT_KEYS + ("mode", "scan", "done_nb"):
            assert a[k] == b[k], (k, a["round"])
        assert a["rows_written"] + a["aliased"] == b["rows_written"] + b["aliased"], a["round"]
        assert a["row_bytes"] <= b["row_bytes"], a["round"]
        assert a["rows_gathered"] <= b["rows_gathered"], a["round"]
        fired = fired or a["row_bytes"] < b["row_bytes"]
    for k in ("seen", "digest", "coverage", "forwards"):
        assert np.array_equal(on[k], off[k]), k
    assert fired, "no round read fewer row bytes with the rule on"


def _same_work(a, b):
    for x, y in zip(a["stats"], b["stats"]):
        for k in ("scan", "row_bytes", "rows_gathered", "arcs_scanned", "rows_written", "aliased", "done_nb"):
            assert x[k] == y[k], (k, x["round"], x[k], y[k])


@pytest.fixture(scope="module")
def base(pkg, oracle):
    g = _overlay(pkg, oracle, "one")
    origin, inject = _messages(pkg, g)
    return g, origin, inject, _reference(oracle, "one", g, origin, inject)


@pytest.fixture(scope="module")
def base_off(pkg, base):
    """The base case with the rule off (shared by the on / off and gate cases)."""
    g, origin, inject, _ = base
    mp = pytest.MonkeyPatch()
    try:
        return _run(pkg, mp, g, origin, inject, line_done=0)
    finally:
        mp.undo()


def test_on_against_off_to_quiescence(pkg, base, base_off, monkeypatch):
    """Rule on against off with the same settings, both to quiescence: the
    aliasing and done-probe rounds run behind the rule's rounds (candidates
    aliased by then), and both runs equal the oracle."""
    g, origin, inject, ref = base
    on = _run(pkg, monkeypatch, g, origin, inject, line_done=1)
    _check_oracle(on, ref)
    _check_oracle(base_off, ref)
    _check_on_off(on, base_off)
    assert any(s["aliased"] for s in on["stats"]), "no aliasing round ran"
    assert any(s["scan"] & 64 for s in on["stats"]), "no done-probe round ran"
    # both kernels that take the rule dropped loads: the plain unfiltered pull
    # (before any receiver aliases) and the first aliasing round's (quads)
    less = [(a["aliased"] > 0) for a, b in zip(on["stats"], base_off["stats"])
            if a["scan"] == 2 and a["row_bytes"] < b["row_bytes"]]
    assert False in less and True in less, less


def _staged_overlay(pkg):
    """A crafted overlay in which the complete lines of a receiver's two
    in-neighbours cover its whole target while neither is done.  Two mirrored
    chains of big vertices A - A2 - A3 and B - B2 - B3; 64 origins hang off A
    with the messages of lines 0-1, 64 off B with those of lines 2-3, and four
    connectors join A and B.  A holds lines 0-1 whole after round 0, A2 after
    round 1, A3 after round 2, and none of them anything else until the round
    after (B's chain the same with lines 2-3).  5,000 leaves each of A and of B
    take half the table in round 1, which makes round 2 an early-exit round
    with a quarter of the bits held (the plain pull), and the 6,000 leaves of
    {A2, B2}, which complete in round 2, put round 3 over half (the first
    aliasing round, in-degree 2: gather_pairs), where the leaves of {A3, B3}
    complete."""
    n = 20_000
    A, B, A2, B2, A3, B3 = range(6)
    x = np.arange(6, 70)
    y = np.arange(70, 134)
    c = np.arange(134, 138)
    p1 = np.arange(138, 5138)
    p2 = np.arange(5138, 10138)
    v = np.arange(10138, 16138)
    w = np.arange(16138, n)

    def star(hub, leaves):
        return np.stack([np.full(len(leaves), hub), leaves], axis=1)
    edges = np.concatenate([[[A, A2], [A2, A3], [B, B2], [B2, B3]], star(A, x), star(B, y), star(A, c), star(B, c),
                            star(A, p1), star(B, p2), star(A2, v), star(B2, v), star(A3, w), star(B3, w)])
    g = pkg.CSR.from_edges(n, edges)
    k = np.arange(M)
    origin = np.where(k < M // 2, x[k % 64], y[k % 64]).astype(np.int32)
    return g, origin, dict(v=v, w=w)


def test_receivers_covered_whole(pkg, oracle, monkeypatch):
    """Receivers whose whole target is covered by the complete lines of their
    two in-neighbours gather no row and scan no arc: in the plain pull (round
    2: the serial loop skips the scan) and in the first aliasing round (round
    3: gather_pairs ends before its first batch and the receiver commits its
    component row's alias).  rows_gathered falls in both; arcs_scanned falls in
    the plain pull (gather_pairs loads a pair's column ids beside its seen
    rows, before it knows the target, and counts them)."""
    g, origin, sets = _staged_overlay(pkg)
    ref = _reference(oracle, "staged", g, origin, None)
    nm = g.n * M
    held = np.cumsum([s["new_bits"] + s["injected"] for s in ref["stats"]])
    assert ref["stats"][1]["new_bits"] * 16 >= nm and held[1] * 2 < nm <= held[2] * 2   # round 2 plain, round 3 aliasing
    on = _run(pkg, monkeypatch, g, origin, None, line_done=1)
    off = _run(pkg, monkeypatch, g, origin, None, line_done=0)
    _check_oracle(on, ref)
    _check_oracle(off, ref)
    _check_on_off(on, off)
    a2, b2, a3, b3 = on["stats"][2], off["stats"][2], on["stats"][3], off["stats"][3]
    assert a2["scan"] == 2 and a2["aliased"] == 0 and a2["done_nb"] == 0           # the plain pull
    assert a3["scan"] == 2 and a3["aliased"] >= len(sets["w"]) and b3["aliased"] == a3["aliased"]
    # every leaf of {A2, B2} gathered two rows over two arcs with the rule off, none with it on
    assert b2["rows_gathered"] - a2["rows_gathered"] == 2 * len(sets["v"])
    assert b2["arcs_scanned"] - a2["arcs_scanned"] == 2 * len(sets["v"])
    # ... and every leaf of {A3, B3} two rows in the aliasing round
    assert b3["rows_gathered"] - a3["rows_gathered"] == 2 * len(sets["w"])
    assert a3["arcs_scanned"] <= b3["arcs_scanned"]


def test_every_vertex_a_candidate(pkg, base, base_off, monkeypatch):
    """Minimum degree 1: the widest use of the rule."""
    g, origin, inject, ref = base
    on = _run(pkg, monkeypatch, g, origin, inject, line_done=1, min_deg=1)
    _check_oracle(on, ref)
    _check_on_off(on, base_off)


def test_hub_splits_on(pkg, base, monkeypatch):
    """hub_threshold 512: hub receivers are split over waves beside the main
    kernel and stay outside the rule; hub senders are candidates.  Outputs only
    (the hub chunks' work counters depend on wave timing)."""
    g, origin, inject, ref = base
    assert np.diff(g.row_ptr).max() > 512
    _check_oracle(_run(pkg, monkeypatch, g, origin, inject, line_done=1, hub_threshold=512), ref)


def test_two_components(pkg, oracle, monkeypatch):
    """Two components of different size, messages in both: the component
    targets differ, and candidates sit in the small one too."""
    g = _overlay(pkg, oracle, "two")
    origin, inject = _messages(pkg, g)
    assert (origin < 150_000).any() and (origin >= 150_000).any()
    assert (np.diff(g.row_ptr)[150_000:] >= 16).any()
    ref = _reference(oracle, "two", g, origin, inject)
    on = _run(pkg, monkeypatch, g, origin, inject, line_done=1)
    off = _run(pkg, monkeypatch, g, origin, inject, line_done=0)
    _check_oracle(on, ref)
    _check_on_off(on, off)


def test_staggered_injection(pkg, base, oracle, monkeypatch):
    """Inject rounds 0-2 (line 1 mixes messages of rounds 0 and 1, line 2 of
    rounds 1 and 2): no line may count as complete before the messages of its
    component that it lacks exist."""
    g = base[0]
    origin, inject = _messages(pkg, g, staggered=True)
    ref = _reference(oracle, "staggered", g, origin, inject)
    on = _run(pkg, monkeypatch, g, origin, inject, line_done=1)
    off = _run(pkg, monkeypatch, g, origin, inject, line_done=0)
    _check_oracle(on, ref)
    _check_on_off(on, off)


def test_reset_and_second_run(pkg, base, monkeypatch):
    """A second run in the same context reads no byte of the first."""
    g, origin, inject, ref = base
    first, second = _run(pkg, monkeypatch, g, origin, inject, line_done=1, runs=2)
    _check_oracle(first, ref)
    _check_oracle(second, ref)
    _same_work(first, second)


def test_liveness_keeps_the_rule_off(pkg, base, oracle, monkeypatch):
    """With churn the targets are narrowed by the alive sets, which the rule
    does not know: it must stay off whatever GP_LINE_DONE says."""
    g, origin, inject, _ = base
    kw = dict(churn=True, p_fail=0.01, churn_seed=9)
    ref = _reference(oracle, "churn", g, origin, inject, **kw)
    cfg = dict(churn=1, p_fail=0.01, churn_seed=9, track_msg_forwards=1)
    on = _run(pkg, monkeypatch, g, origin, inject, line_done=1, **cfg)
    off = _run(pkg, monkeypatch, g, origin, inject, line_done=0, **cfg)
    _check_oracle(on, ref)
    _check_oracle(off, ref)
    _same_work(on, off)


def test_default_gate_is_off_at_this_size(pkg, base, base_off, monkeypatch):
    """No overrides: 200,000 x 512 B stay inside the Infinity Cache, the rule is off."""
    g, origin, inject, ref = base
    dflt = _run(pkg, monkeypatch, g, origin, inject, line_done=None, min_deg=None)
    _check_oracle(dflt, ref)
    _same_work(dflt, base_off)
