"""Per-peer traffic record (csrc/load.hip, gp_track_load, GP_LOAD_SENT /
GP_LOAD_RECV / GP_SEENPOP) against the CPU oracle.

sent[u] is the gossip lines peer u put on the wire and recv[v] the lines that
arrived at v, duplicates included: the totals of what each reference peer logs
per arrival (Peer.py:206, Peer.py:286) and sends per link (Peer.py:402-404).
Every case compares load_sent() / load_recv() exactly with tests/load_ref.py,
which reconstructs them from the oracle's outputs alone, and checks that every
other output of the tracked run equals the oracle's as before.

Each shape runs lazy (no vertex ever down: nothing per round, one pass at read
time) and eager (GP_LOAD_EAGER=1: the per-round pass from round 0).  Shapes are
the smallest that reach each path: 4,099 vertices (no multiple of a wave's 64
receivers) and 5 (fewer than one wave), every row width, the five direction /
scan modes, hubs split over items and long rows walked by the main kernel,
churn and explicit crashes, a lazy run turned eager by gp_crash, directed
overlays, aliased Message-Lists, message shards, and the lifecycle.
"""
import functools

import numpy as np
import pytest

import directed_shapes as ds
import load_ref
from test_gpu_curve import MODE_IDS, MODES, STAT_KEYS, _alias_ref, _width_ref, check_run, mode_cfg, overlay, run

pytestmark = pytest.mark.gpu

KINDS = ["lazy", "eager"]


def set_kind(monkeypatch, kind):
    """before the engine is created: GP_LOAD_EAGER is read at gp_create"""
    if kind == "eager":
        monkeypatch.setenv("GP_LOAD_EAGER", "1")
    else:
        monkeypatch.delenv("GP_LOAD_EAGER", raising=False)


def tracked(pkg, g, origin, inject, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.track_load()
    eng.reset()
    return eng


def check_load(eng, exp):
    sent, recv = eng.load_sent(), eng.load_recv()
    assert sent.dtype == recv.dtype == np.uint64 and sent.shape == recv.shape == (eng.n,)
    assert np.array_equal(sent.astype(np.int64), exp["sent"]), np.nonzero(sent.astype(np.int64) != exp["sent"])[0][:8]
    assert np.array_equal(recv.astype(np.int64), exp["recv"]), np.nonzero(recv.astype(np.int64) != exp["recv"])[0][:8]


_EXP = {}


def expected(key, g, ref, **kw):
    """load_ref.totals, once per shape"""
    if key not in _EXP:
        _EXP[key] = load_ref.totals(g, ref, **kw)
    return _EXP[key]


# -- sizes, widths, modes -----------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [1, 100, 1000, 4096])
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_modes(pkg, oracle, monkeypatch, n, m, mode, kind):
    g, origin, inject, ref = _width_ref(n, m)
    exp = expected(("width", n, m), g, ref)
    assert int(exp["sent"].sum()) == sum(s["sends"] for s in ref["stats"]) == int(exp["recv"].sum())
    set_kind(monkeypatch, kind)
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_load(eng, exp)
        check_load(eng, exp)   # a read changes nothing
        assert np.array_equal(eng.seenpop(), (ref["first"] != 255).sum(axis=1))
        check_run(eng, stats, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_read_between_rounds(pkg, oracle, monkeypatch, kind):
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = expected(("width", 4099, 100), g, ref)
    set_kind(monkeypatch, kind)
    with tracked(pkg, g, origin, inject) as eng:
        assert not eng.load_sent().any() and not eng.load_recv().any()
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            s, v = exp["per_round"][r]
            check_load(eng, {"sent": s, "recv": v})
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


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hub_threshold", [64, 1 << 30], ids=["split", "whole"])
def test_hubs(pkg, oracle, monkeypatch, hub_threshold, kind):
    """hub_threshold=64: k_load_hub walks the items of every vertex above 64
    arcs; 1 << 30: nothing is split and the main kernel walks the long rows."""
    g, origin, ref = _hub_ref()
    assert np.diff(g.row_ptr).max() > 1000
    exp = expected("hub", g, ref)
    set_kind(monkeypatch, kind)
    with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
        stats = run(eng, None)
        check_load(eng, exp)
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
    tot = {k: sum(s[k] for s in ref["stats"]) for k in ("crashed", "removals", "lost", "sends")}
    assert tot["crashed"] > 0 and tot["removals"] > 0 and tot["lost"] > 0
    exp = expected(("churn", m), g, ref, **CHURN)
    assert int(exp["recv"].sum()) < int(exp["sent"].sum()) == tot["sends"]
    set_kind(monkeypatch, "lazy")   # (churn: eager by necessity)
    with tracked(pkg, g, origin, inject, churn=1, p_fail=0.02, churn_seed=5, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_load(eng, exp)
        check_run(eng, stats, ref)
        # duplicates: the messages lost at a down origin are left out of own
        lost = ref["first"][origin, np.arange(m)] == 255
        own = np.bincount(origin[~lost], minlength=g.n)
        dup = pkg.load.duplicates(eng.load_recv(), eng.seenpop(), own)
        assert int(dup.sum()) == int(exp["recv"].sum()) - sum(s["new_bits"] for s in ref["stats"])


def _crash_shapes(ref, g):
    got2 = np.nonzero((ref["first"] == 2).any(axis=1))[0][:20]
    assert got2.size == 20
    hub = int(np.argmax(np.diff(g.row_ptr)))
    return {"after-receipt": [(int(v), 2) for v in got2], "top-hub": [(hub, 2)]}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("which", ["after-receipt", "top-hub"])
def test_explicit_crashes(pkg, oracle, monkeypatch, which, mode, kind):
    """A crash in the round right after a receipt drops that frontier (k_churn
    zeroes its count before the pass reads it); a crash of the top hub takes
    the busiest receiver and sender out.  Eager from round 0, or lazy until
    the crash of round 2."""
    g, origin, inject, plain = _width_ref(4099, 100)
    crashes = _crash_shapes(plain, g)[which]
    ref = ds.CachedOracle(oracle).run(g, origin, inject, crashes=crashes, want_first=True)
    exp = expected(("crash", which), g, ref, crashes=crashes)
    assert int(exp["recv"].sum()) < int(exp["sent"].sum())
    if which == "after-receipt":
        assert (ref["first"][[v for v, _ in crashes]] == 2).any()
    set_kind(monkeypatch, kind)
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject, crashes)
        check_load(eng, exp)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
def test_lazy_turns_eager_at_gp_crash(pkg, oracle, monkeypatch, mode):
    """No churn; the run starts lazy and gp_crash comes before round 3: the
    rounds so far are booked from the state before the crash is applied, the
    later ones per round."""
    g, origin, inject, plain = _width_ref(4099, 100)
    got3 = np.nonzero((plain["first"] == 3).any(axis=1))[0][:20]
    hub = int(np.argmax(np.diff(g.row_ptr)))
    crashes = [(int(v), 3) for v in got3] + [(hub, 3)]
    ref = ds.CachedOracle(oracle).run(g, origin, inject, crashes=crashes, want_first=True)
    exp = expected("lazy-eager", g, ref, crashes=crashes)
    assert ref["rounds"] > 4 and int(exp["recv"].sum()) < int(exp["sent"].sum())
    set_kind(monkeypatch, "lazy")
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject, crashes)
        check_load(eng, exp)
        check_run(eng, stats, ref)
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:   # and read on either side of the switch
        stats = [eng.round() for _ in range(3)]
        check_load(eng, dict(zip(("sent", "recv"), exp["per_round"][2])))
        eng.crash([v for v, _ in crashes])
        check_load(eng, dict(zip(("sent", "recv"), exp["per_round"][2])))
        stats.append(eng.round())
        check_load(eng, dict(zip(("sent", "recv"), exp["per_round"][3])))


# -- directed -----------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("crash", [False, True], ids=["plain", "crash"])
@pytest.mark.parametrize("shape", ["down", "up", "first3"])
def test_directed(pkg, oracle, monkeypatch, shape, crash, kind):
    """in-degree != out-degree: sent uses out-links, recv in-links"""
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
    set_kind(monkeypatch, kind)
    with tracked(pkg, g, origin, None) as eng:
        stats = run(eng, None, crashes)
        check_load(eng, exp)
        check_run(eng, stats, ref)


# -- aliased Message-Lists and receiver lists ----------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_aliases_and_receiver_lists(pkg, oracle, monkeypatch, kind):
    """The shape of test_aliased_message_lists: complete receivers alias their
    component row; the lazy read takes their seenpop."""
    g = overlay(pkg, 120_000, 12, 2.4, 41)
    origin = pkg.overlay.random_origins(g.n, 4096, seed=41)
    ref = _alias_ref(pkg)
    exp = expected("alias", g, ref)
    set_kind(monkeypatch, kind)
    with tracked(pkg, g, origin, None, push_ratio=0.0, unfiltered_pct=0, hub_threshold=1 << 30,
                 arc_mask_permille=0, compact_rows=0) as eng:
        stats = run(eng, None)
        assert sum(s["aliased"] for s in stats) > 0
        assert any(s["scan"] & 128 for s in stats)
        check_load(eng, exp)
        assert np.array_equal(eng.seenpop(), np.unpackbits(ref["seen"].view(np.uint8), axis=1).sum(axis=1))
        check_run(eng, stats, ref)


# -- message shards -----------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_message_shards_add_up(pkg, oracle, monkeypatch, kind):
    g, origin, inject, ref = _width_ref(4099, 4096)
    exp = expected(("width", 4099, 4096), g, ref)
    set_kind(monkeypatch, kind)
    sent = np.zeros(g.n, np.uint64)
    recv = np.zeros(g.n, np.uint64)
    digest = np.zeros(g.n, np.uint64)
    sums = {k: np.zeros(ref["rounds"], np.int64) for k in ("injected", "new_bits", "sends")}
    for lo, hi in ((0, 1024), (1024, 4096)):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.track_load()
            eng.reset()
            stats = run(eng, inject[lo:hi])
            sent += eng.load_sent()
            recv += eng.load_recv()
            assert np.array_equal(eng.seenpop(), (ref["first"][:, lo:hi] != 255).sum(axis=1))
            # the shard's other outputs are the whole run's, cut at its block
            assert len(stats) <= ref["rounds"]
            for k in sums:
                sums[k][:len(stats)] += [s[k] for s in stats]
            eng.finalize()
            assert np.array_equal(eng.seen()[:, :(hi - lo) // 64], ref["seen"][:, lo // 64:hi // 64])
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
            digest ^= eng.digest()
    assert np.array_equal(sent.astype(np.int64), exp["sent"])
    assert np.array_equal(recv.astype(np.int64), exp["recv"])
    assert np.array_equal(digest, ref["digest"])
    for k in sums:
        assert sums[k].tolist() == [s[k] for s in ref["stats"]], k


# -- lifecycle ----------------------------------------------------------------

def _status(pkg, fn):
    with pytest.raises(pkg.GossipError) as e:
        fn()
    return e.value.status


def test_errors_and_lifecycle(pkg, oracle, monkeypatch):
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = expected(("width", 4099, 100), g, ref)
    lib = pkg._lib
    set_kind(monkeypatch, "lazy")
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        assert _status(pkg, eng.load_sent) == lib.GP_ENOTRACK      # not tracked
        assert eng.seenpop().shape == (g.n,)                        # readable without tracking
        eng.track_load()
        assert _status(pkg, eng.load_recv) == lib.GP_ENOTRACK      # takes effect at the next reset
        eng.reset()
        buf = np.zeros(g.n - 1, np.uint64)                          # a short buffer
        assert eng._lib.gp_read(eng._ctx, lib.LOAD_SENT, buf.ctypes.data, buf.nbytes) == lib.GP_EINVAL
        stats = run(eng, inject)
        check_load(eng, exp)
        check_run(eng, stats, ref)
        eng.reset()                                                 # a second run starts from zero
        assert not eng.load_sent().any() and not eng.load_recv().any()
        stats = [eng.round() for _ in range(3)]
        blob3 = eng.checkpoint()
        # a lazy run restored past round 0, in a fresh context: a function of the restored state
        with tracked(pkg, g, origin, inject) as other:
            other.restore(blob3)
            check_load(other, dict(zip(("sent", "recv"), exp["per_round"][2])))
            more = run(other, inject)
            check_load(other, exp)
            check_run(other, stats + more, ref)
        eng.track_load(False)                                       # off again: at the next reset
        check_load(eng, dict(zip(("sent", "recv"), exp["per_round"][2])))
        eng.reset()
        assert _status(pkg, eng.load_sent) == lib.GP_ENOTRACK
        assert _status(pkg, eng.load_recv) == lib.GP_ENOTRACK
    # an eager run restored past round 0: its totals are not in the blob
    set_kind(monkeypatch, "eager")
    with tracked(pkg, g, origin, inject) as eng:
        blob0 = eng.checkpoint()
        stats = [eng.round() for _ in range(3)]
        blob3 = eng.checkpoint()
        with tracked(pkg, g, origin, inject) as other:
            other.restore(blob3)
            assert _status(pkg, other.load_sent) == lib.GP_ESTATE
            more = run(other, inject)
            assert _status(pkg, other.load_recv) == lib.GP_ESTATE
            check_run(other, stats + more, ref)                     # the restored run itself is exact
            other.reset()
            run(other, inject)
            check_load(other, exp)
            other.restore(blob0)                                    # a blob of round 0 keeps everything
            run(other, inject)
            check_load(other, exp)


def test_partitioned_context_keeps_no_loads(pkg, oracle):
    g, origin, inject, _ = _width_ref(4099, 100)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.track_load()
        eng.reset()
        assert _status(pkg, eng.load_sent) == pkg._lib.GP_ENOTRACK
        assert _status(pkg, eng.load_recv) == pkg._lib.GP_ENOTRACK
        assert eng.seenpop().shape == (eng.nloc(),)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_tracking_changes_no_counter(pkg, oracle, monkeypatch, churn, kind):
    """a tracked and an untracked run of one case: identical gp_round_stats
    counters, the work counters included (timings aside)"""
    g, origin, inject, _ = _churn_ref(100) if churn else _width_ref(4099, 1000)
    cfg = dict(churn=1, p_fail=0.02, churn_seed=5) if churn else {}
    set_kind(monkeypatch, kind)
    runs = []
    for track in (False, True):
        with pkg.GossipEngine(0, **cfg) as eng:
            eng.load_graph(g)
            eng.set_messages(origin, inject)
            eng.track_load(track)
            eng.reset()
            runs.append(run(eng, inject))
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert set(STAT_KEYS) <= set(a)
        for k in a:
            if not k.endswith("_ms"):
                assert a[k] == b[k], (k, a["round"], a[k], b[k])
