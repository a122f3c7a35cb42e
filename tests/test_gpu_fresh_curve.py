"""Fresh-delivery curves (csrc/fresh_curve.hip, gp_track_fresh_curve /
gp_read_fresh_curve) against the CPU oracle.

fresh_curve[R][k] is the sends of message k in round R - 1 that delivered a
first receipt: the deliverers behind the spread curve's curve[R][k].  Every case
compares fresh_curve() exactly with tests/fresh_curve_ref.py, which evaluates
the first-receipt formula of DESIGN.md §2.4 on the oracle's outputs alone (and
is held to a per-delivery replay by test_fresh_curve_ref.py), and checks that
every other output of the tracked run equals the oracle's as before.

Shapes are the smallest that reach each path: 4,099 vertices (no multiple of a
wave's 64 owners) and 5 (fewer than one wave), every row width, the five
direction / scan modes (every commit path must store the receivers' new rows),
hubs split over items and long rows walked whole, a double star whose hubs have
5,000 simultaneous deliverers of one message (more than a plane set holds, so
the planes fill within one receiver), one block walking a whole overlay
(GP_FRESH_CURVE_GRID=1: the planes fill across owners), churn and explicit
crashes, directed overlays, aliased Message-Lists, message shards, both
fresh-delivery records together, and the lifecycle.
"""
import ctypes
import functools

import numpy as np
import pytest

import directed_shapes as ds
import fresh_curve_ref
import fresh_ref
from test_gpu_curve import (MODE_IDS, MODES, PLANE_ROWS, _alias_ref, _width_ref, check_curve, check_run, mode_cfg,
                            overlay, run)
from test_gpu_fresh import CHURN, _churn_ref, _crash_shapes, _hub_ref, _outputs, _same, _status, check_fresh

pytestmark = pytest.mark.gpu

LEAVES = 5000   # the double star's


def tracked(pkg, g, origin, inject, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.track_fresh_curve()
    eng.reset()
    return eng


def check_fc(eng, exp, columns=None):
    """fresh_curve() against the expected int64 [rows][m] (columns: the sample
    of messages `exp` holds)"""
    got = eng.fresh_curve()
    assert got.dtype == np.uint64 and got.shape == (exp.shape[0], eng.m)
    got = got.astype(np.int64)
    if columns is not None:
        got = got[:, columns]
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:8]


_EXP = {}


def expected(key, g, ref, **kw):
    """fresh_curve_ref.curve, once per shape"""
    if key not in _EXP:
        _EXP[key] = fresh_curve_ref.curve(g, ref, **kw)
    return _EXP[key]


# -- sizes, widths, modes -----------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [1, 100, 1000, 4096])
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_modes(pkg, oracle, n, m, mode):
    g, origin, inject, ref = _width_ref(n, m)
    exp = expected(("width", n, m), g, ref)
    assert int(exp["curve"].sum()) >= sum(s["new_bits"] for s in ref["stats"])
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_fc(eng, exp["curve"])
        check_fc(eng, exp["curve"])   # a read changes nothing
        check_run(eng, stats, ref)


@pytest.mark.parametrize("m", [100, 4096])
def test_read_between_rounds(pkg, oracle, m):
    g, origin, inject, ref = _width_ref(4099, m)
    exp = expected(("width", 4099, m), g, ref)
    with tracked(pkg, g, origin, inject) as eng:
        assert eng.fresh_curve().shape == (1, m) and not eng.fresh_curve().any()
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            check_fc(eng, exp["per_round"][r])
            assert int(exp["per_round"][r][r + 1].sum()) >= stats[-1]["new_bits"]
        check_run(eng, stats, ref)


# -- hubs and full planes -----------------------------------------------------

@pytest.mark.parametrize("hub_threshold", [64, 1 << 30], ids=["split", "whole"])
def test_hubs(pkg, oracle, hub_threshold):
    """hub_threshold=64: k_fresh_curve_hub walks the items of every receiver
    above 64 arcs; 1 << 30: nothing is split and the main kernel walks the long
    rows."""
    g, origin, ref = _hub_ref()
    assert np.diff(g.row_ptr).max() > 1000
    exp = expected("hub", g, ref)
    with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
        stats = run(eng, None)
        check_fc(eng, exp["curve"])
        check_run(eng, stats, ref)


@functools.lru_cache(maxsize=None)
def _star_ref(m):
    import _gossip_pkg
    from oracle import lib
    pkg = _gossip_pkg.load()
    g = fresh_curve_ref.double_star(pkg, LEAVES)
    origin = np.array([0, 2, 1], np.int32)[np.arange(m) % 3]   # cycling A, leaf 2, B
    return g, origin, lib.run(g, origin, None, want_first=True)


@pytest.mark.parametrize("hub_threshold", [1 << 30, 64], ids=["whole", "split"])
@pytest.mark.parametrize("m", [3, 4096])
def test_double_star(pkg, oracle, m, hub_threshold):
    """Hubs A and B, each adjacent to all of 5,000 leaves: in round 1 hub B (or
    A) hears a hub's message from every leaf at once -- 5,000 deliverers of one
    receipt, 2,500 rows per row slot at W = 64, more than the 2,047 a plane set
    holds: the planes fill within one receiver.  Expected by hand."""
    assert LEAVES // 2 > PLANE_ROWS
    g, origin, ref = _star_ref(m)
    assert ref["rounds"] == 3 and (ref["coverage"] == LEAVES + 2).all()
    hand = fresh_curve_ref.double_star_expected(LEAVES, origin == 2)
    if m == 3:
        assert hand.tolist() == [[0, 0, 0], [5000, 2, 5000], [5000, 9998, 5000], [0, 0, 0]]
    with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
        assert eng.words == (1 if m == 3 else 64)
        stats = run(eng, None)
        check_fc(eng, hand)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("m", [100, 4096])
def test_full_planes_across_owners(pkg, oracle, monkeypatch, m):
    """One block walks every owner (GP_FRESH_CURVE_GRID=1), so its waves'
    planes, held across owners and chunks, fill more than twice over in the
    densest round.  Two conditions on the reference's live arcs prove it.
    W = 64 (two row slots per wave): the densest round's live arcs exceed
    2 x 2047 x the row slots.  For every width: a wave books at least one row
    per owner that has a live arc (at W = 2 a 64-arc step is one row in each of
    the 64 row slots, so it is owners and steps that fill narrow planes, not
    arcs -- 2 x 2047 x 64 arcs would be more than this overlay has), and each
    of the block's four waves, which take the 64-owner chunks in turn, has
    more than 2 x 2047 such owners."""
    g = overlay(pkg, 20_000, 10, 2.4, 13)
    origin = pkg.overlay.random_origins(g.n, m, seed=13)
    ref = oracle.run(g, origin, None, want_first=True)
    exp = expected(("planes", m), g, ref)
    W = 64 if m > 2048 else 2
    dense = int(np.argmax(exp["live_arcs"]))
    if W == 64:
        assert exp["live_arcs"][dense] > 2 * PLANE_ROWS * 2
    first = ref["first"]
    src = np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.row_ptr))
    live = (first == dense).any(axis=1)[src] & (first == dense + 1).any(axis=1)[dst]
    owners = np.unique(dst[live])
    waves = 4   # csrc/fresh_curve.hip FC_WAVES: wave w of the one block takes the chunks c = w mod 4
    per_wave = np.bincount((owners // 64) % waves, minlength=waves)
    assert (per_wave > 2 * PLANE_ROWS).all(), per_wave
    monkeypatch.setenv("GP_FRESH_CURVE_GRID", "1")
    with tracked(pkg, g, origin, None, hub_threshold=1 << 30) as eng:
        assert eng.words == W
        stats = run(eng, None)
        check_fc(eng, exp["curve"])
        check_run(eng, stats, ref)


# -- liveness -----------------------------------------------------------------

@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("m", [100, 1000])
def test_churn(pkg, oracle, m, mode):
    g, origin, inject, ref = _churn_ref(m)
    tot = {k: sum(s[k] for s in ref["stats"]) for k in ("crashed", "removals", "lost", "new_bits")}
    assert tot["crashed"] > 0 and tot["removals"] > 0 and tot["lost"] > 0
    exp = expected(("churn", m), g, ref, **CHURN)
    assert int(exp["curve"].sum()) >= tot["new_bits"]
    with tracked(pkg, g, origin, inject, churn=1, p_fail=0.02, churn_seed=5, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_fc(eng, exp["curve"])
        check_run(eng, stats, ref)
        lost = ref["first"][origin, np.arange(m)] == 255   # lost at a down origin: nobody delivered it
        assert lost.any() and not eng.fresh_curve()[:, lost].any()


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("which", ["after-receipt", "top-hub"])
def test_explicit_crashes(pkg, oracle, which, mode):
    """A crash in the round right after a receipt drops that frontier: its row is
    stale and must not be read, and what the vertex received still had its
    deliverers.  A crash of the top hub takes the busiest receiver out."""
    g, origin, inject, plain = _width_ref(4099, 100)
    crashes = _crash_shapes(plain, g)[which]
    ref = ds.CachedOracle(oracle).run(g, origin, inject, crashes=crashes, want_first=True)
    exp = expected(("crash", which), g, ref, crashes=crashes)
    assert not np.array_equal(exp["curve"], expected(("width", 4099, 100), g, plain)["curve"][:ref["rounds"] + 1])
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject, crashes)
        check_fc(eng, exp["curve"])
        check_run(eng, stats, ref)


# -- directed -----------------------------------------------------------------

@pytest.mark.parametrize("crash", [False, True], ids=["plain", "crash"])
@pytest.mark.parametrize("shape", ["down", "up", "first3"])
def test_directed(pkg, oracle, shape, crash):
    """in-degree != out-degree: hubs that only send, hubs that only receive; the
    pass walks the in-CSR whatever the overlay"""
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
    assert int(exp["curve"].sum()) > 0
    for hub_threshold in (64, 1 << 30):
        with tracked(pkg, g, origin, None, hub_threshold=hub_threshold) as eng:
            stats = run(eng, None, crashes)
            check_fc(eng, exp["curve"])
            check_run(eng, stats, ref)


# -- aliased Message-Lists and receiver lists ----------------------------------

ALIAS_WORDS = [0, 9, 18, 27, 36, 45, 54, 63]   # two words of each of a row's four 128-B lines


def test_aliases_and_receiver_lists(pkg, oracle):
    """The shape of test_aliased_message_lists (W = 64): receivers that complete
    commit an alias of their component row and no row of their own -- their new
    bits must still be stored as a frontier row.  The reference of 120,000 x
    4096 takes its time per bit column, so the columns of eight words spread
    over the row's four lines are compared exactly, and every row's sum over
    all 4096 columns against the growth of fresh_ref's sum of fresh_recv."""
    g = overlay(pkg, 120_000, 12, 2.4, 41)
    origin = pkg.overlay.random_origins(g.n, 4096, seed=41)
    ref = _alias_ref(pkg)
    exp = expected("alias", g, ref, words=ALIAS_WORDS)
    sums = [int(v.sum()) for _, v in fresh_ref.totals(g, ref)["per_round"]]
    with tracked(pkg, g, origin, None, push_ratio=0.0, unfiltered_pct=0, hub_threshold=1 << 30,
                 arc_mask_permille=0, compact_rows=0) as eng:
        stats = run(eng, None)
        assert sum(s["aliased"] for s in stats) > 0
        assert any(s["scan"] & 128 for s in stats)
        check_fc(eng, exp["curve"], exp["columns"])
        rows = eng.fresh_curve().astype(np.int64).sum(axis=1)
        assert rows.tolist() == [0] + np.diff([0] + sums).tolist()
        check_run(eng, stats, ref)


# -- message shards -----------------------------------------------------------

def test_message_shards_concatenate(pkg, oracle):
    g, origin, inject, ref = _width_ref(4099, 4096)
    exp = expected(("width", 4099, 4096), g, ref)
    parts = []
    digest = np.zeros(g.n, np.uint64)
    for lo, hi in ((0, 1024), (1024, 4096)):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.track_fresh_curve()
            eng.reset()
            stats = run(eng, inject[lo:hi])
            part = eng.fresh_curve().astype(np.int64)
            assert part.shape == (len(stats) + 1, hi - lo)
            parts.append(np.pad(part, ((0, ref["rounds"] + 1 - part.shape[0]), (0, 0))))   # (a shard may stop earlier)
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
            digest ^= eng.digest()
    assert np.array_equal(np.concatenate(parts, axis=1), exp["curve"])
    assert np.array_equal(digest, ref["digest"])


# -- both fresh-delivery records, and nothing else moves -------------------------

@pytest.mark.parametrize("churn", [False, True], ids=["plain", "churn"])
def test_both_records_and_nothing_else_moves(pkg, oracle, churn):
    """an untracked run, a run with gp_track_fresh_curve alone, and one with
    gp_track_fresh and the spread curve beside it: identical outputs and
    gp_round_stats (with this record alone the work counters too, timings
    aside); with both fresh-delivery records on, the row sums are the growth of
    sum fresh_recv round by round, and all records match their references"""
    g, origin, inject, ref = _churn_ref(100) if churn else _width_ref(4099, 1000)
    kw = CHURN if churn else {}
    cfg = dict(churn=1, p_fail=0.02, churn_seed=5) if churn else {}
    exp = expected(("churn", 100) if churn else ("width", 4099, 1000), g, ref, **kw)
    fexp = fresh_ref.totals(g, ref, **kw)
    outs = []
    for records in ((), ("fresh_curve",), ("fresh_curve", "fresh", "curve")):
        with pkg.GossipEngine(0, **cfg) as eng:
            eng.load_graph(g)
            eng.set_messages(origin, inject)
            for rec in records:
                getattr(eng, "track_" + rec)()
            eng.reset()
            if "fresh" not in records:
                outs.append(_outputs(pkg, eng, inject))
            else:   # round by round: the two records move together
                stats, prev = [], 0
                last = int(np.max(inject))
                while not stats or stats[-1]["new_bits"] or stats[-1]["round"] < last:
                    stats.append(eng.round())
                    total = int(eng.fresh_recv().astype(np.int64).sum())
                    assert int(eng.fresh_curve()[-1].astype(np.int64).sum()) == total - prev, len(stats)
                    prev = total
                check_fresh(eng, fexp)
                check_curve(eng.curve(), ref, inject)
                check_run(eng, stats, ref)
                assert int(eng.fresh_curve().astype(np.int64).sum()) == int(eng.fresh_sent().astype(np.int64).sum())
            if records:
                check_fc(eng, exp["curve"])
    # tracking makes neither GP_FRONTIER nor (under churn) GP_FORWARDS readable
    assert outs[0]["frontier"] == pkg._lib.GP_ENOTRACK
    _same(outs[0], outs[1], work_counters=True)
    assert np.array_equal(outs[1]["digest"], ref["digest"])


def test_helpers_on_a_run(pkg, oracle):
    """redundancy.py's per-message views on a real run's arrays"""
    g, origin, inject, ref = _width_ref(4099, 100)
    with pkg.GossipEngine(0, track_msg_forwards=1) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.track_fresh_curve()
        eng.track_curve()
        eng.reset()
        run(eng, inject)
        fc, cv = eng.fresh_curve(), eng.curve()
        eng.finalize()
        cov, fwd = eng.coverage(), eng.forwards()
    red = pkg.redundancy
    d = red.message_deliverers(fc)
    assert (d >= cov.astype(np.int64) - 1).all() and (d <= fwd.astype(np.int64)).all()
    per = red.deliverers_per_receipt(fc, cov)
    reached = cov > 1                                   # (an isolated origin's message reaches nobody: 0.0)
    assert reached.any() and (per[reached] >= 1.0).all() and not per[~reached].any()
    assert per.max() > 1.0                              # an overlay with cycles: some receipt had two deliverers
    assert (red.message_redundancy(fwd, cov) >= per - 1.0).all()
    by_round = red.deliverers_by_round(fc, cv)
    assert by_round.shape == fc.shape and by_round.max() >= per.max()


# -- lifecycle ----------------------------------------------------------------

def test_errors_and_lifecycle(pkg, oracle):
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = expected(("width", 4099, 100), g, ref)
    lib = pkg._lib
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        assert _status(pkg, eng.fresh_curve) == lib.GP_ENOTRACK    # not tracked
        eng.track_fresh_curve()
        assert _status(pkg, eng.fresh_curve) == lib.GP_ENOTRACK    # takes effect at the next reset
        eng.reset()
        assert eng.fresh_curve().shape == (1, 100)
        stats = [eng.round() for _ in range(3)]
        buf = np.full((3, 100), 0xABCD, np.uint64)                  # a short buffer: refused, nothing written
        rows = ctypes.c_int32(-7)
        read = eng._lib.gp_read_fresh_curve
        assert read(eng._ctx, ctypes.c_void_p(buf.ctypes.data), 3, ctypes.byref(rows)) == lib.GP_EINVAL
        assert rows.value == -7 and (buf == 0xABCD).all()
        assert read(eng._ctx, None, 255, ctypes.byref(rows)) == lib.GP_EINVAL
        assert read(eng._ctx, ctypes.c_void_p(buf.ctypes.data), 255, None) == lib.GP_EINVAL
        assert read(None, ctypes.c_void_p(buf.ctypes.data), 255, ctypes.byref(rows)) == lib.GP_EINVAL
        assert eng._lib.gp_track_fresh_curve(None, 1) == lib.GP_EINVAL
        assert rows.value == -7 and (buf == 0xABCD).all()
        check_fc(eng, exp["per_round"][2])
        while not (stats[-1]["new_bits"] == 0 and stats[-1]["round"] >= 2):
            stats.append(eng.round())
        check_fc(eng, exp["curve"])
        check_run(eng, stats, ref)
        eng.reset()                                                 # a second run carries nothing over
        assert eng.fresh_curve().shape == (1, 100) and not eng.fresh_curve().any()
        stats = [eng.round() for _ in range(3)]
        check_fc(eng, exp["per_round"][2])
        eng.track_fresh_curve(False)                                # off again: at the next reset
        check_fc(eng, exp["per_round"][2])
        eng.reset()
        assert _status(pkg, eng.fresh_curve) == lib.GP_ENOTRACK
        stats = run(eng, inject)                                    # and the untracked run is the oracle's
        check_run(eng, stats, ref)
        # a blob of a run without frontier rows is not one of a run with them
        eng.reset()
        plain = eng.checkpoint()
        eng.track_fresh_curve()
        assert _status(pkg, lambda: eng.restore(plain)) == lib.GP_EINVAL
    # a run restored past round 0: the record is not in the blob
    with tracked(pkg, g, origin, inject) as eng:
        blob0 = eng.checkpoint()
        stats = [eng.round() for _ in range(3)]
        blob3 = eng.checkpoint()
        with tracked(pkg, g, origin, inject) as other:
            other.restore(blob3)
            assert _status(pkg, other.fresh_curve) == lib.GP_ESTATE
            more = run(other, inject)
            assert _status(pkg, other.fresh_curve) == lib.GP_ESTATE
            check_run(other, stats + more, ref)                     # the restored run itself is exact
            other.reset()
            run(other, inject)
            check_fc(other, exp["curve"])
            other.restore(blob0)                                    # a blob of round 0 has counted nothing yet
            assert other.fresh_curve().shape == (1, 100) and not other.fresh_curve().any()
            run(other, inject)
            check_fc(other, exp["curve"])


def test_partitioned_context_keeps_no_fresh_curve(pkg, oracle):
    g, origin, inject, _ = _width_ref(4099, 100)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.track_fresh_curve()
        eng.reset()
        assert _status(pkg, eng.fresh_curve) == pkg._lib.GP_ENOTRACK
