"""Spread curves (csrc/curve.hip, gp_track_curve / gp_read_curve) against the
CPU oracle.

curve[r][k] = vertices whose first receipt of message k has receipt round r:
the aggregate of what each reference peer logs per arrival (Peer.py:175-216).
The reference of every case is the oracle's first-receipt matrix
(oracle.run(..., want_first=True)), never the engine's own first(): the
expected curve is (first == r).sum(axis=0) for r = 0 .. rounds, compared
exactly.  Every case also checks the three sums the oracle gives directly:
row r's expansion part against stats[r-1].new_bits, its injection part
against stats[r].injected, each column's total against coverage[k].

Shapes are the smallest that reach each path: vertex counts that are no
multiple of any 64 / W rows per wave step (4,099) and fewer than one step (5),
every row width, the five direction / scan modes of test_gpu_parity, hubs
split over waves, crashes right after a receipt, aliased Message-Lists and
receiver lists (the shape of test_aliased_message_lists), planes that fill
(one block, via GP_CURVE_GRID), and a vertex partition.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAT_KEYS = ("injected", "lost", "new_bits", "receivers", "sends", "active", "crashed",
             "reports", "removals", "dup_reports")
# (push_ratio, unfiltered_pct, flat_max_words, arc_mask_permille): test_gpu_parity.MODES
MODES = [(0.0, 0, 0, 0), (0.0, 0, 0, 1), (0.0, 1, 32, 0), (1e-12, 90, 16, 10), (10.0, 90, 16, 10)]
MODE_IDS = ["pull", "pull-masked", "pull-unfiltered", "push", "adaptive"]
PLANE_ROWS = 2047   # csrc/curve_planes.h CURVE_PLANE_ROWS (tests/test_curve_planes.py pins it)


def mode_cfg(mode):
    push_ratio, unfiltered_pct, flat_max_words, arc_mask = mode
    return dict(push_ratio=push_ratio, unfiltered_pct=unfiltered_pct, flat_max_words=flat_max_words,
                arc_mask_permille=arc_mask)


@functools.lru_cache(maxsize=None)
def _overlay(n, dbar, gamma, seed):
    from oracle import lib
    return lib.chung_lu(n, dbar, gamma, seed)


def overlay(pkg, n, dbar=8, gamma=2.2, seed=7):
    rp, col = _overlay(n, dbar, gamma, seed)
    return pkg.CSR(n, rp, col, False)


def histogram(first, rows):
    return np.stack([(first == r).sum(axis=0) for r in range(rows)]).astype(np.uint64)


def tracked(pkg, g, origin, inject, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.track_curve()
    eng.reset()
    return eng


def run(eng, inject, crashes=(), max_rounds=254):
    by_round = {}
    for v, r in crashes:
        by_round.setdefault(r, []).append(v)
    last = int(np.max(inject)) if inject is not None and len(inject) else 0
    stats = []
    for r in range(len(stats), max_rounds):
        if r in by_round:
            eng.crash(by_round[r])
        st = eng.round()
        stats.append(st)
        if st["new_bits"] == 0 and st["round"] >= last:
            break
    return stats


def check_curve(curve, ref, inject):
    """curve against the oracle's run `ref` (first matrix, stats, coverage)."""
    m = ref["first"].shape[1]
    R = ref["rounds"]
    inj = np.zeros(m, np.int64) if inject is None else np.asarray(inject, np.int64)
    assert curve.dtype == np.uint64 and curve.shape == (R + 1, m)
    exp = histogram(ref["first"], R + 1)
    assert np.array_equal(curve, exp), np.argwhere(curve != exp)[:8]
    for r in range(R + 1):
        # message k's column holds an injection in row inject_round[k] and nowhere
        # else; before that round the message does not exist, so that entry has no
        # expansion part
        inj_part = int(curve[r, inj == r].sum())
        exp_part = int(curve[r, inj != r].sum())
        assert exp_part == (ref["stats"][r - 1]["new_bits"] if r >= 1 else 0), r
        assert inj_part == (ref["stats"][r]["injected"] if r < R else 0), r
    assert np.array_equal(curve.sum(axis=0), ref["coverage"])


def check_run(eng, stats, ref):
    """every other output of a tracked run equals the oracle's as before"""
    assert len(stats) == ref["rounds"]
    for a, b in zip(stats, ref["stats"]):
        for k in STAT_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    eng.finalize()
    assert np.array_equal(eng.seen(), ref["seen"][:, :eng.words])
    assert np.array_equal(eng.digest(), ref["digest"])
    assert np.array_equal(eng.coverage(), ref["coverage"])


@functools.lru_cache(maxsize=None)
def _width_ref(n, m):
    import _gossip_pkg
    from oracle import lib
    pkg = _gossip_pkg.load()
    g = overlay(pkg, n, 8 if n > 5 else 2, 2.2, 7)
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 3).astype(np.int32)
    return g, origin, inject, lib.run(g, origin, inject, want_first=True)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [1, 64, 100, 512, 1000, 2048, 4096])
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_tails(pkg, oracle, n, m, mode):
    g, origin, inject, ref = _width_ref(n, m)
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_curve(eng.curve(), ref, inject)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [100, 4096])
def test_hub_commits_feed_the_count(pkg, oracle, m, mode):
    """hub_threshold=64: the receivers k_hub_final commits are counted too."""
    g, origin, inject, ref = _width_ref(4099, m)
    assert np.diff(g.row_ptr).max() > 4 * 64
    with tracked(pkg, g, origin, inject, hub_threshold=64, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_curve(eng.curve(), ref, inject)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("schedule", ["mod3", "c1"])
def test_injections_and_reset(pkg, oracle, schedule, mode):
    """Staggered inject rounds, several messages of one origin, and a second
    run after a reset: no stale frontier row or count survives it."""
    g = overlay(pkg, 4099)
    if schedule == "c1":   # 10 messages per origin, one every 5 rounds, up to round 5 (n - 1) = 45
        origin, inject, _ = pkg.peer.c1_schedule(10)
        origin, inject = np.array(origin, np.int32) * 400 + 3, np.array(inject, np.int32)
        assert inject.max() == 45
    else:
        origin = np.repeat(pkg.overlay.random_origins(g.n, 75, seed=3), 4)   # 4 messages per origin
        inject = (np.arange(origin.size) % 3).astype(np.int32)
    assert len(set(origin.tolist())) < origin.size
    ref = oracle.run(g, origin, inject, want_first=True)
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        first_curve = eng.curve()
        check_curve(first_curve, ref, inject)
        check_run(eng, stats, ref)
        eng.reset()
        assert eng.curve().shape == (1, origin.size) and not eng.curve().any()
        run(eng, inject)
        assert np.array_equal(eng.curve(), first_curve)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_stopping_early(pkg, oracle, mode):
    """After R = 2 rounds the curve has 3 rows: row 2 holds the receipts of
    round 1's expansion, round 2's injections are not made yet -- as
    oracle.run(max_rounds=2)."""
    g, origin, inject, ref = _width_ref(4099, 1000)
    ref2 = oracle.run(g, origin, inject, want_first=True, max_rounds=2)
    assert ref2["rounds"] == 2 and (inject == 2).any()
    with tracked(pkg, g, origin, inject, **mode_cfg(mode)) as eng:
        stats = [eng.round(), eng.round()]
        check_curve(eng.curve(), ref2, inject)
        while not (stats[-1]["new_bits"] == 0 and stats[-1]["round"] >= 2):
            stats.append(eng.round())
        check_curve(eng.curve(), ref, inject)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_crash_right_after_receipt(pkg, oracle, mode):
    """50 vertices with a first receipt in round 3 crash in round 3: k_churn
    zeroes their frontier counts before they send, their receipts stay in
    row 3 and their forwards vanish."""
    g = overlay(pkg, 20_000, 8, 2.4, 5)
    origin = pkg.overlay.random_origins(g.n, 256, seed=5)
    plain = oracle.run(g, origin, None, want_first=True)
    picked = np.nonzero((plain["first"] == 3).any(axis=1))[0][:50]
    assert picked.size == 50
    crashes = [(int(v), 3) for v in picked]
    ref = oracle.run(g, origin, None, crashes=crashes, want_first=True)
    assert (ref["first"][picked] == 3).any(), "no crashed vertex received in round 3"
    assert not np.array_equal(ref["forwards"], plain["forwards"])
    with tracked(pkg, g, origin, None, **mode_cfg(mode)) as eng:
        stats = run(eng, None, crashes)
        check_curve(eng.curve(), ref, None)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
@pytest.mark.parametrize("track_fwd", [0, 1])
def test_random_churn(pkg, oracle, track_fwd, mode):
    g = overlay(pkg, 20_000, 8, 2.4, 5)
    origin = pkg.overlay.random_origins(g.n, 1024, seed=9)
    inject = (np.arange(1024) % 3).astype(np.int32)
    ref = _churn_ref(g, tuple(origin.tolist()), tuple(inject.tolist()))
    assert sum(s["crashed"] for s in ref["stats"]) > 0
    with tracked(pkg, g, origin, inject, churn=1, p_fail=0.01, churn_seed=9, track_msg_forwards=track_fwd,
                 **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_curve(eng.curve(), ref, inject)
        check_run(eng, stats, ref)
        if track_fwd:
            assert np.array_equal(eng.forwards(), ref["forwards"])
        else:   # tracking the curve does not make the forwards or the frontier readable
            for read in (eng.forwards, eng.frontier):
                with pytest.raises(pkg.GossipError) as e:
                    read()
                assert e.value.status == pkg._lib.GP_ENOTRACK


_CHURN = {}


def _churn_ref(g, origin, inject):
    from oracle import lib
    key = (g.n, origin, inject)
    if key not in _CHURN:
        _CHURN[key] = lib.run(g, np.array(origin, np.int32), np.array(inject, np.int32), churn=True, p_fail=0.01,
                              churn_seed=9, want_first=True)
    return _CHURN[key]


@pytest.mark.parametrize("mode", ["pull", "adaptive"])
def test_aliases_and_receiver_lists(pkg, oracle, mode):
    """The shape of test_aliased_message_lists: receivers that complete their
    component write no row but still store their new bits, and the last pulls
    take their receivers from a list."""
    push_ratio, unfiltered_pct, hub = {"pull": (0.0, 0, 1 << 30), "adaptive": (10.0, 90, 4096)}[mode]
    g = overlay(pkg, 120_000, 12, 2.4, 41)
    origin = pkg.overlay.random_origins(g.n, 4096, seed=41)
    ref = _alias_ref(pkg)
    with tracked(pkg, g, origin, None, push_ratio=push_ratio, unfiltered_pct=unfiltered_pct, hub_threshold=hub,
                 arc_mask_permille=0, compact_rows=0) as eng:
        stats = run(eng, None)
        assert sum(s["aliased"] for s in stats) > 0
        assert any(s["scan"] & 64 for s in stats)
        assert any(s["scan"] & 128 for s in stats)   # (adaptive: its last pull, before the pushes)
        check_curve(eng.curve(), ref, None)
        check_run(eng, stats, ref)


@functools.lru_cache(maxsize=None)
def _alias_ref(pkg):
    from oracle import lib
    g = overlay(pkg, 120_000, 12, 2.4, 41)
    return lib.run(g, pkg.overlay.random_origins(g.n, 4096, seed=41), None, want_first=True)


@pytest.mark.parametrize("n,m", [(30_000, 2049), (200_000, 512)], ids=["W64", "W8"])
def test_full_planes(pkg, oracle, monkeypatch, n, m):
    """One block counts every row (GP_CURVE_GRID=1), so each of its four waves
    fills its planes more than twice over in the densest round."""
    g = overlay(pkg, n, 10, 2.4, 13)
    origin = pkg.overlay.random_origins(g.n, m, seed=13)
    ref = oracle.run(g, origin, None, want_first=True)
    W = 64 if m > 2048 else 8
    assert max(s["receivers"] for s in ref["stats"]) > 2 * PLANE_ROWS * 4 * (64 // W)
    monkeypatch.setenv("GP_CURVE_GRID", "1")
    with tracked(pkg, g, origin, None) as eng:
        assert eng.words == W
        stats = run(eng, None)
        check_curve(eng.curve(), ref, None)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("churn", [False, True])
def test_partition(pkg, oracle, churn):
    """Three contexts of a vertex partition on one GPU: each counts its owned
    vertices, as GP_COVERAGE does, and the curves add up to the oracle's."""
    g = pkg.overlay.barabasi_albert(3001, 2, seed=8)
    origin = pkg.overlay.random_origins(g.n, 200, seed=8)
    inject = (np.arange(200) % 4).astype(np.int32)
    kw = dict(churn=True, p_fail=0.02, churn_seed=3) if churn else {}
    cfg = dict(churn=1, p_fail=0.02, churn_seed=3, track_msg_forwards=1) if churn else {}
    ref = oracle.run(g, origin, inject, want_first=True, **kw)
    engs = []
    for k in range(3):
        e = pkg.GossipEngine(0, **cfg)
        e.load_graph(g)
        e.set_partition(k, 3)
        e.set_messages(origin, inject)
        e.track_curve()
        e.reset()
        engs.append(e)
    stats = pkg.GossipEngine.run_group(engs)
    assert len(stats) == ref["rounds"]
    for a, b in zip(stats, ref["stats"]):
        for k in STAT_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    curves = [e.curve() for e in engs]
    for e, c in zip(engs, curves):   # a context's curve is the histogram of its owned slice
        lo, hi = e.partition()
        assert np.array_equal(c, histogram(ref["first"][lo:hi], ref["rounds"] + 1))
    check_curve(sum(curves[1:], curves[0]), ref, inject)
    for e in engs:
        e.close()


def test_errors_and_lifecycle(pkg, oracle):
    g, origin, inject, ref = _width_ref(4099, 100)
    lib = pkg._lib
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        with pytest.raises(pkg.GossipError) as e:   # not tracked
            eng.curve()
        assert e.value.status == lib.GP_ENOTRACK
        eng.track_curve()
        with pytest.raises(pkg.GossipError) as e:   # takes effect at the next reset
            eng.curve()
        assert e.value.status == lib.GP_ENOTRACK
        eng.reset()
        assert eng.curve().shape == (1, 100)
        stats = [eng.round() for _ in range(3)]
        # a short buffer: GP_EINVAL, nothing written
        import ctypes
        buf = np.full((3, 100), 0xABCD, np.uint64)
        rows = ctypes.c_int32(-7)
        rc = eng._lib.gp_read_curve(eng._ctx, 0, ctypes.c_void_p(buf.ctypes.data), 3, ctypes.byref(rows))
        assert rc == lib.GP_EINVAL and rows.value == -7 and (buf == 0xABCD).all()
        rc = eng._lib.gp_read_curve(eng._ctx, 2, ctypes.c_void_p(buf.ctypes.data), 3, ctypes.byref(rows))
        assert rc == lib.GP_EINVAL
        with pytest.raises(pkg.GossipError) as e:   # no shard job
            eng.job_curve(100)
        assert e.value.status == lib.GP_ESTATE
        mid = eng.curve()
        assert mid.shape == (4, 100)
        blob3 = eng.checkpoint()
        # a restore past round 0: the blob holds no curve
        eng.restore(blob3)
        with pytest.raises(pkg.GossipError) as e:
            eng.curve()
        assert e.value.status == lib.GP_ESTATE
        while not (stats[-1]["new_bits"] == 0 and stats[-1]["round"] >= 2):
            stats.append(eng.round())
        with pytest.raises(pkg.GossipError) as e:
            eng.curve()
        assert e.value.status == lib.GP_ESTATE
        check_run(eng, stats, ref)   # the restored run itself is exact
        # the next reset gives a valid curve again
        eng.reset()
        blob0 = eng.checkpoint()
        stats = run(eng, inject)
        check_curve(eng.curve(), ref, inject)
        # a restore at round 0 keeps the curve valid
        eng.restore(blob0)
        assert eng.curve().shape == (1, 100) and not eng.curve().any()
        stats = run(eng, inject)
        check_curve(eng.curve(), ref, inject)
        check_run(eng, stats, ref)
        # tracking off again: at the next reset
        eng.track_curve(False)
        assert eng.curve().shape == (len(stats) + 1, 100)
        eng.reset()
        with pytest.raises(pkg.GossipError) as e:
            eng.curve()
        assert e.value.status == lib.GP_ENOTRACK
        # a blob of a run without frontier rows is not one of a run with them
        plain = eng.checkpoint()
        eng.track_curve()
        with pytest.raises(pkg.GossipError) as e:
            eng.restore(plain)
        assert e.value.status == lib.GP_EINVAL


def test_spread_helpers_on_a_run(pkg, oracle):
    """spread.py on a real curve: cumulative ends at the coverage, and every
    message that reached anyone reached its first holder at its inject round."""
    g, origin, inject, ref = _width_ref(4099, 100)
    with tracked(pkg, g, origin, inject) as eng:
        run(eng, inject)
        curve = eng.curve()
    cum = pkg.spread.cumulative(curve)
    assert np.array_equal(cum[-1].astype(np.uint64), ref["coverage"])
    t50 = pkg.spread.rounds_to_reach(curve, inject, 0.5)
    t99 = pkg.spread.rounds_to_reach(curve, inject, 0.99, of=g.n)
    first = ref["first"].astype(np.int64)
    for k in range(100):
        held = np.sort(first[first[:, k] != 255, k])
        assert t50[k] == held[int(np.ceil(0.5 * held.size)) - 1] - inject[k]
        need = int(np.ceil(0.99 * g.n))
        assert t99[k] == (held[need - 1] - inject[k] if held.size >= need else -1)
