"""Lossy links (csrc/lossy.hip, gp_link_loss) on the GPU.

With loss on, the line a peer writes to one link in its send loop
(Peer.py:402-404) arrives iff the link's draw of that round passes; the peer
sends once, so a dropped line is lost for good.  Two references, neither of
them the engine:
 - with p = 0 every arc is open and k_expand_lossy / k_hub_lossy must give the
   C oracle's flood (oracle.run) bit for bit -- from frontier rows, where the
   planner's pulls read whole Message-Lists;
 - with p > 0 the numpy round loop of tests/lossy_ref.py (pinned to the oracle
   and to the draw alone by tests/test_lossy_ref.py): first-receipt matrix,
   seenpop, the per-round counters, coverage and forwards, all exact.
Every lossy case first asserts, on the reference alone, that loss changed at
least a fifth of the first-receipt cells against the flood's: a kernel that
ignored the draw could not pass.

Shapes are test_gpu_delay.py's: 4,099 vertices (no multiple of a wave's 64)
and 5 (fewer than one wave), every row width with partial last words, hubs
split over the hub table (hub_threshold=64: 44 receivers, one of in-degree
913), a directed overlay, a raw CSR with self-loops and repeated arcs.
"""
import functools

import numpy as np
import pytest

import delay_dist_ref
import delay_ref
import directed_shapes as ds
import load_ref
import lossy_ref
import raw_csr
from test_gpu_curve import MODE_IDS, MODES, _width_ref, check_run, histogram, mode_cfg, overlay, run
from test_gpu_delay import WIDTH_MS, WORDS
from test_gpu_fresh import _status

pytestmark = pytest.mark.gpu

KEYS = ("injected", "new_bits", "receivers", "sends", "active")
LIVE_KEYS = ("injected", "lost", "new_bits", "receivers", "active", "crashed")


def lossy(pkg, g, origin, inject, p, seed=0, track=(), **cfg):
    cfg.setdefault("track_first", 1)
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.link_loss(p, seed)
    for t in track:
        getattr(eng, t)()
    eng.reset()
    return eng


@functools.lru_cache(maxsize=None)
def _ref(n, m, p, seed):
    g, origin, inject, flood = _width_ref(n, m)
    return g, origin, inject, flood, lossy_ref.run(g, origin, inject, p=p, seed=seed)


def changed_share(ref, flood):
    return float((ref["first"] != flood["first"]).mean())


def check_lossy(eng, stats, ref, keys=KEYS, forwards=True):
    """a lossy run against lossy_ref.run's result: all exact"""
    assert all(s["mode"] == 2 and s["scan"] == 0 for s in stats)
    assert len(stats) == ref["rounds"], (len(stats), ref["rounds"])
    for a, b in zip(stats, ref["stats"]):
        for k in keys:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    first = eng.first()
    bad = np.argwhere(first != ref["first"])
    assert bad.size == 0, (bad[:8], first[tuple(bad[:8].T)], ref["first"][tuple(bad[:8].T)])
    assert np.array_equal(eng.seenpop().astype(np.int64), ref["seenpop"])
    eng.finalize()
    assert np.array_equal(eng.coverage(), ref["coverage"])
    if forwards:
        assert np.array_equal(eng.forwards(), ref["forwards"])


def outputs(eng, stats):
    eng.finalize()
    return ([tuple(s[k] for k in KEYS) for s in stats], eng.first(), eng.digest(), eng.seen(), eng.coverage(),
            eng.forwards())


def same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# -- the kernel against the C oracle: every arc open ----------------------------

def check_flood(eng, stats, ref):
    assert all(s["mode"] == 2 and s["scan"] == 0 for s in stats)
    check_run(eng, stats, ref)
    assert np.array_equal(eng.first(), ref["first"])
    assert np.array_equal(eng.forwards(), ref["forwards"])


@pytest.mark.parametrize("m", WIDTH_MS)
@pytest.mark.parametrize("n", [4099, 5])
def test_open_arcs_are_the_oracles_flood(pkg, oracle, n, m):
    g, origin, inject, ref = _width_ref(n, m)
    with lossy(pkg, g, origin, inject, 0.0) as eng:
        assert eng.info()[3] == WORDS[m] and eng.link_loss_info() == (True, 0.0, 0)
        check_flood(eng, run(eng, inject), ref)


@pytest.mark.parametrize("m", WIDTH_MS)
def test_open_arcs_hubs(pkg, oracle, m):
    """hub_threshold=64: 44 receivers go through k_hub_lossy and the push's receiver side"""
    g, origin, inject, ref = _width_ref(4099, m)
    deg = np.diff(g.row_ptr)
    assert (deg > 64).sum() == 44 and deg.max() == 913
    with lossy(pkg, g, origin, inject, 0.0, hub_threshold=64) as eng:
        check_flood(eng, run(eng, inject), ref)


@pytest.mark.parametrize("hub_threshold", [4096, 64])
@pytest.mark.parametrize("m", [100, 4096])
def test_open_arcs_directed(pkg, oracle, m, hub_threshold):
    g = ds.oriented_chung_lu(pkg, oracle, 4099, 8, 2.2, 7, "coin")
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 3).astype(np.int32)
    ref = ds.CachedOracle(oracle).run(g, origin, inject, want_first=True)
    with lossy(pkg, g, origin, inject, 0.0, hub_threshold=hub_threshold) as eng:
        check_flood(eng, run(eng, inject), ref)


@pytest.mark.parametrize("m", [100, 4096])
def test_open_arcs_raw_csr(pkg, oracle, m):
    """self-loops and repeated arcs: a loop delivers nothing new, parallel arcs share their fate"""
    g = raw_csr.loops_and_repeats(pkg)
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 3).astype(np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    with lossy(pkg, g, origin, inject, 0.0) as eng:
        check_flood(eng, run(eng, inject), ref)
    lref = lossy_ref.run(g, origin, inject, p=0.5, seed=11)
    assert changed_share(lref, ref) >= 0.2
    with lossy(pkg, g, origin, inject, 0.5, 11) as eng:
        check_lossy(eng, run(eng, inject), lref)


# -- against lossy_ref ----------------------------------------------------------

LOSSY_CASES = [(p, m) for p in (0.25, 0.5, 0.9) for m in (64, 100, 512, 1000)] + [(0.5, 2048), (0.5, 4096)]


@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("p,m", LOSSY_CASES)
def test_lossy_run(pkg, oracle, p, m, seed):
    g, origin, inject, flood, ref = _ref(4099, m, p, seed)
    share = changed_share(ref, flood)
    print(f"p={p} m={m} seed={seed}: {share:.3f} of the cells differ from the flood's, {ref['rounds']} rounds")
    assert share >= 0.2
    with lossy(pkg, g, origin, inject, p, seed) as eng:
        assert eng.link_loss_info() == (True, p, seed)
        check_lossy(eng, run(eng, inject), ref)
        if m == 64:   # the digest is still a pure function of the first-receipt matrix
            assert np.array_equal(eng.digest(), oracle.digest_from_first(ref["first"], origin))


@pytest.mark.parametrize("hub_threshold", [4096, 64])
def test_four_word_rows(pkg, oracle, hub_threshold):
    """m = 200: W = 4, the one width WIDTH_MS has no table for"""
    g, origin, inject, flood, ref = _ref(4099, 200, 0.5, 11)
    assert changed_share(ref, flood) >= 0.2
    with lossy(pkg, g, origin, inject, 0.0, hub_threshold=hub_threshold) as eng:
        assert eng.words == 4
        check_flood(eng, run(eng, inject), flood)
    with lossy(pkg, g, origin, inject, 0.5, 11, hub_threshold=hub_threshold) as eng:
        check_lossy(eng, run(eng, inject), ref)


@pytest.mark.parametrize("n,m", [(5, 1), (5, 100), (4099, 1), (5, 4096)])
def test_lossy_run_small(pkg, oracle, n, m):
    """fewer vertices than a wave, one message (no share asserted there)"""
    g, origin, inject, _, ref = _ref(n, m, 0.5, 11)
    with lossy(pkg, g, origin, inject, 0.5, 11) as eng:
        check_lossy(eng, run(eng, inject), ref)


def test_lossy_hubs(pkg, oracle):
    """hub_threshold=64 at p = 0.5: every hub's receipts come in over several
    rounds, each through k_hub_lossy's items and one commit"""
    g, origin, inject, flood, ref = _ref(4099, 1000, 0.5, 11)
    hubs = np.nonzero(np.diff(g.row_ptr) > 64)[0]
    assert hubs.size == 44
    for v in hubs:
        got = ref["first"][v]
        rounds = set(got[(got != 255) & ~((origin == v) & (got == inject))].tolist())   # (its own injections are no receipts)
        assert len(rounds) >= 3, (v, rounds)
    with lossy(pkg, g, origin, inject, 0.5, 11, hub_threshold=64) as eng:
        check_lossy(eng, run(eng, inject), ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [100, 4096])
def test_tuning_fields_change_nothing(pkg, oracle, m, mode):
    g, origin, inject, flood, ref = _ref(4099, m, 0.5, 11)
    with lossy(pkg, g, origin, inject, 0.5, 11, **mode_cfg(mode)) as eng:
        check_lossy(eng, run(eng, inject), ref)


@pytest.mark.parametrize("shards", [2, 8])
def test_message_shards(pkg, oracle, shards):
    """the draw does not see the message: a table run in blocks gives the columns of the whole run"""
    g, origin, inject, flood, ref = _ref(4099, 4096, 0.5, 11)
    step = 4096 // shards
    cols = []
    for k in range(shards):
        with pkg.GossipEngine(0, track_first=1) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, k * step, (k + 1) * step)
            assert eng.words == step // 64
            eng.link_loss(0.5, 11)
            eng.reset()
            stats = eng.run()
            assert all(s["mode"] == 2 for s in stats)
            cols.append(eng.first())
    assert np.array_equal(np.concatenate(cols, axis=1), ref["first"])


# -- schedule and lifecycle -------------------------------------------------------

def test_c1_schedule(pkg, oracle):
    g = overlay(pkg, 4099)
    origin, inject, _ = pkg.peer.c1_schedule(10)
    origin, inject = np.array(origin, np.int32) * 400 + 3, np.array(inject, np.int32)
    assert inject.max() == 45
    flood = ds.CachedOracle(oracle).run(g, origin, inject, want_first=True)
    ref = lossy_ref.run(g, origin, inject, p=0.5, seed=11)
    assert changed_share(ref, flood) >= 0.2
    with lossy(pkg, g, origin, inject, 0.5, 11) as eng:
        check_lossy(eng, run(eng, inject), ref)


def test_lifecycle(pkg, oracle):
    g, origin, inject, flood, ref = _ref(4099, 100, 0.5, 11)
    ref25 = _ref(4099, 100, 0.25, 11)[4]
    ref12 = _ref(4099, 100, 0.5, 12)[4]
    assert not np.array_equal(ref["first"], ref12["first"])
    with lossy(pkg, g, origin, inject, 0.5, 11) as eng:
        stats = run(eng, inject)
        check_lossy(eng, stats, ref)
        a = outputs(eng, stats)
        eng.reset()                      # same seed twice: identical
        stats = run(eng, inject)
        assert same(a, outputs(eng, stats))
        eng.link_loss(0.5, 12)           # another seed differs
        eng.reset()
        stats = run(eng, inject)
        check_lossy(eng, stats, ref12)
        assert not same(a, outputs(eng, stats))
        eng.link_loss(0.25, 11)          # another p
        eng.reset()
        assert eng.link_loss_info() == (True, 0.25, 11)
        eng.round()
        eng.link_loss(0.9, 3)            # a setting made mid-run changes nothing before the reset
        assert eng.link_loss_info() == (True, 0.25, 11)
        stats = [s for s in eng.run()]
        assert len(stats) + 1 == ref25["rounds"]
        assert np.array_equal(eng.first(), ref25["first"])
        eng.link_loss(None)              # back to the oracle's flood
        eng.reset()
        assert eng.link_loss_info() == (False, 0.0, 0)
        stats = run(eng, inject)
        assert all(s["mode"] in (0, 1) for s in stats)
        check_run(eng, stats, flood)
        assert np.array_equal(eng.first(), flood["first"])


def test_every_arc_closed(pkg, oracle):
    """p = 1: the run stops after the last injection with coverage 1 per message"""
    g, origin, inject, flood = _width_ref(4099, 100)
    with lossy(pkg, g, origin, inject, 1.0, 5) as eng:
        stats = run(eng, inject)
        assert len(stats) == int(inject.max()) + 1 and all(s["new_bits"] == 0 and s["mode"] == 2 for s in stats)
        assert sum(s["rows_gathered"] for s in stats) == 0
        check_lossy(eng, stats, lossy_ref.run(g, origin, inject, p=1.0, seed=5))
        assert (eng.coverage() == 1).all()


def test_sweep(pkg, oracle):
    """loss.sweep: one reset and run per p, the survival curve"""
    g, origin, inject, flood, ref = _ref(4099, 100, 0.5, 11)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        out = pkg.loss.sweep(eng, [0.0, 0.5, 1.0], seed=11)
        assert eng.link_loss_info() == (True, 1.0, 11)
    assert [o["p"] for o in out] == [0.0, 0.5, 1.0]
    assert out[0]["rounds"] == flood["rounds"] and np.array_equal(out[0]["coverage"], flood["coverage"])
    assert out[1]["rounds"] == ref["rounds"] and np.array_equal(out[1]["coverage"], ref["coverage"])
    assert out[1]["reached"] == float(ref["coverage"].sum()) / (g.n * 100)
    assert out[2]["rounds"] == 3 and (out[2]["coverage"] == 1).all() and out[2]["reached"] == 100.0 / (g.n * 100)


# -- liveness -------------------------------------------------------------------
# (`sends` is left out: deg_live follows the seed's removals, the engine's
# unchanged removal path, which lossy_ref does not model; forwards likewise)

def test_crash_right_after_receipt(pkg, oracle):
    """20 vertices with a first receipt in round 2 crash in round 2: they never send it"""
    g, origin, inject, flood, plain = _ref(4099, 100, 0.25, 11)
    picked = np.nonzero((plain["first"] == 2).any(axis=1))[0][:20]
    assert picked.size == 20
    crashes = [(int(v), 2) for v in picked]
    ref = lossy_ref.run(g, origin, inject, p=0.25, seed=11, crash_at=load_ref.crash_rounds(g.n, 64, crashes))
    assert ref["rounds"] < 64 and (ref["first"][picked] == 2).any()
    assert not np.array_equal(ref["first"], plain["first"])
    with lossy(pkg, g, origin, inject, 0.25, 11) as eng:
        check_lossy(eng, run(eng, inject, crashes), ref, LIVE_KEYS, forwards=False)


def test_churn(pkg, oracle):
    g, origin, inject, flood, plain = _ref(4099, 100, 0.25, 11)
    crash_at = load_ref.crash_rounds(g.n, 64, churn=True, p_fail=0.01, churn_seed=5)
    ref = lossy_ref.run(g, origin, inject, p=0.25, seed=11, crash_at=crash_at)
    assert ref["rounds"] < 64 and sum(s["crashed"] for s in ref["stats"]) > 100
    assert not np.array_equal(ref["first"], plain["first"])
    with lossy(pkg, g, origin, inject, 0.25, 11, churn=1, p_fail=0.01, churn_seed=5) as eng:
        check_lossy(eng, run(eng, inject), ref, LIVE_KEYS, forwards=False)


# -- records that survive ---------------------------------------------------------

@pytest.mark.parametrize("fwd", [0, 1], ids=["plain", "msg-forwards"])
@pytest.mark.parametrize("m", [100, 1000])
def test_records_of_the_receivers_rows(pkg, oracle, m, fwd):
    """track_curve, track_delay, track_delay_dist read only the receivers' new
    rows: exact for the lossy run"""
    g, origin, inject, flood, ref = _ref(4099, m, 0.5, 11)
    with lossy(pkg, g, origin, inject, 0.5, 11, ("track_curve", "track_delay", "track_delay_dist"),
               track_msg_forwards=fwd) as eng:
        stats = run(eng, inject)
        assert np.array_equal(eng.curve(), histogram(ref["first"], ref["rounds"] + 1))
        d = delay_ref.totals(ref, inject)
        assert np.array_equal(eng.delay_sum().astype(np.int64), d["sum"])
        assert np.array_equal(eng.delay_max().astype(np.int64), d["max"])
        assert np.array_equal(eng.delay_dist().astype(np.int64), delay_dist_ref.totals(ref, inject)["dist"])
        check_lossy(eng, stats, ref)


# -- refusals ---------------------------------------------------------------------

def test_refusals(pkg, oracle):
    g, origin, inject, flood, ref = _ref(4099, 100, 0.5, 11)
    lib = pkg._lib
    with pkg.GossipEngine(0, track_first=1) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.link_loss(0.5, 11)
        for bad in (-0.01, 1.01, float("nan")):
            assert _status(pkg, lambda: eng.link_loss(bad, 3)) == lib.GP_EINVAL
        for name, on, off in (("track_load", eng.track_load, lambda: eng.track_load(False)),
                              ("track_fresh", eng.track_fresh, lambda: eng.track_fresh(False)),
                              ("track_fresh_curve", eng.track_fresh_curve, lambda: eng.track_fresh_curve(False)),
                              ("track_link_fresh", eng.track_link_fresh, lambda: eng.track_link_fresh(False)),
                              ("track_mult", eng.track_mult, lambda: eng.track_mult(False)),
                              ("watch", lambda: eng.watch([1, 2]), lambda: eng.watch([]))):
            on()
            with pytest.raises(pkg.GossipError) as e:
                eng.reset()
            assert e.value.status == lib.GP_EINVAL and name in str(e.value), (name, str(e.value))
            off()
        eng.reset()   # the bad p's left the request as it was
        assert eng.link_loss_info() == (True, 0.5, 11)
        check_lossy(eng, run(eng, inject), ref)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.link_loss(0.5, 11)
        assert _status(pkg, eng.reset) == lib.GP_EINVAL
        eng.link_loss(None)
        eng.reset()


# -- checkpoint -------------------------------------------------------------------

def test_checkpoint(pkg, oracle):
    g, origin, inject, flood, ref = _ref(4099, 1000, 0.5, 11)
    with lossy(pkg, g, origin, inject, 0.5, 11) as eng:
        head = [eng.round() for _ in range(3)]
        blob = eng.checkpoint()
    with lossy(pkg, g, origin, inject, 0.5, 11) as eng:
        eng.restore(blob)
        stats = head + eng.run()
        check_lossy(eng, stats, ref)
