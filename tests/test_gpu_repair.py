"""Anti-entropy repair (csrc/repair.hip, gp_repair) on
the GPU.

In a repair round every up peer pulls the whole Message-List of one drawn
in-neighbour over that link, if the round's loss draw leaves it open; what it
brings is a first receipt like any other.  Two references, neither of them the
engine:
 - without loss (or with p = 0) repair changes no first receipt, so
   k_repair_offer / k_expand_repair must give the C oracle's flood (oracle.run)
   bit for bit, while the repair record -- exchanges and lines per round -- is
   the numpy reference's and is not empty;
 - with p = 0.5 the numpy round loop of tests/repair_ref.py (pinned by
   tests/test_repair_ref.py): first-receipt matrix, seenpop, the per-round
   counters, the repair record, coverage and forwards, all exact.
Every lossy case with m >= 64 first asserts, on the reference alone, that
repair changed at least 0.15 of the first-receipt cells against the lossy run
without it: a kernel that dropped the offers could not pass.

Shapes are test_gpu_link_loss.py's: 4,099 vertices (no multiple of a wave's 64)
and 5 (fewer than one wave), every row width with partial last words, hubs
split over the hub table (hub_threshold=64), a directed overlay, a raw CSR with
self-loops and repeated arcs.  Lossy runs are stepped for at most 48 rounds.
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
import repair_cases as rc
import repair_ref
from test_gpu_curve import MODE_IDS, MODES, check_run, histogram, mode_cfg, run
from test_gpu_delay import WIDTH_MS, WORDS
from test_gpu_fresh import _status
from test_gpu_link_loss import KEYS, LIVE_KEYS, check_flood

pytestmark = pytest.mark.gpu

RSEED = rc.RSEED


def repairing(pkg, g, origin, inject, period, rseed=RSEED, p=None, seed=0, track=(), **cfg):
    cfg.setdefault("track_first", 1)
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    if p is not None:
        eng.link_loss(p, seed)
    eng.repair(period, rseed)
    for t in track:
        getattr(eng, t)()
    eng.reset()
    return eng


def step(eng, period, max_rounds=rc.CUT, crashes=()):
    """round() until `period` silent rounds (repair_info's quiet), max_rounds at most"""
    by_round = {}
    for v, r in crashes:
        by_round.setdefault(r, []).append(v)
    stats = []
    for r in range(max_rounds):
        if r in by_round:
            eng.crash(by_round[r])
        stats.append(eng.round())
        if eng.repair_info()[3] >= period:
            break
    return stats


def check_repair(eng, stats, ref, keys=KEYS, forwards=True):
    """a run with repair against repair_ref.run's result: all exact"""
    assert all(s["mode"] == 2 and s["scan"] == 0 for s in stats)
    assert len(stats) == ref["rounds"], (len(stats), ref["rounds"])
    for a, b in zip(stats, ref["stats"]):
        for k in keys:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    rec = eng.repair_record()
    assert rec.dtype == np.uint64 and rec.shape == ref["repair"].shape
    bad = np.argwhere(rec != ref["repair"])
    assert bad.size == 0, (bad[:8], rec[bad[:8, 0]], ref["repair"][bad[:8, 0]])
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
            eng.forwards(), eng.repair_record())


def same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# -- 1. repair over open arcs is the oracle's flood -------------------------------

@functools.lru_cache(maxsize=None)
def _open_ref(n, m):
    g, origin, inject, _ = rc.table(n, m)
    return repair_ref.run(g, origin, inject, p=0.0, period=1, rseed=RSEED)


def check_open(eng, stats, flood, rref):
    check_flood(eng, stats, flood)
    rec = eng.repair_record()
    assert np.array_equal(rec, rref["repair"])
    assert np.array_equal(rref["first"], flood["first"])


@pytest.mark.parametrize("loss", [None, 0.0], ids=["alone", "p0"])
@pytest.mark.parametrize("m", WIDTH_MS)
@pytest.mark.parametrize("n", [4099, 5])
def test_open_arcs_are_the_oracles_flood(pkg, oracle, n, m, loss):
    g, origin, inject, flood = rc.table(n, m)
    rref = _open_ref(n, m)
    assert rref["repair"][:, 1].sum() > 0 or m == 1
    with repairing(pkg, g, origin, inject, 1, p=loss) as eng:
        assert eng.info()[3] == WORDS[m] and eng.repair_info() == (True, 1, RSEED, 0)
        assert eng.link_loss_info() == ((True, 0.0, 0) if loss is not None else (False, 0.0, 0))
        check_open(eng, run(eng, inject), flood, rref)
        assert eng.repair_info()[3] == 1


@pytest.mark.parametrize("m", WIDTH_MS)
def test_open_arcs_hubs(pkg, oracle, m):
    """hub_threshold=64: 44 receivers take their offers through tbits, k_hub_lossy and the push's receiver side"""
    g, origin, inject, flood = rc.table(4099, m)
    assert (np.diff(g.row_ptr) > 64).sum() == 44
    with repairing(pkg, g, origin, inject, 1, hub_threshold=64) as eng:
        check_open(eng, run(eng, inject), flood, _open_ref(4099, m))


@pytest.mark.parametrize("hub_threshold", [4096, 64])
@pytest.mark.parametrize("m", [100, 4096])
def test_open_arcs_directed(pkg, oracle, m, hub_threshold):
    g = ds.oriented_chung_lu(pkg, oracle, 4099, 8, 2.2, 7, "coin")
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 3).astype(np.int32)
    flood = ds.CachedOracle(oracle).run(g, origin, inject, want_first=True)
    rref = repair_ref.run(g, origin, inject, p=0.0, period=1, rseed=RSEED)
    assert rref["repair"][:, 1].sum() > 0 and (rref["repair"][:, 0] < g.n).all()   # (some vertices have no in-arc)
    with repairing(pkg, g, origin, inject, 1, hub_threshold=hub_threshold) as eng:
        check_open(eng, run(eng, inject), flood, rref)


@pytest.mark.parametrize("m", [100, 4096])
def test_open_arcs_raw_csr(pkg, oracle, m):
    """self-loops and repeated arcs: a self-loop partner is an exchange that offers nothing"""
    g = raw_csr.loops_and_repeats(pkg)
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 3).astype(np.int32)
    flood = oracle.run(g, origin, inject, want_first=True)
    rref = repair_ref.run(g, origin, inject, p=0.0, period=1, rseed=RSEED)
    pr = repair_ref.partners(g, RSEED, 0)
    assert (pr == np.arange(g.n)).sum() >= 5 and rref["repair"][:, 1].sum() > 0
    with repairing(pkg, g, origin, inject, 1) as eng:
        check_open(eng, run(eng, inject), flood, rref)
    lref = repair_ref.run(g, origin, inject, p=0.5, seed=11, period=1, rseed=RSEED, max_rounds=rc.CUT)
    assert rc.changed_share(lref, lossy_ref.run(g, origin, inject, p=0.5, seed=11)) >= rc.MIN_SHARE
    with repairing(pkg, g, origin, inject, 1, p=0.5, seed=11) as eng:
        check_repair(eng, step(eng, 1), lref)


# -- 2. lossy repair against the reference ------------------------------------------

def _lossy_case(n, m, period):
    ref = rc.repaired(n, m, period)
    if n == 4099 and m >= 64:
        share = rc.changed_share(ref, rc.plain(n, m))
        print(f"m={m} period={period}: {share:.3f} of the cells differ from the lossy run's, {ref['rounds']} rounds")
        assert share >= rc.MIN_SHARE
    return rc.table(n, m)[:3] + (ref,)


@pytest.mark.parametrize("period", rc.PERIODS)
@pytest.mark.parametrize("m", WIDTH_MS)
@pytest.mark.parametrize("n", [4099, 5])
def test_lossy_repair(pkg, oracle, n, m, period):
    g, origin, inject, ref = _lossy_case(n, m, period)
    with repairing(pkg, g, origin, inject, period, p=rc.P, seed=rc.SEED) as eng:
        assert eng.repair_info()[:3] == (True, period, RSEED) and eng.link_loss_info() == (True, rc.P, rc.SEED)
        check_repair(eng, step(eng, period), ref)
        if m == 64:   # the digest is still a pure function of the first-receipt matrix
            assert np.array_equal(eng.digest(), oracle.digest_from_first(ref["first"], origin))


@pytest.mark.parametrize("period", rc.PERIODS)
@pytest.mark.parametrize("m", [100, 4096])
def test_lossy_repair_hubs(pkg, oracle, m, period):
    g, origin, inject, ref = _lossy_case(4099, m, period)
    with repairing(pkg, g, origin, inject, period, p=rc.P, seed=rc.SEED, hub_threshold=64) as eng:
        check_repair(eng, step(eng, period), ref)


# -- 3. run() stops by the rule -----------------------------------------------------

@pytest.mark.parametrize("period", [1, 2])
def test_run_stops_by_the_rule(pkg, oracle, period):
    g, origin, inject, _ = rc.table(4099, 100)
    ref = rc.repaired(4099, 100, period, max_rounds=254)
    print(f"period={period}: {ref['rounds']} rounds")
    nb = [s["new_bits"] for s in ref["stats"]]
    assert ref["rounds"] < 254 and not any(nb[-period:]) and nb[-period - 1] > 0
    with repairing(pkg, g, origin, inject, period, p=rc.P, seed=rc.SEED) as eng:
        stats = eng.run()
        assert eng.repair_info()[3] == period
        check_repair(eng, stats, ref)


# -- 4. liveness ----------------------------------------------------------------------
# (`sends` and forwards are left out, as in test_gpu_link_loss.py)

def test_crashed_partners_and_receivers(pkg, oracle):
    """before the repair round 5, ten partners whose Message-List would have
    brought news go down, and ten receivers about to be repaired"""
    g, origin, inject, _ = rc.table(4099, 100)
    plain = rc.repaired(4099, 100, 1)
    r0 = 5
    held = plain["first"] <= r0
    pr = repair_ref.partners(g, RSEED, r0)
    v = np.arange(g.n)
    helped = np.nonzero(lossy_ref.arc_open(rc.SEED, r0, pr, v, rc.P) & (held[pr] & ~held).any(axis=1))[0]
    assert helped.size >= 40
    down_p, down_v = pr[helped[:10]], helped[10:20]
    crashes = [(int(x), r0) for x in np.concatenate([down_p, down_v])]
    crash_at = load_ref.crash_rounds(g.n, 64, crashes)
    ref = repair_ref.run(g, origin, inject, p=rc.P, seed=rc.SEED, period=1, rseed=RSEED, max_rounds=rc.CUT,
                         crash_at=crash_at)
    assert ref["repair"][r0, 0] < plain["repair"][r0, 0] and not np.array_equal(ref["first"], plain["first"])
    # (most of the twenty lose something for it; gossip of the same round may bring one of them the same bits)
    assert (ref["first"][helped[:20]] != plain["first"][helped[:20]]).any(axis=1).sum() >= 15
    with repairing(pkg, g, origin, inject, 1, p=rc.P, seed=rc.SEED) as eng:
        check_repair(eng, step(eng, 1, crashes=crashes), ref, LIVE_KEYS, forwards=False)


@pytest.mark.parametrize("period", [1, 3])
def test_churn(pkg, oracle, period):
    g, origin, inject, _ = rc.table(4099, 100)
    crash_at = load_ref.crash_rounds(g.n, 64, churn=True, p_fail=0.01, churn_seed=5)
    ref = repair_ref.run(g, origin, inject, p=rc.P, seed=rc.SEED, period=period, rseed=RSEED, max_rounds=rc.CUT,
                         crash_at=crash_at)
    assert sum(s["crashed"] for s in ref["stats"]) > 100
    assert not np.array_equal(ref["first"], rc.repaired(4099, 100, period)["first"])
    with repairing(pkg, g, origin, inject, period, p=rc.P, seed=rc.SEED, churn=1, p_fail=0.01, churn_seed=5) as eng:
        check_repair(eng, step(eng, period), ref, LIVE_KEYS, forwards=False)


# -- 5. blocks ------------------------------------------------------------------------

def test_message_blocks(pkg, oracle):
    """the partner draw does not see the message: two halves of the table give
    the whole run's columns, their lines add up, their exchanges are the run's"""
    g, origin, inject, ref = _lossy_case(4099, 4096, 1)
    R = ref["rounds"]
    cols, recs = [], []
    for k in range(2):
        with pkg.GossipEngine(0, track_first=1) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, k * 2048, (k + 1) * 2048)
            assert eng.words == 32
            eng.link_loss(rc.P, rc.SEED)
            eng.repair(1, RSEED)
            eng.reset()
            stats = [eng.round() for _ in range(R)]   # (the whole run's rounds, whatever the block's own silence)
            assert all(s["mode"] == 2 for s in stats)
            cols.append(eng.first())
            recs.append(eng.repair_record())
    assert np.array_equal(np.concatenate(cols, axis=1), ref["first"])
    assert np.array_equal(recs[0][:, 0], ref["repair"][:, 0]) and np.array_equal(recs[1][:, 0], ref["repair"][:, 0])
    assert np.array_equal(recs[0][:, 1] + recs[1][:, 1], ref["repair"][:, 1])


# -- 6. checkpoint ----------------------------------------------------------------------

def test_checkpoint(pkg, oracle):
    g, origin, inject, ref = _lossy_case(4099, 1000, 3)
    lib = pkg._lib
    with repairing(pkg, g, origin, inject, 3, p=rc.P, seed=rc.SEED) as eng:
        head = [eng.round() for _ in range(7)]
        blob = eng.checkpoint()
        whole = outputs(eng, head + step(eng, 3, rc.CUT - 7))
    with repairing(pkg, g, origin, inject, 3, p=rc.P, seed=rc.SEED) as eng:
        eng.restore(blob)
        assert eng.repair_info() == (True, 3, RSEED, 0)
        assert _status(pkg, eng.repair_record) == lib.GP_ESTATE
        stats = head + step(eng, 3, rc.CUT - 7)
        assert _status(pkg, eng.repair_record) == lib.GP_ESTATE
        assert len(stats) == ref["rounds"]
        assert np.array_equal(eng.first(), ref["first"])
        eng.finalize()
        got = ([tuple(s[k] for k in KEYS) for s in stats], eng.first(), eng.digest(), eng.seen(), eng.coverage(),
               eng.forwards())
        assert same(got, whole[:6])
        eng.reset()   # a new run keeps its record again
        eng.round()
        assert eng.repair_record().shape == (1, 2)


# -- 7. records that survive ---------------------------------------------------------------

@pytest.mark.parametrize("m", [100, 1000])
def test_records_of_the_receivers_rows(pkg, oracle, m):
    """track_curve, track_delay, track_delay_dist read only the receivers' new rows: exact under repair"""
    g, origin, inject, ref = _lossy_case(4099, m, 1)
    with repairing(pkg, g, origin, inject, 1, p=rc.P, seed=rc.SEED,
                   track=("track_curve", "track_delay", "track_delay_dist")) as eng:
        stats = step(eng, 1)
        assert np.array_equal(eng.curve(), histogram(ref["first"], ref["rounds"] + 1))
        d = delay_ref.totals(ref, inject)
        assert np.array_equal(eng.delay_sum().astype(np.int64), d["sum"])
        assert np.array_equal(eng.delay_max().astype(np.int64), d["max"])
        assert np.array_equal(eng.delay_dist().astype(np.int64), delay_dist_ref.totals(ref, inject)["dist"])
        check_repair(eng, stats, ref)


# -- 8. modes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("hub_threshold", [4096, 64])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [100, 4096])
def test_tuning_fields_change_nothing(pkg, oracle, m, mode, hub_threshold):
    g, origin, inject, ref = _lossy_case(4099, m, 3)
    with repairing(pkg, g, origin, inject, 3, p=rc.P, seed=rc.SEED, hub_threshold=hub_threshold,
                   **mode_cfg(mode)) as eng:
        check_repair(eng, step(eng, 3), ref)


# -- 9. refusals and info -------------------------------------------------------------------------

def test_refusals_and_info(pkg, oracle):
    g, origin, inject, _ = rc.table(4099, 100)
    ref, plain = rc.repaired(4099, 100, 3), rc.plain(4099, 100)
    lib = pkg._lib
    with pkg.GossipEngine(0, track_first=1) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        assert eng.repair_info() == (False, 1, 0, 0)
        eng.reset()
        assert _status(pkg, eng.repair_record) == lib.GP_ENOTRACK
        eng.link_loss(rc.P, rc.SEED)
        eng.repair(3, RSEED)
        assert eng.repair_info() == (False, 1, 0, 0)   # (the request takes effect at the reset)
        for bad in (0, -1, 65, 1000):
            assert _status(pkg, lambda: eng.repair(bad, 5)) == lib.GP_EINVAL
        for loss in (True, False):   # the arc-walking records are refused with or without loss
            eng.link_loss(rc.P if loss else None, rc.SEED)
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
                if not loss:
                    assert "repair" in str(e.value)
                off()
        eng.link_delay(2, 3)
        with pytest.raises(pkg.GossipError) as e:
            eng.reset()
        assert e.value.status == lib.GP_EINVAL and "gp_link_delay" in str(e.value) and "repair" in str(e.value)
        eng.link_delay(None)
        assert eng.repair_info() == (False, 1, 0, 0) and eng.link_loss_info() == (False, 0.0, 0)   # nothing changed
        eng.link_loss(rc.P, rc.SEED)
        eng.reset()   # the bad periods left the request as it was
        assert eng.repair_info() == (True, 3, RSEED, 0)
        stats = step(eng, 3)
        check_repair(eng, stats, ref)
        a = outputs(eng, stats)
        eng.reset()   # the same setting twice: identical
        assert same(a, outputs(eng, step(eng, 3)))
        eng.repair(3, RSEED + 1)   # another seed differs
        eng.reset()
        assert not same(a, outputs(eng, step(eng, 3)))
        eng.repair(None)   # back to the plain lossy run
        eng.round()
        assert eng.repair_info()[:3] == (True, 3, RSEED + 1)   # (a setting made mid-run changes nothing before the reset)
        eng.reset()
        assert eng.repair_info() == (False, 1, 0, 0)
        assert _status(pkg, eng.repair_record) == lib.GP_ENOTRACK
        stats = run(eng, inject)
        assert len(stats) == plain["rounds"] and np.array_equal(eng.first(), plain["first"])
    with pkg.GossipEngine(0) as eng:   # a vertex partition
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.repair(1, RSEED)
        with pytest.raises(pkg.GossipError) as e:
            eng.reset()
        assert e.value.status == lib.GP_EINVAL and "partition" in str(e.value)
        eng.repair(None)
        eng.reset()


def test_shard_job_is_refused(pkg, oracle):
    """in a message-shard job: by name at the reset; a transport joined after the reset, at the top of the round"""
    g, origin, inject, _ = rc.table(4099, 100)
    lib = pkg._lib
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.repair(1, RSEED)
        eng.reset()
        eng.round()
        eng.shard_host_init(lambda b: [b], 1, 0)
        with pytest.raises(pkg.GossipError) as e:
            eng.round()
        assert e.value.status == lib.GP_ESTATE and "shard" in str(e.value)
        with pytest.raises(pkg.GossipError) as e:
            eng.reset()
        assert e.value.status == lib.GP_EINVAL and "gp_shard_" in str(e.value)
        eng.repair(None)
        eng.reset()
        eng.run()


def test_sweep(pkg, oracle):
    """repair.sweep: one reset and run per period, on top of the loss setting"""
    g, origin, inject, _ = rc.table(4099, 100)
    plain = rc.plain(4099, 100)
    r1, r2 = rc.repaired(4099, 100, 1, max_rounds=254), rc.repaired(4099, 100, 2, max_rounds=254)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.link_loss(rc.P, rc.SEED)
        out = pkg.repair.sweep(eng, [None, 1, 2], seed=RSEED)
        assert eng.repair_info()[:3] == (True, 2, RSEED)
    assert [o["period"] for o in out] == [0, 1, 2]
    for o, ref in zip(out, (plain, r1, r2)):
        assert o["rounds"] == ref["rounds"] and np.array_equal(o["coverage"], ref["coverage"])
        assert o["reached"] == float(ref["coverage"].sum()) / (g.n * 100)
    assert (out[0]["exchanges"], out[0]["lines"]) == (0, 0)
    for o, ref in zip(out[1:], (r1, r2)):
        assert (o["exchanges"], o["lines"]) == tuple(int(x) for x in ref["repair"].sum(axis=0))
    assert out[1]["reached"] > out[0]["reached"] + 0.15
