"""Delayed links (csrc/delayed.hip) up to the 254-round ceiling, at every dmax,
and stopped mid-flight -- on the GPU.

test_gpu_link_delay.py runs to quiescence in a few dozen rounds at dmax in
{1, 2, 4, 8}.  Here the three overlays of long_shapes.py are still being
flooded when the ceiling cuts the run, so the ring of dmax + 1 frontier-row
buffers has wrapped 28 to 84 times, the guard row r % dmax and the ring slot
s % (dmax + 1) have gone through every combination (dmax 3, 5, 6, 7 too), a
round-253 receiver with loss on draws with the keys of send rounds 246 .. 253,
the run ends with dmax - 1 send rounds in flight, and forwards() is read from
runs that are not quiescent.

Every comparison is exact and against tests/delayed_ref.py (pinned at the
ceiling by test_delayed_long_ref.py) or, at dmax = 1, the C oracle -- never
against the engine's own output, except where a case says "identical to the
first run".  What makes a case late is asserted on the reference alone before
the engine is touched, and printed (test_delayed_long_ref.lateness).

  a  every dmax to the ceiling            g  records that survive, late
  b  every row width                      h  loss with delay, late
  c  dmax = 1 to the ceiling              i  crashes late, lines in flight
  d  hubs late                            j  tuning fields change nothing
  e  the ceiling itself                   k  lifecycle across long runs
  f  forwards of a run that is not quiescent
"""
import functools

import numpy as np
import pytest

import delay_dist_ref
import delay_ref
import delayed_ref
import long_shapes as ls
import lossy_ref
from test_delayed_long_ref import R, SEED, case, dref, hub_commits, in_flight, last_round_messages, lateness
from test_gpu_curve import MODE_IDS, MODES, check_run, histogram, mode_cfg
from test_gpu_link_delay import KEYS, LIVE_KEYS, check_delayed, check_flood, delayed, outputs, run, same
from test_gpu_long_runs import _ref as oracle_ref, status

pytestmark = pytest.mark.gpu

SHAPES = ("path", "far_hubs", "thick_ring")
RECORDS = ("track_curve", "track_delay", "track_delay_dist")
LOSS_SEED = 11
CHURN = (0.0002, 3)   # 25 crashes past round 128 on thick_ring, the run still cut at 254 (asserted below)


def to_the_ceiling(eng, stats, ref, dmax, **kw):
    """a run the ceiling cut: R rounds, dmax - 1 send rounds still in flight"""
    assert len(stats) == R
    assert eng.link_delay_info()[3] == dmax - 1 == in_flight(ref, dmax)
    check_delayed(eng, stats, ref, **kw)


# -- a. every dmax to the ceiling ---------------------------------------------------

@pytest.mark.parametrize("dmax", range(2, 9))
@pytest.mark.parametrize("shape", SHAPES)
def test_every_dmax_to_the_ceiling(pkg, shape, dmax):
    g, origin, inject = case(shape, "late", 100)
    ref = dref(shape, "late", 100, dmax)
    lateness(f"a {shape} late m=100", ref, dmax)
    assert last_round_messages(g, origin, inject, ref, dmax) > 0
    with delayed(pkg, g, origin, inject, dmax, SEED) as eng:
        assert eng.words == 2 and eng.link_delay_info() == (True, dmax, SEED, 0)
        to_the_ceiling(eng, run(eng, inject), ref, dmax)


# -- b. every row width ---------------------------------------------------------------

WIDTHS = ([("path", d, m) for d in (3, 8) for m in (64, 200, 1000, 4096)] +
          [("thick_ring", 3, m) for m in (200, 1000)])


@pytest.mark.parametrize("shape,dmax,m", WIDTHS, ids=[f"{s}-{d}-{m}" for s, d, m in WIDTHS])
def test_every_row_width(pkg, shape, dmax, m):
    g, origin, inject = case(shape, "late", m)
    ref = dref(shape, "late", m, dmax)
    lateness(f"b {shape} late m={m}", ref, dmax)
    with delayed(pkg, g, origin, inject, dmax, SEED) as eng:
        assert eng.words == {**ls.WORDS, 64: 1}[m]
        to_the_ceiling(eng, run(eng, inject), ref, dmax)


# -- c. dmax = 1 to the ceiling ---------------------------------------------------------

ONE_ROUND = [("path", 4096), ("far_hubs", 4096), ("far_hubs", 64), ("thick_ring", 4096)]


@pytest.mark.parametrize("shape,hub", ONE_ROUND, ids=[f"{s}-hub{h}" for s, h in ONE_ROUND])
def test_one_round_links_to_the_ceiling(pkg, oracle, shape, hub):
    """k_expand_delayed / k_hub_delayed through a ring of two, against the
    oracle's cut run (its forwards leave out the receivers of round 253)"""
    g, origin, inject, _, ref = oracle_ref(shape, "late", 100)
    late, last, never = ls.late_counts(ref["first"])
    print(f"c {shape} late m=100 dmax=1: rounds={ref['rounds']} cells>=128: {late} cells==254: {last} never: {never}")
    assert ref["rounds"] == R and late > 0 and last > 0 and never > 0
    if hub == 64:
        assert (np.diff(np.asarray(g.row_ptr, np.int64)) > hub).sum() == 2
    with delayed(pkg, g, origin, inject, 1, SEED, hub_threshold=hub) as eng:
        stats = run(eng, inject)
        assert len(stats) == R and eng.link_delay_info() == (True, 1, SEED, 0)
        check_flood(eng, stats, ref)


# -- d. hubs late -------------------------------------------------------------------------

@pytest.mark.parametrize("kind,m", [("ends", 1000), ("late", 100)])
@pytest.mark.parametrize("dmax", [2, 4])
def test_hubs_late(pkg, dmax, kind, m):
    """hub_threshold=64: vertices 130 and 250 (in-degree 102) go through
    k_hub_delayed's items and the push's tail, each in several rounds"""
    g, origin, inject = case("far_hubs", kind, m)
    ref = dref("far_hubs", kind, m, dmax)
    lateness(f"d far_hubs {kind} m={m}", ref, dmax)
    a, b = hub_commits(ref, origin, inject, 130), hub_commits(ref, origin, inject, 250)
    print(f"d far_hubs {kind} m={m} dmax={dmax}: hub 130 commits in rounds {a}, hub 250 in rounds {b}")
    assert len(b) >= 3 and (dmax > 2 or len(a) >= 3)
    with delayed(pkg, g, origin, inject, dmax, SEED, hub_threshold=64) as eng:
        to_the_ceiling(eng, run(eng, inject), ref, dmax)


# -- e. the ceiling itself ------------------------------------------------------------------

READS = ("first", "seen", "seenpop", "digest", "coverage", "forwards", "curve", "link_delay_info")


@pytest.mark.parametrize("shape,dmax,hub", [("far_hubs", 2, 64), ("thick_ring", 7, 4096), ("path", 8, 4096)])
def test_the_ceiling(pkg, shape, dmax, hub):
    g, origin, inject = case(shape, "late", 100)
    ref = dref(shape, "late", 100, dmax)
    lateness(f"e {shape} late m=100", ref, dmax)
    lib = pkg._lib
    with delayed(pkg, g, origin, inject, dmax, SEED, track=("track_curve",), hub_threshold=hub) as eng:
        stats = run(eng, inject)
        to_the_ceiling(eng, stats, ref, dmax)
        first_run = outputs(eng, stats)
        before = {k: getattr(eng, k)() for k in READS}
        assert {254, 255} <= set(np.unique(before["first"]).tolist())
        assert np.array_equal(before["curve"], histogram(ref["first"], R + 1))
        for _ in range(2):                                  # round 254 is refused, twice over ...
            assert status(pkg, eng.round) == lib.GP_ESTATE
            assert status(pkg, eng.run) == lib.GP_ESTATE    # ... through gp_run too
        assert eng.link_delay_info()[3] == dmax - 1         # the lines are still under way
        for k in READS:                                     # and nothing was touched
            assert np.array_equal(getattr(eng, k)(), before[k]), k
        eng.reset()
        assert eng.link_delay_info() == (True, dmax, SEED, 0)
        stats = eng.run()                                   # gp_run from a fresh reset: 254 rounds, no error
        assert [s["round"] for s in stats] == list(range(R))
        to_the_ceiling(eng, stats, ref, dmax)
        eng.reset()
        again = run(eng, inject)
        assert same(first_run, outputs(eng, again))         # identical to the first run
        for k in READS:
            assert np.array_equal(getattr(eng, k)(), before[k]), k


# -- f. forwards of a delayed run that is not quiescent ---------------------------------------

def stops(ref, dmax):
    """the cuts k of a case, from the reference alone: (busy, quiet) -- round
    k - 1 made new bits (finalize takes the receivers' unsent share off), or
    made none while lines are in flight (nothing may come off)"""
    nb = [s["new_bits"] for s in ref["stats"]]
    busy = [k for k in (1, 100, 128, 129, 200, 253) if nb[k - 1] > 0]
    quiet = [k for k in range(1, R) if nb[k - 1] == 0 and in_flight(ref, dmax, k) > 0]
    return busy[-3:], sorted(set(quiet[:1] + quiet[-2:]))


def check_counts(eng, stats, ref):
    """what a context without track_first still gives"""
    assert len(stats) == ref["rounds"]
    for a, b in zip(stats, ref["stats"]):
        for k in KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    assert np.array_equal(eng.seenpop().astype(np.int64), ref["seenpop"])
    eng.finalize()
    assert np.array_equal(eng.coverage(), ref["coverage"])
    assert np.array_equal(eng.forwards(), ref["forwards"])


MIDFLIGHT = [("path", 4, "late", 2, 2), ("thick_ring", 3, "late", 2, 0), ("thick_ring", 8, "late", 2, 0),
             ("thick_ring", 3, "uniform", 2, 2), ("thick_ring", 8, "uniform", 2, 2)]


@pytest.mark.parametrize("variant", ["seen-rows", "msg-forwards", "no-first"])
@pytest.mark.parametrize("shape,dmax,kind,nbusy,nquiet", MIDFLIGHT, ids=[f"{s}-{d}-{k}" for s, d, k, _, _ in MIDFLIGHT])
def test_forwards_mid_flight(pkg, shape, dmax, kind, nbusy, nquiet, variant):
    """finalize() after k rounds, k from the reference: forwards() counts the
    send rounds <= k - 1 -- by the Message-Lists minus d_frx[cur] x deg_live
    where round k - 1 made new bits (d_frx[cur] is the ring's slot of round k),
    by the Message-Lists alone where it made none, and by the per-round pass
    with track_msg_forwards.  The run then goes on: a finalize changes nothing.
    (thick_ring x late has no quiet round with lines in flight: the table
    `uniform` gives them.)"""
    g, origin, inject = case(shape, kind, 100)
    ref = dref(shape, kind, 100, dmax)
    busy, quiet = stops(ref, dmax)
    print(f"f {shape} {kind} dmax={dmax}: rounds={ref['rounds']} cuts with new bits in round k - 1: {busy}, "
          f"with none and lines in flight: {quiet} (in flight {[in_flight(ref, dmax, k) for k in quiet]}), and {R}; "
          f"in flight at the cut: {in_flight(ref, dmax)}")
    assert ref["rounds"] == R and in_flight(ref, dmax) > 0
    assert len(busy) >= nbusy and len(quiet) >= nquiet
    cfg = {"seen-rows": {}, "msg-forwards": dict(track_msg_forwards=1), "no-first": dict(track_first=0)}[variant]
    check = check_counts if variant == "no-first" else check_delayed
    with delayed(pkg, g, origin, inject, dmax, SEED, **cfg) as eng:
        stats = []
        for k in sorted(busy + quiet):
            cut = dref(shape, kind, 100, dmax, max_rounds=k)
            assert cut["rounds"] == k and (cut["stats"][-1]["new_bits"] > 0) == (k in busy)
            stats += [eng.round() for _ in range(len(stats), k)]
            assert eng.link_delay_info()[3] == in_flight(cut, dmax) > 0
            assert status(pkg, lambda: (eng.finalize(), eng.forwards())) == 0   # never GP_ENOTRACK: the rows are kept
            check(eng, stats, cut)
        stats += [eng.round() for _ in range(len(stats), R)]
        assert status(pkg, eng.round) == pkg._lib.GP_ESTATE
        check(eng, stats, ref)


# -- g. records that survive, late --------------------------------------------------------------

@pytest.mark.parametrize("dmax", [3, 8])
@pytest.mark.parametrize("shape", ["thick_ring", "far_hubs"])
def test_records_late(pkg, shape, dmax):
    g, origin, inject = case(shape, "late", 100)
    ref = dref(shape, "late", 100, dmax)
    lateness(f"g {shape} late m=100", ref, dmax)
    d = delay_ref.totals(ref, inject)
    dist = delay_dist_ref.totals(ref, inject)["dist"]
    print(f"g {shape} dmax={dmax}: delay_max={int(d['max'].max())} receipts in the saturated column: "
          f"{int(dist[:, -1].sum())}")
    # (far_hubs at dmax = 8: 252, no message is slow and old enough to be heard first in round 254)
    assert int(d["max"].max()) == R if shape == "thick_ring" or dmax <= 4 else int(d["max"].max()) >= 128
    assert dist.shape[1] == 16 and int(dist[:, -1].sum()) > 0
    with delayed(pkg, g, origin, inject, dmax, SEED, track=RECORDS, hub_threshold=64) as eng:
        stats = run(eng, inject)
        curve = eng.curve()
        assert curve.shape == (R + 1, 100) and np.array_equal(curve, histogram(ref["first"], R + 1))
        assert np.array_equal(eng.delay_sum().astype(np.int64), d["sum"])
        assert np.array_equal(eng.delay_max().astype(np.int64), d["max"])
        assert np.array_equal(eng.delay_dist().astype(np.int64), dist)
        to_the_ceiling(eng, stats, ref, dmax)


# -- h. loss with delay, late ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loss_only(p):
    g, origin, inject = case("thick_ring", "late", 100)
    return lossy_ref.run(g, origin, inject, p=p, seed=LOSS_SEED)


@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("dmax", [3, 4, 8])
def test_loss_with_delay_late(pkg, dmax, p):
    """a receiver of round 253 draws with the keys of send rounds 254 - dmax .. 253.
    Loss seed 11; measured on the reference at p = 0.3: 594 / 540 / 1291 cells
    >= 128 and 60 / 49 / 36 cells of 254 at dmax 3 / 4 / 8."""
    g, origin, inject = case("thick_ring", "late", 100)
    ref = dref("thick_ring", "late", 100, dmax, p, LOSS_SEED)
    late, last, _ = lateness(f"h thick_ring late m=100 p={p}", ref, dmax)
    assert late > 0 and last > 0
    for tag, other in (("loss-only", _loss_only(p)), ("delay-only", dref("thick_ring", "late", 100, dmax))):
        differ = (ref["first"] != other["first"]) & ((ref["first"] >= 128) | (other["first"] >= 128))
        print(f"h dmax={dmax} p={p}: {int(differ.sum())} cells at rounds >= 128 differ from the {tag} run's")
        assert differ.any()
    with delayed(pkg, g, origin, inject, dmax, SEED, p=p, loss_seed=LOSS_SEED) as eng:
        assert eng.link_loss_info() == (True, p, LOSS_SEED)
        to_the_ceiling(eng, run(eng, inject), ref, dmax)


def test_every_arc_closed_to_the_ceiling(pkg):
    g, origin, inject = case("thick_ring", "late", 100)
    ref = dref("thick_ring", "late", 100, 4, 1.0, 5)
    assert ref["rounds"] == R and sum(s["new_bits"] for s in ref["stats"]) == 0 and in_flight(ref, 4) == 3
    with delayed(pkg, g, origin, inject, 4, SEED, p=1.0, loss_seed=5) as eng:
        stats = run(eng, inject)
        assert all(s["new_bits"] == 0 for s in stats) and sum(s["rows_gathered"] for s in stats) == 0
        to_the_ceiling(eng, stats, ref, 4)
        assert (eng.coverage() == 1).all()


# -- i. crashes late with lines in flight -----------------------------------------------------------
# (keys LIVE_KEYS, forwards off: as test_gpu_link_delay.py's liveness cases)

CRASH_S = 200


@functools.lru_cache(maxsize=None)
def _picked():
    """20 vertices of the ring with a first receipt in round CRASH_S, no two within reach of each other"""
    g, _, _ = case("thick_ring", "late", 100)
    plain = dref("thick_ring", "late", 100, 4)
    picked = []
    for v in np.nonzero((plain["first"] == CRASH_S).any(axis=1))[0].tolist():
        if all(min((v - u) % g.n, (u - v) % g.n) > 4 for u in picked):
            picked.append(v)
    assert len(picked) >= 20
    return tuple(picked[:20])


def test_crash_late_with_lines_in_flight(pkg):
    """they crash in round 202: what they sent in round 200 over links of 3 or
    4 rounds arrives after they are gone"""
    g, origin, inject = case("thick_ring", "late", 100)
    plain = dref("thick_ring", "late", 100, 4)
    picked = _picked()
    crashes = tuple((v, CRASH_S + 2) for v in picked)
    ref = dref("thick_ring", "late", 100, 4, crashes=crashes)
    lateness("i thick_ring late m=100 crashes in 202", ref, 4, every_delay=False)
    assert ref["stats"][CRASH_S + 2]["crashed"] == 20 and not np.array_equal(ref["first"], plain["first"])
    delay = delayed_ref.arc_delays(g, 4, SEED)
    dst = np.repeat(np.arange(g.n), np.diff(g.row_ptr))
    late = [j for j in np.nonzero(np.isin(g.col, picked) & (delay >= 3))[0]
            if ((ref["first"][g.col[j]] == CRASH_S) & (ref["first"][dst[j]] == CRASH_S + delay[j])).any()]
    print(f"i: {len(late)} arcs carry a line of round {CRASH_S} that is a first receipt after its sender's crash")
    assert late
    with delayed(pkg, g, origin, inject, 4, SEED) as eng:
        to_the_ceiling(eng, run(eng, inject, crashes), ref, 4, keys=LIVE_KEYS, forwards=False)


def test_crash_late_right_after_receipt(pkg):
    """the same 20 crash in round 200: they never send"""
    g, origin, inject = case("thick_ring", "late", 100)
    plain = dref("thick_ring", "late", 100, 4)
    picked = _picked()
    crashes = tuple((v, CRASH_S) for v in picked)
    ref = dref("thick_ring", "late", 100, 4, crashes=crashes)
    lateness("i thick_ring late m=100 crashes in 200", ref, 4, every_delay=False)
    assert (ref["first"][list(picked)] == CRASH_S).any()
    assert ref["stats"][CRASH_S]["active"] == plain["stats"][CRASH_S]["active"] - 20
    with delayed(pkg, g, origin, inject, 4, SEED) as eng:
        to_the_ceiling(eng, run(eng, inject, crashes), ref, 4, keys=LIVE_KEYS, forwards=False)


def test_churn_late(pkg):
    g, origin, inject = case("thick_ring", "late", 100)
    plain = dref("thick_ring", "late", 100, 4)
    ref = dref("thick_ring", "late", 100, 4, churn=CHURN)
    lateness(f"i thick_ring late m=100 churn p_fail={CHURN[0]}", ref, 4, every_delay=False)
    crashed = sum(s["crashed"] for s in ref["stats"][128:])
    print(f"i: {crashed} crashes past round 128, {sum(s['crashed'] for s in ref['stats'])} in all")
    assert crashed >= 20 and not np.array_equal(ref["first"], plain["first"])
    with delayed(pkg, g, origin, inject, 4, SEED, churn=1, p_fail=CHURN[0], churn_seed=CHURN[1]) as eng:
        to_the_ceiling(eng, run(eng, inject), ref, 4, keys=LIVE_KEYS, forwards=False)


# -- j. tuning fields change nothing --------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_tuning_fields_change_nothing(pkg, mode):
    g, origin, inject = case("thick_ring", "late", 100)
    ref = dref("thick_ring", "late", 100, 3)
    lateness("j thick_ring late m=100", ref, 3)
    with delayed(pkg, g, origin, inject, 3, SEED, **mode_cfg(mode)) as eng:
        to_the_ceiling(eng, run(eng, inject), ref, 3)


# -- k. lifecycle across long runs ------------------------------------------------------------------------

def test_lifecycle_across_long_runs(pkg, oracle):
    """one engine: the ring of nine, then of four (reallocated, with whatever
    round 253 left in the slots), then released for the planner's flood"""
    g, origin, inject, _, flood = oracle_ref("thick_ring", "late", 100)
    ref8, ref3 = dref("thick_ring", "late", 100, 8), dref("thick_ring", "late", 100, 3)
    lateness("k thick_ring late m=100", ref8, 8)
    lateness("k thick_ring late m=100", ref3, 3)
    assert flood["rounds"] == R and not np.array_equal(ref8["first"], ref3["first"])
    with delayed(pkg, g, origin, inject, 8, SEED) as eng:
        to_the_ceiling(eng, run(eng, inject), ref8, 8)
        eng.link_delay(3, SEED)
        assert eng.link_delay_info() == (True, 8, SEED, 7)   # nothing changes before the reset
        eng.reset()
        assert eng.link_delay_info() == (True, 3, SEED, 0)
        to_the_ceiling(eng, run(eng, inject), ref3, 3)
        eng.link_delay(None)
        eng.reset()
        assert eng.link_delay_info() == (False, 1, 0, 0)
        stats = eng.run()
        assert len(stats) == R and all(s["mode"] in (0, 1) for s in stats)
        check_run(eng, stats, flood)
        assert np.array_equal(eng.first(), flood["first"])
