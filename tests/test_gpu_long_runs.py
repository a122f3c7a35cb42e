"""Floods and every record up to the 254-round ceiling, on the GPU.

The engine is built for runs of up to 254 rounds: a receipt round is a u8 with
255 = never, gp_round refuses round 254, inject rounds go up to 253, the curves
have 255 rows, delay_max reaches 254, the crash and loss streams run to round
253.  The power-law overlays of the other files are flooded in about ten
rounds; the three overlays of long_shapes.py (a path, a path with two far hubs,
a thick ring) are still being flooded when the ceiling cuts the run, so every
byte value up to 254 occurs beside the sentinel, and the planner's late
switches, the hub commits, crashes, removals, closed arcs and injections all
happen at rounds past 128 and in the last rounds.

Every comparison is an exact integer comparison against the oracle's run
(oracle.run, lossy_ref.run) or against the reference modules evaluated on the
oracle's first-receipt matrix -- never against the engine's own output, except
where a case says "identical to the first run".  The conditions that make a
case late (rounds == 254, cells with first >= 128, a value of 254, crashes past
round 128 ...) are asserted on the references before the engine is touched and
printed, so a flood that ended early cannot pass.

  a  parity in the five forced modes            e  the ceiling itself
  b  the planner's switches, late               f  liveness late (crashes, churn, partitions)
  c  every record at once, late                 g  lossy links late
  d  records between rounds                     h  message shards, a shard job, checkpoints
"""
import functools

import numpy as np
import pytest

import delay_dist_ref
import delay_ref
import load_ref
import long_shapes as ls
import lossy_ref
import watch_ref
from test_gpu_curve import MODE_IDS, MODES, STAT_KEYS, check_curve, check_run, histogram, mode_cfg, run
from test_gpu_delay_dist import check_dist
from test_gpu_link_loss import LIVE_KEYS, changed_share, check_lossy, lossy
from test_gpu_parity import _group_run
from test_gpu_records_matrix import RECORDS, check_records, check_sums, expected
from test_gpu_shard_job import Job, check_record, record
from test_gpu_watch import check_watch

pytestmark = pytest.mark.gpu

R = ls.CEILING
SHAPES = {"path": ls.path, "far_hubs": ls.far_hubs, "thick_ring": ls.thick_ring}
WATCHED = [1, 130, 250, 254, 255, 299, 400, 401]   # far_hubs: both centres, the last vertex reached, two leaves of 250
ALL = RECORDS + ("delay_dist",)


def _pkg():
    import _gossip_pkg
    return _gossip_pkg.load()


@functools.lru_cache(maxsize=None)
def _ref(shape, kind, m, crashes=(), churn=None):
    """(g, origin, inject, kw, ref): the oracle's run of table `kind` on overlay
    `shape`; crashes: tuple of (vertex, round); churn: (p_fail, churn_seed)"""
    from oracle import lib
    pkg = _pkg()
    g = SHAPES[shape](pkg)
    origin, inject = ls.table(pkg, g, kind, m)
    kw = {}
    if crashes:
        kw["crashes"] = list(crashes)
    if churn:
        kw.update(churn=True, p_fail=churn[0], churn_seed=churn[1])
    ref = lib.run(g, origin, inject, want_first=True, **kw)
    return g, origin, inject, kw, ref


def describe(tag, ref, g=None):
    """the printed counts the summary quotes: what the reference holds late"""
    late, last, never = ls.late_counts(ref["first"])
    st = ref["stats"]
    line = (f"{tag}: rounds={ref['rounds']} cells>=128: {late} cells==254: {last} never: {never} "
            f"injected>=128: {sum(s['injected'] for s in st[128:])} lost>=128: {sum(s.get('lost', 0) for s in st[128:])} "
            f"crashed>=128: {sum(s['crashed'] for s in st[128:])} "
            f"reports>=128: {sum(s.get('reports', 0) for s in st[128:])} "
            f"removals>=128: {sum(s.get('removals', 0) for s in st[128:])}")
    if g is not None:
        hubs = np.nonzero(np.diff(np.asarray(g.row_ptr, np.int64)) > 64)[0]
        for v in hubs:
            got = ref["first"][v]
            line += f" hub {int(v)} commits in rounds {sorted(set((got[got != 255].astype(int) - 1).tolist()) - {-1})}"
    print(line)
    return late, last, never


def is_late(ref, cells=1):
    """conditions on the reference alone: the run was cut by the ceiling, holds
    254 beside 255, and `cells` receipts at or past the middle of the u8 range"""
    late, last, never = ls.late_counts(ref["first"])
    assert ref["rounds"] == R and late >= cells and last > 0 and never > 0, (ref["rounds"], late, last, never)
    assert int(ref["first"][ref["first"] != 255].max()) == R


def cfg_of(kw, **cfg):
    if "churn" in kw:
        cfg.update(churn=1, p_fail=kw["p_fail"], churn_seed=kw["churn_seed"])
    return cfg


def engine(pkg, g, origin, inject, records=(), watch=None, **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    for rec in records:
        getattr(eng, "track_" + rec)()
    if watch is not None:
        eng.watch(watch)
    eng.reset()
    return eng


def run_with_reports(eng, inject, crashes=()):
    """test_gpu_curve.run, collecting the dead-node reports of every round"""
    by_round = {}
    for v, r in crashes:
        by_round.setdefault(r, []).append(v)
    last = int(np.max(inject))
    stats, reports = [], []
    for r in range(R):
        if r in by_round:
            eng.crash(by_round[r])
        st = eng.round()
        stats.append(st)
        rep, nrep = eng.reports()
        assert nrep == len(rep)
        reports.extend(map(tuple, rep.tolist()))
        if st["new_bits"] == 0 and r >= last:
            break
    return stats, reports


def check_parity(eng, stats, ref, inject, forwards=True, monkeypatch=None):
    """stats per round, first, seen, seenpop, digest, the 255-row curve, and
    coverage and forwards after finalize(), through both of its paths"""
    assert len(stats) == R
    assert np.array_equal(eng.first(), ref["first"]), np.argwhere(eng.first() != ref["first"])[:8]
    assert np.array_equal(eng.seenpop().astype(np.int64), (ref["first"] != 255).sum(axis=1))
    check_curve(eng.curve(), ref, inject)
    check_run(eng, stats, ref)   # (finalize by the component path: no component is ever completed here)
    if forwards:
        assert np.array_equal(eng.forwards(), ref["forwards"])
    if monkeypatch is not None:
        monkeypatch.setenv("GP_FINALIZE_ROWS", "1")
        eng.finalize()
        monkeypatch.delenv("GP_FINALIZE_ROWS")
        assert np.array_equal(eng.coverage(), ref["coverage"])
        if forwards:
            assert np.array_equal(eng.forwards(), ref["forwards"])


# -- a. parity in every forced mode -------------------------------------------------

PARITY = [("path", 4096)] + [("far_hubs", h) for h in (4096, 64)]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [100, 4096])
@pytest.mark.parametrize("kind", ["ends", "late", "uniform"])
@pytest.mark.parametrize("shape,hub", PARITY, ids=[f"{s}-hub{h}" for s, h in PARITY])
def test_parity(pkg, oracle, monkeypatch, shape, hub, kind, m, mode):
    g, origin, inject, _, ref = _ref(shape, kind, m)
    describe(f"a {shape} {kind} m={m}", ref, g if hub == 64 else None)
    is_late(ref)
    if shape == "path" and kind == "uniform":
        assert ref["first"][254, 0] == 254 and ref["first"][255, 0] == 255
    if kind == "late":   # an injection of round 253 is held by its neighbours in receipt round 254
        k = int(np.nonzero((inject == 253) & (origin == 299))[0][0])
        assert ref["first"][299, k] == 253 and ref["first"][298, k] == 254
    with engine(pkg, g, origin, inject, ("curve",), track_first=1, track_digest=1, hub_threshold=hub,
                **mode_cfg(mode)) as eng:
        assert eng.words == ls.WORDS[m]
        stats = run(eng, inject)
        check_parity(eng, stats, ref, inject, monkeypatch=monkeypatch)


# -- b. the planner's switches, late ------------------------------------------------

SWITCH_CASES = [(4, None), (2, None), (0, None), (2, 0), (0, 0)]


@pytest.mark.parametrize("mi,prefilter", SWITCH_CASES,
                         ids=[MODE_IDS[mi] + ("" if pf is None else f"-prefilter{pf}") for mi, pf in SWITCH_CASES])
def test_planner_switches_late(pkg, oracle, mi, prefilter):
    """path x uniform at m = 4096, one context, no liveness, compact_rows = 0
    (the setting of the suite's aliasing cases).  The frontier is one vertex in
    every round, and half the n x m bits are held once vertex 149 is reached
    (csrc/round_plan.h: half_held), so the late switches can only fire late:

      adaptive: the direction estimate is the two arcs of last round's one
        receiver, est * push_ratio = 20 <= nnz = 598: every round pushes, and
        none of the pull's switches is ever planned (mode 1, scan 0).
      pulls (push_ratio 0): early exit and the done-neighbour rule start with
        half_held: done_nb = 1 in every round from 149 to 253, in none before.
        One sender is under prefilter_pct = 20 % of the vertices, so every pull
        is the prefiltered variant (scan 3; before half_held a degree-split
        round, scan 35), which compiles no aliasing (csrc/pull.hip: ALIASABLE
        wants SCAN_FILTERED or SCAN_UNFILTERED): the receiver that completes
        its component writes its row, aliased stays 0 and the done probe (scan
        bit 64) is never planned.
      pulls with prefilter_pct = 0: the plain filtered variant runs, the
        receiver of every round from 149 on completes its component and
        commits an alias (aliased = 1), and from the round after the first
        alias every scanned arc probes the done bitmap (scan bit 64).  The
        receivers still neither done nor sated are under a third of the
        vertices once 200 of the 300 are complete: from round 200 the waves take
        their receivers from the list the pull before left (scan bit 128).
    """
    g, origin, inject, _, ref = _ref("path", "uniform", 4096)
    is_late(ref)
    cfg = dict(mode_cfg(MODES[mi]), compact_rows=0)
    if prefilter is not None:
        cfg["prefilter_pct"] = prefilter
    with engine(pkg, g, origin, inject, ("curve",), track_first=1, **cfg) as eng:
        assert eng.words == 64
        stats = run(eng, inject)
        for key in ("mode", "scan", "done_nb", "aliased"):
            print(key, [s[key] for s in stats])
        at = {key: [s["round"] for s in stats if s[key] > 0] for key in ("done_nb", "aliased")}
        probed = [s["round"] for s in stats if s["scan"] & 64]
        if MODE_IDS[mi] == "adaptive":
            assert all(s["next_arcs"] * 10.0 <= g.nnz for s in stats[:-1])   # the gate that keeps the pull away
            assert all(s["mode"] == 1 and s["scan"] == 0 for s in stats) and not at["done_nb"] and not at["aliased"]
        else:
            assert all(s["mode"] == 0 for s in stats)
            assert at["done_nb"] and min(at["done_nb"]) >= 128 and max(at["done_nb"]) == 253, at["done_nb"]
            if prefilter is None:
                assert all((s["scan"] & 3) == 3 for s in stats) and not at["aliased"] and not probed
            else:
                assert at["aliased"] and min(at["aliased"]) >= 128 and max(at["aliased"]) == 253, at["aliased"]
                assert probed and min(probed) > min(at["aliased"]) and max(probed) == 253, probed
                listed = [s["round"] for s in stats if s["scan"] & 128]
                assert listed and min(listed) >= 128 and max(listed) == 253, listed
                for s in stats:   # an aliased receiver writes no row
                    assert s["rows_written"] + s["aliased"] <= s["receivers"]
        check_parity(eng, stats, ref, inject)


# -- c. every record at once, late ----------------------------------------------------

def all_expected(key, g, ref, inject, verts, **kw):
    """expected() of test_gpu_records_matrix with the delay distributions and the watch record"""
    exp = expected(key, g, ref, inject, **kw)
    if "dist" not in exp:
        exp["dist"] = delay_dist_ref.totals(ref, inject)
        exp["watch"] = watch_ref.record(g, ref, verts, **kw)
    return exp


def check_all(pkg, eng, g, exp, origin, inject, r=None):
    """the nine records: at the end of the run, or as they stand after round r"""
    check_records(pkg, eng, g, exp, r)
    if r is None:
        check_dist(pkg, eng, g, (exp["dist"]["dist"], exp["dist"]["seenpop"]))
        check_watch(eng, exp["watch"])
    else:
        check_dist(pkg, eng, g, exp["dist"]["per_round"][r])
        check_watch(eng, exp["watch"], origin, inject, r + 1)


def late_records(g, ref, exp, inject):
    """conditions on the references alone, before the engine is touched"""
    is_late(ref)
    assert int(exp["delay"]["max"].max()) == R
    dist = exp["dist"]["dist"]
    window = np.nonzero((dist[:, 1:16] > 0).all(axis=1))[0]   # delays 1 .. 14 and the saturated column at once
    assert ls.FAN_AT in window.tolist(), window
    assert int(exp["fc"]["curve"][R].sum()) > 0 and exp["fc"]["curve"].shape[0] == R + 1
    arr = exp["watch"]["arrival"]
    assert (arr == R).any() and ((arr >= 128) & (arr <= 253)).any()
    print(f"records: delay_max={int(exp['delay']['max'].max())} vertices with columns 1..15 > 0: {window.tolist()} "
          f"fresh_curve[254]={int(exp['fc']['curve'][R].sum())} watch arrivals ==254: {int((arr == R).sum())} "
          f"in 128..253: {int(((arr >= 128) & (arr <= 253)).sum())}")


RECORD_CASES = [(200, 0), (200, 4), (1000, 0), (4096, 0), (4096, 4)]


@pytest.mark.parametrize("m,mi", RECORD_CASES, ids=[f"{m}-{MODE_IDS[mi]}" for m, mi in RECORD_CASES])
def test_every_record_late(pkg, oracle, m, mi):
    g, origin, inject, _, ref = _ref("far_hubs", "late", m)
    exp = all_expected(("long", "far_hubs", "late", m), g, ref, inject, WATCHED)
    describe(f"c far_hubs late m={m}", ref, g)
    late_records(g, ref, exp, inject)
    with engine(pkg, g, origin, inject, ALL, WATCHED, hub_threshold=64, **mode_cfg(MODES[mi])) as eng:
        assert eng.words == ls.WORDS[m]
        stats = run(eng, inject)
        assert len(stats) == R
        check_all(pkg, eng, g, exp, origin, inject)   # (check_records ends with check_sums: the identities of §2.4)
        curve = eng.curve()
        check_curve(curve, ref, inject)
        assert curve.shape[0] == R + 1
        d = delay_ref.totals(ref, inject)
        assert pkg.latency.total_delay(curve, inject) == int(d["sum"].sum())
        hist = pkg.latency.delay_hist(curve, inject).astype(np.int64)
        delays = ref["first"].astype(np.int64) - inject.astype(np.int64)[None, :]
        assert np.array_equal(hist, np.bincount(delays[ref["first"] != 255], minlength=R + 1)) and hist[R] > 0
        check_run(eng, stats, ref)


# -- d. records between rounds ----------------------------------------------------------

@pytest.mark.parametrize("mi", [0, 4], ids=["pull", "adaptive"])
def test_records_between_rounds(pkg, oracle, mi):
    """every record read after rounds 127, 128, 253 and 254: on both sides of
    the u8's sign bit, and on both sides of the last round"""
    m = 200
    g, origin, inject, _, ref = _ref("far_hubs", "late", m)
    exp = all_expected(("long", "far_hubs", "late", m), g, ref, inject, WATCHED)
    late_records(g, ref, exp, inject)
    with engine(pkg, g, origin, inject, ALL, WATCHED, hub_threshold=64, **mode_cfg(MODES[mi])) as eng:
        stats = []
        for after in (127, 128, 253, 254):
            while len(stats) < after:
                stats.append(eng.round())
            check_all(pkg, eng, g, exp, origin, inject, after - 1)
            want = histogram(ref["first"], after + 1)
            want[after, inject == after] = 0   # round `after`'s injections are not made yet
            assert np.array_equal(eng.curve(), want)
        check_all(pkg, eng, g, exp, origin, inject)
        check_run(eng, stats, ref)


# -- e. the ceiling itself ------------------------------------------------------------------

READS = ("first", "seen", "seenpop", "digest", "curve", "load_sent", "load_recv", "fresh_sent", "fresh_recv",
         "fresh_curve", "link_fresh", "delay_sum", "delay_max", "delay_bins", "sole_sent", "sole_recv", "mult_hist",
         "delay_dist", "delay_dist_bins", "watch_first", "watch_arrival", "coverage", "forwards")


def status(pkg, fn, *args):
    try:
        fn(*args)
    except pkg.GossipError as e:
        return e.status
    return 0


def test_the_ceiling(pkg, oracle):
    m = 200
    g, origin, inject, _, ref = _ref("far_hubs", "late", m)
    is_late(ref)
    lib = pkg._lib
    with engine(pkg, g, origin, inject, ALL, WATCHED, track_first=1, hub_threshold=64) as eng:
        stats = eng.run(max_rounds=R)   # a fresh reset: 254 entries, no error
        assert len(stats) == R and [s["round"] for s in stats] == list(range(R))
        eng.finalize()
        before = {k: getattr(eng, k)() for k in READS}
        assert np.array_equal(before["first"], ref["first"]) and np.array_equal(before["coverage"], ref["coverage"])
        assert status(pkg, eng.round) == lib.GP_ESTATE          # round 254 is refused ...
        assert status(pkg, eng.run) == lib.GP_ESTATE            # ... through gp_run too
        assert status(pkg, eng.run, 1) == lib.GP_ESTATE
        for k in READS:                                         # and nothing was touched
            assert np.array_equal(getattr(eng, k)(), before[k]), k
        # inject rounds: 253 is the last one accepted, 254 and -1 leave the table in force
        for bad in (254, -1):
            inj = inject.copy()
            inj[3] = bad
            assert status(pkg, eng.set_messages, origin, inj) == lib.GP_EINVAL
        assert np.array_equal(eng.inject_round, inject) and eng.info()[2:] == (m, ls.WORDS[m])
        eng.reset()
        again = run(eng, inject)
        eng.finalize()
        assert len(again) == R
        for a, b in zip(again, stats):
            assert [a[k] for k in STAT_KEYS] == [b[k] for k in STAT_KEYS]
        for k in READS:                                         # a second full run is identical to the first
            assert np.array_equal(getattr(eng, k)(), before[k]), k
        check_run(eng, again, ref)
        inj = inject.copy()
        inj[:] = 253                                            # accepted: every message in the last round
        eng.set_messages(origin, inj)
        eng.reset()
        ref253 = oracle.run(g, origin, inj, want_first=True)
        assert ref253["rounds"] == R and set(np.unique(ref253["first"]).tolist()) == {253, 254, 255}
        stats = eng.run()
        assert np.array_equal(eng.first(), ref253["first"])
        check_curve(eng.curve(), ref253, inj)
        d = delay_ref.totals(ref253, inj)                       # (one inject round: the uniform passes, at round 253)
        assert np.array_equal(eng.delay_sum().astype(np.int64), d["sum"]) and set(d["max"].tolist()) == {0, 1}
        assert np.array_equal(eng.delay_max().astype(np.int64), d["max"])
        dd = delay_dist_ref.totals(ref253, inj)
        check_dist(pkg, eng, g, (dd["dist"], dd["seenpop"]))
        check_run(eng, stats, ref253)


@pytest.mark.parametrize("rounds", [100, R])
def test_forwards_of_a_cut_run(pkg, oracle, rounds):
    """A run that stops while its last round still made new bits -- after 100
    rounds, or at the ceiling -- holds receivers that have not sent yet.  The
    forwards taken from the Message-Lists (no track_msg_forwards) leave their
    sends out where the context keeps frontier rows (here: for the curve), and
    are refused (GP_ENOTRACK), not approximated, where it keeps none; the
    per-round pass (track_msg_forwards) is exact as ever, and a quiescent run of
    a plain context reads as before."""
    g, origin, inject, _, whole = _ref("far_hubs", "ends", 200)
    ref = whole if rounds == R else oracle.run(g, origin, inject, want_first=True, max_rounds=rounds)
    assert ref["rounds"] == rounds and ref["stats"][-1]["new_bits"] > 0
    holders = (ref["first"] != 255).astype(np.int64).T @ np.diff(np.asarray(g.row_ptr, np.int64))
    assert (ref["forwards"].astype(np.int64) < holders).all()   # every message has holders that never sent
    for records, fwd in (("curve",), 0), ((), 1), ((), 0):
        with engine(pkg, g, origin, inject, records, hub_threshold=64, track_msg_forwards=fwd) as eng:
            stats = [eng.round() for _ in range(rounds)]
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"])
            if records or fwd:
                assert np.array_equal(eng.forwards(), ref["forwards"])
            else:
                assert status(pkg, eng.forwards) == pkg._lib.GP_ENOTRACK
            assert [s["new_bits"] for s in stats] == [s["new_bits"] for s in ref["stats"]]
    small = ls.path(pkg, 40)
    o, i = np.arange(64, dtype=np.int32) % 40, (np.arange(64) % 3).astype(np.int32)
    done = oracle.run(small, o, i)
    with engine(pkg, small, o, i) as eng:
        stats = run(eng, i)
        assert len(stats) == done["rounds"] < R and stats[-1]["new_bits"] == 0
        eng.finalize()
        assert np.array_equal(eng.forwards(), done["forwards"]) and np.array_equal(eng.coverage(), done["coverage"])


# -- f. liveness late -----------------------------------------------------------------------

CHURN = (0.0002, 3)


@functools.lru_cache(maxsize=None)
def _late_crashes():
    """20 isolated vertices of the ring whose first receipt of some message is
    in round 200 crash in round 200 (no two of them within the ring's reach of
    2, so the floods go on), and two origins of round-253 messages in round 253"""
    g, origin, inject, _, plain = _ref("thick_ring", "late", 100)
    picked = []
    for v in np.nonzero((plain["first"] == 200).any(axis=1))[0].tolist():
        if all(min((v - u) % g.n, (u - v) % g.n) > 4 for u in picked):
            picked.append(v)
    picked = picked[:20]
    assert len(picked) == 20
    late_origins = sorted(set(origin[inject == 253].tolist()))[:2]
    assert len(late_origins) == 2 and not set(late_origins) & set(picked)
    return tuple((v, 200) for v in picked) + tuple((int(v), 253) for v in late_origins)


def liveness_ref(variant):
    crashes = _late_crashes() if variant == "crashes" else ()
    g, origin, inject, kw, ref = _ref("thick_ring", "late", 100, crashes, CHURN if variant == "churn" else None)
    plain = _ref("thick_ring", "late", 100)[4]
    late, last, never = describe(f"f thick_ring late m=100 {variant}", ref)
    is_late(ref, 10_000)
    st = ref["stats"]
    if variant == "crashes":
        picked = [v for v, r in crashes if r == 200]
        assert (ref["first"][picked] == 200).any() and not np.array_equal(ref["forwards"], plain["forwards"])
        assert st[200]["crashed"] == 20 and st[253]["crashed"] == 2 and st[253]["lost"] >= 2
        # (a crash in round 200 is missed in rounds 200, 201 and 202, miss_threshold = 3: the reports of round 202)
        assert sum(s["reports"] for s in st[201:]) >= 20 and sum(s["removals"] for s in st[201:]) == 20
    else:
        assert sum(s["crashed"] for s in st[128:]) >= 10 and sum(s["removals"] for s in st[128:]) > 0
    return g, origin, inject, kw, ref, list(crashes)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant,fwd", [("crashes", 1), ("churn", 0), ("churn", 1)],
                         ids=["crashes", "churn-bench-c5", "churn-frontier-rows"])
def test_liveness_late(pkg, oracle, variant, fwd, mode):
    g, origin, inject, kw, ref, crashes = liveness_ref(variant)
    with engine(pkg, g, origin, inject, ("curve",), **cfg_of(kw, track_first=1, track_digest=1, track_msg_forwards=fwd,
                                                           **mode_cfg(mode))) as eng:
        stats, reports = run_with_reports(eng, inject, crashes)
        assert sorted(reports) == sorted(map(tuple, ref["reports"].tolist()))
        assert any(r[2] >= (201 if variant == "crashes" else 128) for r in reports)
        check_parity(eng, stats, ref, inject, forwards=bool(fwd))


@pytest.mark.parametrize("mi", [0, 4], ids=["pull", "adaptive"])
def test_records_under_late_crashes(pkg, oracle, mi):
    g, origin, inject, kw, ref, crashes = liveness_ref("crashes")
    verts = [0, 5, 150, 299, crashes[0][0], crashes[0][0] + 1, 700, 1099]
    exp = all_expected(("long", "thick_ring", "late", 100, "crashes"), g, ref, inject, verts, **kw)
    assert np.array_equal(exp["load"]["crashed_at"], load_ref.crash_rounds(g.n, R, crashes))
    arr = exp["watch"]["arrival"]
    assert (arr == R).any() and ((arr >= 128) & (arr <= 253)).any()
    with engine(pkg, g, origin, inject, ALL, verts, track_msg_forwards=1, **mode_cfg(MODES[mi])) as eng:
        stats, _ = run_with_reports(eng, inject, crashes)
        check_all(pkg, eng, g, exp, origin, inject)
        check_curve(eng.curve(), ref, inject)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("variant", ["crashes", "churn"])
def test_liveness_late_partitioned(pkg, oracle, variant, P):
    g, origin, inject, kw, ref, crashes = liveness_ref(variant)
    engs, stats, reports = _group_run(pkg, g, origin, inject, P, crashes,
                                      **cfg_of(kw, track_first=1, track_digest=1, track_msg_forwards=1))
    try:
        assert len(stats) == R
        for a, b in zip(stats, ref["stats"]):
            for k in STAT_KEYS:
                assert a[k] == b[k], (P, k, a["round"], a[k], b[k])
        assert sum(s["xchg_rows"] for s in stats[128:]) > 0
        assert sorted(reports) == sorted(map(tuple, ref["reports"].tolist()))
        assert np.array_equal(np.concatenate([e.digest() for e in engs]), ref["digest"])
        assert np.array_equal(np.concatenate([e.first() for e in engs]), ref["first"])
    finally:
        for e in engs:
            e.close()


# -- g. lossy links late ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lossy_ref(m, churn):
    g, origin, inject, _, flood = _ref("thick_ring", "late", m)
    crash_at = load_ref.crash_rounds(g.n, R, churn=True, p_fail=CHURN[0], churn_seed=CHURN[1]) if churn else None
    ref = lossy_ref.run(g, origin, inject, p=0.1, seed=11, crash_at=crash_at)
    return g, origin, inject, flood, ref


def late_lossy(tag, ref, flood):
    """conditions on lossy_ref's run alone"""
    late, last, never = describe(tag, ref)
    share = changed_share(ref, flood)
    print(f"{tag}: {share:.3f} of the cells differ from the flood's")
    assert ref["rounds"] == R and late >= 10_000 and last > 0 and share >= 0.2


@pytest.mark.parametrize("fwd", [0, 1], ids=["plain", "msg-forwards"])
@pytest.mark.parametrize("m", [100, 1000])
def test_lossy_links_late(pkg, oracle, m, fwd):
    g, origin, inject, flood, ref = _lossy_ref(m, False)
    late_lossy(f"g thick_ring late m={m} p=0.1", ref, flood)
    with lossy(pkg, g, origin, inject, 0.1, 11, ("track_curve", "track_delay", "track_delay_dist"),
               track_msg_forwards=fwd) as eng:
        stats = run(eng, inject)
        assert np.array_equal(eng.curve(), histogram(ref["first"], R + 1))
        d = delay_ref.totals(ref, inject)
        assert int(d["max"].max()) >= 128
        assert np.array_equal(eng.delay_sum().astype(np.int64), d["sum"])
        assert np.array_equal(eng.delay_max().astype(np.int64), d["max"])
        assert np.array_equal(eng.delay_dist().astype(np.int64), delay_dist_ref.totals(ref, inject)["dist"])
        check_lossy(eng, stats, ref)


def test_lossy_links_late_under_churn(pkg, oracle):
    g, origin, inject, flood, ref = _lossy_ref(100, True)
    late_lossy("g thick_ring late m=100 p=0.1 churn", ref, flood)
    assert sum(s["crashed"] for s in ref["stats"][128:]) >= 10
    with lossy(pkg, g, origin, inject, 0.1, 11, ("track_curve",), churn=1, p_fail=CHURN[0], churn_seed=CHURN[1]) as eng:
        stats = run(eng, inject)
        assert np.array_equal(eng.curve(), histogram(ref["first"], R + 1))
        check_lossy(eng, stats, ref, LIVE_KEYS, forwards=False)


# -- h. shards and checkpoints ------------------------------------------------------------------

@pytest.mark.parametrize("shards", [2, 8])
def test_message_shards_late(pkg, oracle, shards):
    """the 4,096-message `late` table on far_hubs in word-aligned blocks: the
    firsts concatenate to the oracle's matrix, the records add or concatenate
    as DESIGN.md §2.4 says"""
    m = 4096
    g, origin, inject, _, ref = _ref("far_hubs", "late", m)
    exp = all_expected(("long", "far_hubs", "late", m), g, ref, inject, WATCHED)
    late_records(g, ref, exp, inject)
    step = m // shards
    add = {k: np.zeros(g.n, np.int64) for k in ("load_sent", "load_recv", "fresh_sent", "fresh_recv", "sole_sent",
                                                "sole_recv", "delay_sum")}
    link = np.zeros(g.nnz, np.int64)
    most = np.zeros(g.n, np.int64)
    firsts, hists, fcs, curves, dists, tables, dtables, wf, wa = [], [], [], [], [], [], [], [], []
    digest = np.zeros(g.n, np.uint64)
    for k in range(shards):
        lo, hi = k * step, (k + 1) * step
        with pkg.GossipEngine(0, track_first=1, hub_threshold=64) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            for rec in ALL:
                getattr(eng, "track_" + rec)()
            eng.watch(WATCHED)
            eng.reset()
            assert eng.words == step // 64
            stats = run(eng, inject[lo:hi])
            assert len(stats) == R   # every block's flood is cut by the ceiling
            for key in add:
                add[key] += getattr(eng, key)().astype(np.int64)
            lf = eng.link_fresh()
            link += lf
            most = np.maximum(most, eng.delay_max().astype(np.int64))
            firsts.append(eng.first())
            hists.append(eng.mult_hist())
            fcs.append(eng.fresh_curve().astype(np.int64))
            curves.append(eng.curve())
            dists.append(eng.delay_dist())
            tables.append(eng.delay_bins())
            dtables.append(eng.delay_dist_bins())
            wf.append(eng.watch_first())
            wa.append(eng.watch_arrival())
            check_sums(pkg, eng, lf)
            eng.finalize()
            assert np.array_equal(eng.coverage(), ref["coverage"][lo:hi])
            digest ^= eng.digest()
    assert np.array_equal(np.concatenate(firsts, axis=1), ref["first"])
    assert np.array_equal(digest, ref["digest"])
    for rec_, a, b in (("load", "sent", "recv"), ("fresh", "sent", "recv")):
        assert np.array_equal(add[rec_ + "_" + a], exp[rec_][a]) and np.array_equal(add[rec_ + "_" + b], exp[rec_][b]), rec_
    assert np.array_equal(link, exp["link"]["link"])
    assert np.array_equal(add["sole_sent"], exp["mult"]["sole_sent"])
    assert np.array_equal(add["sole_recv"], exp["mult"]["sole_recv"])
    assert np.array_equal(pkg.fragility.combine(hists).astype(np.int64), exp["mult"]["hist"])
    assert np.array_equal(add["delay_sum"], exp["delay"]["sum"]) and np.array_equal(most, exp["delay"]["max"])
    assert int(most.max()) == R
    assert np.array_equal(np.concatenate(fcs, axis=1), exp["fc"]["curve"])
    check_curve(np.concatenate(curves, axis=1), ref, inject)
    assert np.array_equal(pkg.latency.dist_combine(dists), exp["dist"]["dist"])
    assert np.array_equal(pkg.latency.dist_combine(dtables), delay_dist_ref.bins(g, exp["dist"]["dist"]).astype(np.int64))
    whole = delay_ref.bins(g, ref, inject)
    got = pkg.latency.combine(tables, disjoint=False)
    assert np.array_equal(got[:, [0, 2, 3, 4]], whole[:, [0, 2, 3, 4]])   # (`reached` is no function of the shards' tables)
    assert np.array_equal(np.concatenate(wf, axis=1), exp["watch"]["first"])
    assert np.array_equal(np.concatenate(wa, axis=1), exp["watch"]["arrival"])


def test_shard_job_to_the_ceiling(pkg, oracle):
    """two ranks over the host all-gather, both cut by the ceiling: combine(254)
    gives the oracle's 254 rounds, digest, coverage and forwards"""
    g, origin, inject, _, ref = _ref("far_hubs", "late", 4096)
    is_late(ref)
    job = Job(pkg, g, origin, inject, 2, dict(track_first=1, hub_threshold=64, track_msg_forwards=1))

    def body(k, e):
        job.join(k)
        stats = run(e, inject[job.blocks[k][0]:job.blocks[k][1]])
        assert len(stats) == R
        out = record(job, e, R)
        out.update(stats=stats)
        return out

    out = job.run(body)
    job.close()
    check_record(out, ref)
    assert all(len(o["job"]) == R for o in out)


@pytest.mark.parametrize("mi", [0, 4], ids=["pull", "adaptive"])
def test_checkpoints_late(pkg, oracle, mi):
    """a checkpoint after round 200 and one after round 254, restored into
    fresh engines"""
    m = 4096
    g, origin, inject, _, ref = _ref("far_hubs", "late", m)
    is_late(ref)
    cfg = dict(track_first=1, track_digest=1, track_msg_forwards=1, hub_threshold=64, **mode_cfg(MODES[mi]))
    with engine(pkg, g, origin, inject, **cfg) as eng:
        head = [eng.round() for _ in range(200)]
        blob200 = eng.checkpoint()
        tail = run_from(eng, 200)
        blob254 = eng.checkpoint()
        check_run(eng, head + tail, ref)
    with engine(pkg, g, origin, inject, **cfg) as eng:
        eng.restore(blob200)
        tail = run_from(eng, 200)
        assert [s["round"] for s in tail] == list(range(200, R))
        assert np.array_equal(eng.first(), ref["first"])
        check_run(eng, head + tail, ref)
        assert np.array_equal(eng.forwards(), ref["forwards"])
    with engine(pkg, g, origin, inject, **cfg) as eng:
        eng.restore(blob254)
        assert status(pkg, eng.round) == pkg._lib.GP_ESTATE
        assert status(pkg, eng.run) == pkg._lib.GP_ESTATE
        eng.finalize()
        assert np.array_equal(eng.coverage(), ref["coverage"])
        assert np.array_equal(eng.forwards(), ref["forwards"])
        assert np.array_equal(eng.first(), ref["first"]) and np.array_equal(eng.digest(), ref["digest"])


def run_from(eng, start):
    """the rounds start .. 253 (these floods never quiesce)"""
    return [eng.round() for _ in range(start, R)]
