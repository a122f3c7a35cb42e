"""Anti-entropy repair (csrc/repair.hip, gp_repair) up to
the 254-round ceiling, at every period class, hubs included -- on the GPU.

test_gpu_repair.py steps a small-world overlay for 48 rounds at most, at periods
1 .. 3.  Here the three overlays of long_shapes.py run under loss and repair
until the ceiling cuts them or the silent-period rule stops them after a long
silence: partner streams up to 0x400 + 253 are drawn, first bytes up to 254 are
written through k_repair_offer / k_expand_repair and through the hubs'
accumulator rows, `quiet` counts up to 64, and runs that died dozens of rounds
ago are restarted by a single exchange.

Every comparison is an exact integer comparison against tests/repair_ref.py
(pinned at the ceiling by test_repair_long_ref.py, which also asserts, on the
reference alone, every condition that makes a case late) -- never against the
engine's own output.  What the reference gives (loss seed 11, repair seed 21
unless repair_long_cases.RSEEDS names another):

  a  every period class to the ceiling: thick_ring "ends" m=100 p=0.5, periods
     1 / 2 / 3 / 7 / 16 / 63 / 64: 25835 / 20156 / 16947 / 8837 / 4484 / 1092 /
     879 cells with first >= 128 (the lossy run alone ends after 38 rounds; at
     periods 63 and 64 quiet peaks at 50 and 47); path and far_hubs "late"
     p=0.3, periods 1 / 8: 4773 / 1293 and 8273 / 1293, 66 / 19 cells at 254
  b  every row width: thick_ring period 2 at m = 40 / 100 / 200 / 500 / 1000 /
     2000 / 4000 (W = 1 .. 64, all with a partial last word): 7984 .. 810641 late
     cells; m = 4096 at period 1: 1047093, 9668 cells at 254
  c  hubs late: far_hubs "leaves", hubs 130 / 250 get 17 / 13 (m=200), 38 / 44
     (1000), 41 / 44 (4096) non-empty offers past round 128 at period 1 and
     13 / 9 (repair seed 230), 12 / 14, 13 / 14 at period 3
  d  the stopping rule: path "ends" period 64 stops after 128 rounds (the
     exchange of round 63 restarts a flood dead for 59 rounds), p = 1 after 64
     with an all-zero record, period 63 in round 253 together with the ceiling
  e  the ceiling itself: thick_ring "ends" period 1, 230 cells at 254
  f  forwards of a cut run: path "late" period 1 stopped after round 164, whose
     news came from offers alone, and at the ceiling (66 new bits in round 253)
  g  records that survive, late: thick_ring "late" p=0.3 (FAN_AT holds the
     delays 1 .. 6) and "leaves" m=1000 period 3 through the hub table
  h  liveness late: 20 crashes in round 200 (exchanges 554 -> 517, 19 of the
     twenty receivers lose something), churn with 25 crashes past round 128
  i  a checkpoint inside a silent window: path "ends" p=0.3 period 16 (repair
     seed 23) ends after 113 rounds; restored at round 112 (quiet 15 -> 0) it
     ends after 161, the exchanges of rounds 127 and 143 bring news
  j  message blocks late                  k  tuning fields change nothing
"""
import ctypes

import numpy as np
import pytest

import delay_dist_ref
import delay_ref
import long_shapes as ls
import repair_long_cases as lc
from test_gpu_curve import MODE_IDS, MODES, histogram, mode_cfg
from test_gpu_link_loss import KEYS, LIVE_KEYS
from test_gpu_long_runs import status
from test_gpu_repair import check_repair, outputs, repairing, same, step

pytestmark = pytest.mark.gpu

R = lc.R
RECORDS = ("track_curve", "track_delay", "track_delay_dist")


def ident(case):
    return "-".join(map(str, case))


def open_case(pkg, case, track=(), **cfg):
    """the engine of a case, reset: (eng, g, origin, inject)"""
    shape, kind, m, p, period = case
    g, origin, inject = lc.table(shape, kind, m)
    eng = repairing(pkg, g, origin, inject, period, rseed=lc.rseed_of(case), p=p, seed=lc.SEED, track=track, **cfg)
    assert eng.repair_info() == (True, period, lc.rseed_of(case), 0) and eng.link_loss_info() == (True, p, lc.SEED)
    return eng, g, origin, inject


def step_by_the_rule(eng, ref, inject, period, start=0, reset_at=None, crashes=()):
    """round() from round `start` until `period` silent rounds or the ceiling;
    repair_info's quiet after every round is the reference's"""
    want = lc.quiets(ref, inject, period, reset_at)
    by_round = {}
    for v, r in crashes:
        by_round.setdefault(r, []).append(v)
    stats = []
    for r in range(start, R):
        if r in by_round:
            eng.crash(by_round[r])
        stats.append(eng.round())
        quiet = eng.repair_info()[3]
        assert r < len(want) and quiet == want[r], (r, quiet, want[r:r + 1])
        if quiet >= period:
            break
    return stats


def is_late(case, ref):
    late = ls.late_counts(ref["first"])[0]
    assert ref["rounds"] == R and late >= lc.LATE_FLOOR[case], (case, ref["rounds"], late)


# -- a. every period class to the ceiling ------------------------------------------

@pytest.mark.parametrize("case", lc.CEILING_CASES, ids=ident)
def test_every_period_to_the_ceiling(pkg, case):
    ref = lc.repaired(*case)
    is_late(case, ref)
    eng, g, origin, inject = open_case(pkg, case)
    with eng:
        assert eng.words == 2
        stats = step_by_the_rule(eng, ref, inject, case[4])
        assert len(stats) == R and [s["round"] for s in stats] == list(range(R))
        check_repair(eng, stats, ref)


# -- b. every row width ---------------------------------------------------------------

@pytest.mark.parametrize("case", lc.WIDTH_CASES, ids=ident)
def test_every_row_width(pkg, case):
    ref = lc.repaired(*case)
    is_late(case, ref)
    eng, g, origin, inject = open_case(pkg, case)
    with eng:
        assert eng.words == lc.WIDTH_WORDS[case[2]]
        check_repair(eng, step_by_the_rule(eng, ref, inject, case[4]), ref)


# -- c. hubs late ------------------------------------------------------------------------

@pytest.mark.parametrize("hub_threshold", [64, 4096])
@pytest.mark.parametrize("case", lc.LEAVES_CASES, ids=ident)
def test_hubs_late(pkg, case, hub_threshold):
    """hub_threshold=64: the offers to vertices 130 and 250 go through tbits,
    k_hub_lossy's accumulator row and the push's tail; 4096: the same receivers
    through k_expand_repair's marks.  Both are the reference's run."""
    ref = lc.repaired(*case)
    is_late(case, ref)
    eng, g, origin, inject = open_case(pkg, case, hub_threshold=hub_threshold)
    with eng:
        assert eng.words == ls.WORDS[case[2]]
        check_repair(eng, step_by_the_rule(eng, ref, inject, case[4]), ref)


# -- d. the stopping rule --------------------------------------------------------------------

@pytest.mark.parametrize("case,rounds", [(lc.STOPS_BY_RULE, 128), (lc.ALL_CLOSED, 64), (lc.COINCIDENCE, R)],
                         ids=["after-a-long-silence", "all-arcs-closed", "with-the-ceiling"])
def test_run_stops_by_the_rule(pkg, case, rounds):
    ref = lc.repaired(*case)
    assert ref["rounds"] == rounds
    eng, g, origin, inject = open_case(pkg, case)
    with eng:
        stats = eng.run()
        assert len(stats) == rounds
        assert eng.repair_info()[3] == case[4] == lc.quiets(ref, inject, case[4])[-1]
        check_repair(eng, stats, ref)
        if case is lc.ALL_CLOSED:
            assert not eng.repair_record().any()
        if rounds == R:
            assert status(pkg, eng.round) == pkg._lib.GP_ESTATE


# -- e. the ceiling itself -------------------------------------------------------------------

def read_repair(pkg, eng, cap):
    """gp_read_repair into a buffer of sentinels -> (rounds, the rows it wrote, the rest untouched)"""
    buf = np.full((301, 2), 0xA5A5A5A5A5A5A5A5, np.uint64)
    k = ctypes.c_int32(-1)
    rc = pkg._lib.load().gp_read_repair(eng._ctx, buf.ctypes.data if cap else None, cap, ctypes.byref(k))
    assert rc == 0
    n = min(cap, k.value)
    return k.value, buf[:n].copy(), bool((buf[n:] == 0xA5A5A5A5A5A5A5A5).all())


def test_the_ceiling(pkg):
    case = lc.CRASHES_LATE
    ref = lc.repaired(*case)
    is_late(case, ref)
    assert ls.late_counts(ref["first"])[1] > 0
    lib = pkg._lib
    eng, g, origin, inject = open_case(pkg, case)
    with eng:
        stats = [eng.round() for _ in range(R)]
        before, info = outputs(eng, stats), eng.repair_info()   # (first, digest, seen, coverage, forwards, the record)
        assert before[-1].shape == (R, 2) and info == (True, 1, lc.RSEED, 0)
        for _ in range(2):   # round 254 is refused, again and again, and nothing was touched
            assert status(pkg, eng.round) == lib.GP_ESTATE
            assert same(before, outputs(eng, stats)) and eng.repair_info() == info
        assert status(pkg, eng.run) == lib.GP_ESTATE
        for cap in (0, 100, R, 300):
            rounds, rows, untouched = read_repair(pkg, eng, cap)
            assert rounds == R and rows.shape[0] == min(cap, R) and untouched, cap
            assert np.array_equal(rows, ref["repair"][:min(cap, R)]), cap
        check_repair(eng, stats, ref)
        eng.reset()   # a new run keeps its record again, from one row on
        short = lc.repaired(*case, max_rounds=3)
        stats = []
        for r in range(3):
            stats.append(eng.round())
            assert eng.repair_record().shape == (r + 1, 2)
        check_repair(eng, stats, short)


# -- f. forwards of a cut repair run ---------------------------------------------------------

@pytest.mark.parametrize("fwd", [1, 0], ids=["msg-forwards", "from-the-lists"])
@pytest.mark.parametrize("stop", ["after-offers-alone", "ceiling"])
def test_forwards_of_a_cut_repair_run(pkg, stop, fwd):
    """A run stopped right after a repair round whose news all came from offers
    (no sender in that round), or by the ceiling with new bits in round 253,
    holds receivers that have not sent.  The per-round pass counts exactly; the
    forwards taken from the Message-Lists are exact too, because a lossy run
    keeps frontier rows to take the last receivers' share off again: the read
    is not refused and not approximate."""
    case = lc.CUT_AFTER_OFFERS
    whole = lc.repaired(*case)
    rounds = lc.offers_alone(whole, case[4])[0] + 1 if stop == "after-offers-alone" else R
    ref = lc.repaired(*case, max_rounds=rounds)
    last = ref["stats"][-1]
    assert ref["rounds"] == rounds >= 129 and last["new_bits"] > 0
    if stop == "after-offers-alone":
        assert last["active"] == 0 and last["lines"] >= last["new_bits"]
    else:
        assert ls.late_counts(ref["first"])[1] > 0
    g = lc.table(*case[:3])[0]
    holders = (ref["first"] != 255).astype(np.int64).T @ np.diff(np.asarray(g.row_ptr, np.int64))
    assert (ref["forwards"].astype(np.int64) < holders).any()   # some holders never sent
    eng, g, origin, inject = open_case(pkg, case, track_msg_forwards=fwd)
    with eng:
        stats = [eng.round() for _ in range(rounds)]
        check_repair(eng, stats, ref)   # (coverage and forwards after finalize(), both exact)


# -- g. records that survive, late -------------------------------------------------------------

@pytest.mark.parametrize("case,hub", [(lc.RECORDS_LATE, 4096), (lc.LEAVES_CASES[3], 64)], ids=["late", "leaves-hubs"])
def test_records_late(pkg, case, hub):
    """track_curve, track_delay, track_delay_dist read only the receivers' new
    rows: exact under repair, after round 200 and at the ceiling"""
    ref, mid = lc.repaired(*case), lc.repaired(*case, max_rounds=200)
    is_late(case, ref)
    eng, g, origin, inject = open_case(pkg, case, track=RECORDS, hub_threshold=hub)
    if case is lc.RECORDS_LATE:
        row = delay_dist_ref.totals(ref, inject)["dist"][ls.FAN_AT]
        assert np.count_nonzero(row[1:15]) >= 4, row
    with eng:
        stats = []
        for want, upto in ((mid, 200), (ref, R)):
            while len(stats) < upto:
                stats.append(eng.round())
            assert np.array_equal(eng.curve(), histogram(want["first"], upto + 1))
            d = delay_ref.totals(want, inject)
            assert np.array_equal(eng.delay_sum().astype(np.int64), d["sum"])
            assert np.array_equal(eng.delay_max().astype(np.int64), d["max"])
            assert np.array_equal(eng.delay_dist().astype(np.int64), delay_dist_ref.totals(want, inject)["dist"])
        assert int(d["max"].max()) >= 100
        check_repair(eng, stats, ref)


# -- h. liveness late ----------------------------------------------------------------------------
# (`sends` and forwards are left out, as in test_gpu_repair.py)

def test_crashed_partners_and_receivers_late(pkg):
    """before the repair round 200, ten partners whose Message-List would have
    brought news go down, and ten receivers about to be repaired"""
    case = lc.CRASHES_LATE
    crashes, helped = lc.late_crashes()
    plain, ref = lc.repaired(*case), lc.repaired(*case, crashes=crashes)
    assert ref["stats"][200]["crashed"] == 20 and ref["repair"][200, 0] < plain["repair"][200, 0]
    assert (ref["first"][helped] != plain["first"][helped]).any(axis=1).sum() >= 15
    eng, g, origin, inject = open_case(pkg, case)
    with eng:
        stats = step_by_the_rule(eng, ref, inject, case[4], crashes=crashes)
        check_repair(eng, stats, ref, LIVE_KEYS, forwards=False)


def test_churn_late(pkg):
    case = lc.CRASHES_LATE
    ref = lc.repaired(*case, churn=lc.CHURN)
    assert sum(s["crashed"] for s in ref["stats"][128:]) >= 10 and ref["rounds"] == R
    assert not np.array_equal(ref["first"], lc.repaired(*case)["first"])
    eng, g, origin, inject = open_case(pkg, case, churn=1, p_fail=lc.CHURN[0], churn_seed=lc.CHURN[1])
    with eng:
        check_repair(eng, step_by_the_rule(eng, ref, inject, case[4]), ref, LIVE_KEYS, forwards=False)


# -- i. a checkpoint inside a silent window ---------------------------------------------------------

def test_checkpoint_in_a_silent_window(pkg):
    """`quiet` is not part of a checkpoint: the restored run counts its silent
    rounds from 0 again, runs past the round the uninterrupted run ended in,
    and meets two more repair rounds that bring news"""
    case = lc.RESTART
    period, rseed = case[4], lc.rseed_of(case)
    whole = lc.repaired(*case)
    c = whole["rounds"] - 1
    ref = lc.repaired(*case, quiet_reset_at=c)
    inject = lc.table(*case[:3])[2]
    assert 0 < lc.quiets(whole, inject, period)[c - 1] < period
    assert whole["rounds"] < ref["rounds"] < R and not np.array_equal(whole["first"], ref["first"])
    lib = pkg._lib
    eng, g, origin, inject = open_case(pkg, case)
    with eng:
        head = [eng.round() for _ in range(c)]
        assert eng.repair_info()[3] == lc.quiets(whole, inject, period)[c - 1] > 0
        blob = eng.checkpoint()
        tail = step_by_the_rule(eng, whole, inject, period, start=c)   # uninterrupted: it ends where `whole` ends
        check_repair(eng, head + tail, whole)
    eng, g, origin, inject = open_case(pkg, case)
    with eng:
        eng.restore(blob)
        assert eng.repair_info() == (True, period, rseed, 0)
        assert status(pkg, eng.repair_record) == lib.GP_ESTATE
        stats = head + step_by_the_rule(eng, ref, inject, period, start=c, reset_at=c)
        assert status(pkg, eng.repair_record) == lib.GP_ESTATE
        assert len(stats) == ref["rounds"] != whole["rounds"] and eng.repair_info()[3] == period
        for a, b in zip(stats, ref["stats"]):
            assert a["mode"] == 2 and all(a[k] == b[k] for k in KEYS), (a["round"], [(a[k], b[k]) for k in KEYS])
        first = eng.first()
        assert np.array_equal(first, ref["first"]), np.argwhere(first != ref["first"])[:8]
        assert np.array_equal(eng.seenpop().astype(np.int64), ref["seenpop"])
        eng.finalize()
        assert np.array_equal(eng.coverage(), ref["coverage"]) and np.array_equal(eng.forwards(), ref["forwards"])
        assert not np.array_equal(eng.coverage(), whole["coverage"])
        eng.reset()   # a new run keeps its record again
        eng.round()
        assert eng.repair_record().shape == (1, 2)


# -- j. message blocks late ------------------------------------------------------------------------

def test_message_blocks_late(pkg):
    """the partner draw does not see the message: two halves of the table, each
    stepped the whole run's 254 rounds, give the run's columns; their lines add
    up, their exchanges are the run's"""
    case = lc.WIDTH_CASES[-1]
    shape, kind, m, p, period = case
    ref = lc.repaired(*case)
    is_late(case, ref)
    g, origin, inject = lc.table(shape, kind, m)
    cols, recs = [], []
    for k in range(2):
        with pkg.GossipEngine(0, track_first=1) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, k * 2048, (k + 1) * 2048)
            assert eng.words == 32
            eng.link_loss(p, lc.SEED)
            eng.repair(period, lc.RSEED)
            eng.reset()
            stats = [eng.round() for _ in range(R)]
            assert all(s["mode"] == 2 for s in stats)
            cols.append(eng.first())
            recs.append(eng.repair_record())
            assert (cols[-1] == R).any()
    assert np.array_equal(np.concatenate(cols, axis=1), ref["first"])
    assert np.array_equal(recs[0][:, 0], ref["repair"][:, 0]) and np.array_equal(recs[1][:, 0], ref["repair"][:, 0])
    assert np.array_equal(recs[0][:, 1] + recs[1][:, 1], ref["repair"][:, 1])
    assert recs[0][128:, 1].sum() > 0 and recs[1][128:, 1].sum() > 0


# -- k. tuning fields change nothing -----------------------------------------------------------------

@pytest.mark.parametrize("hub_threshold", [4096, 64])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_tuning_fields_change_nothing_late(pkg, mode, hub_threshold):
    case = lc.LEAVES_CASES[0]
    ref = lc.repaired(*case)
    is_late(case, ref)
    eng, g, origin, inject = open_case(pkg, case, hub_threshold=hub_threshold, **mode_cfg(mode))
    with eng:
        check_repair(eng, step(eng, case[4], R), ref)
