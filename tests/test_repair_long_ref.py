"""tests/repair_ref.py up to the 254-round ceiling, pinned on the CPU, and the
conditions the cases of tests/test_gpu_repair_long.py rely on, asserted on the
reference alone (tests/repair_long_cases.py computes each case once).

The scalar twin: path(300), eight messages (the last two injected in round 253,
so the rule cannot end the run early), one message at a time in Python integers
from the normative text, all 254 rounds, at (p, period) = (0.5, 1), (0.3, 7)
and (0.5, 64): every cell of the first-receipt matrix, exchanges, lines and
new bits of every round.

The conditions, with what the reference gives (loss seed 11, repair seed 21
unless repair_long_cases.RSEEDS names another):

  to the ceiling, cells with 128 <= first <= 254 (the floor is half of it):
    thick_ring "ends" m=100 p=0.5, periods 1 / 2 / 3 / 7 / 16 / 63 / 64:
      25835 / 20156 / 16947 / 8837 / 4484 / 1092 / 879; the plain lossy run
      ends after 38 rounds; at periods 63 and 64, 149 and 140 rounds are silent
      and quiet peaks at 50 and 47 without stopping the run
    path "late" m=100 p=0.3, periods 1 / 8: 4773 / 1293; far_hubs: 8273 / 1293
    thick_ring "ends" period 2, m = 40 / 200 / 500 / 1000 / 2000 / 4000:
      7984 / 41586 / 101859 / 205314 / 406761 / 810641; m=4096 period 1: 1047093
    far_hubs "leaves" p=0.5, m = 200 / 1000 / 4096: period 1: 18574 / 89647 /
      370592, period 3: 14570 / 64070 / 267089
    thick_ring "late" m=100 p=0.3 period 1: 28485;  path "ends" period 63: 150
  cells with first = 254: thick_ring "ends" m=100 period 1: 230 (the ceiling
    case), path "late" period 1: 66 (the cut-run case), new bits in round 253
  share of the late cells the plain lossy run never reaches (>= 0.15):
    thick_ring 1.000, path "late" 0.961 / 0.858, far_hubs "late" 0.978 / 0.858,
    "leaves" 0.595 .. 0.728, thick_ring "late" p=0.3 0.976
  path "ends" p=0.5 period 64: 128 rounds, quiet = 64 at the end, the exchange
    of round 63 brings news after 59 silent rounds, the one of round 127 none
  path "ends" p=0.5 period 63: 254 rounds, quiet = 63 first reached in round 253
  "leaves", non-empty offers to hub 130 / hub 250 in the rounds >= 128:
    m=200: 17 / 13 (period 1), 13 / 9 (period 3, repair seed 230; seed 21: 6 / 3)
    m=1000: 38 / 44, 12 / 14;  m=4096: 41 / 44, 13 / 14
  repair rounds >= 128 with new bits and no sender, path "late" period 1:
    164, 188, 190, 217, 232
  path "uniform" p=1 period 64: 64 rounds, an all-zero record
  restart: path "ends" p=0.3 period 16 (repair seed 23) stops after 113 rounds;
    with quiet restarted at round 112 (quiet = 15 there) it runs 161 rounds,
    the exchanges of rounds 127 and 143 bring news, 320 cells differ
  the FAN vertex of thick_ring "late" p=0.3 period 1 holds the delays 1 .. 6
  crashes: 27 receivers get a non-empty offer in round 200 of thick_ring "ends"
    period 1; with ten of their partners and ten of them down the round's
    exchanges fall from 554 to 517 and 19 of the twenty receivers lose
    something; under churn (0.0002, seed 3) 25 peers crash at or after round 128
"""
import numpy as np
import pytest

import delay_dist_ref
import long_shapes as ls
import lossy_ref
import repair_long_cases as lc
import repair_ref

R = lc.R


# -- the scalar twin ------------------------------------------------------------------

def _scalar_long(harness, nbr, origins, injects, p, seed, period, rseed, rounds):
    """DESIGN.md §2.2 vertex by vertex in Python integers: the two draws of a
    round are taken once (they do not see the message), then every message
    goes through the round on its own -> (first[k] dicts, per round
    (new bits, exchanges, lines))"""
    thr = lossy_ref.threshold(p)
    closed = p >= 1.0
    first = [{o: i} for o, i in zip(origins, injects)]
    log = []
    for r in range(rounds):
        is_open = {(u, v): not closed and harness.draw(seed, 0x200 + r, (u << 32) | v) >= thr
                   for v, ins in nbr.items() for u in ins}
        partner = {}
        if period and (r + 1) % period == 0:
            for v, ins in nbr.items():
                q = ins[(harness.draw(rseed, 0x400 + r, v) * len(ins)) >> 64]
                if is_open[(q, v)]:
                    partner[v] = q
        new_bits = lines = 0
        for f in first:
            seen = {v for v, t in f.items() if t <= r}
            frontier = [v for v, t in f.items() if t == r]
            new = set()
            for u in frontier:
                for v in nbr[u]:   # (symmetric: u's in-list is its out-list)
                    if is_open[(u, v)] and v not in seen:
                        new.add(v)
            for v, q in partner.items():
                if q in seen and v not in seen:
                    lines += 1
                    new.add(v)
            for v in new:
                f[v] = r + 1
            new_bits += len(new)
        log.append((new_bits, len(partner), lines))
    return first, log


@pytest.mark.parametrize("p,period", [(0.5, 1), (0.3, 7), (0.5, 64)])
def test_scalar_twin_to_the_ceiling(pkg, harness, p, period):
    g = ls.path(pkg, 300)
    rp, col = np.asarray(g.row_ptr), np.asarray(g.col)
    nbr = {v: [int(u) for u in col[rp[v]:rp[v + 1]]] for v in range(g.n)}
    origin = np.array([0, 299, 150, 5, 0, 299, 150, 100], np.int32)
    inject = np.array([0, 1, 2, 100, 200, 240, 253, 253], np.int32)
    got = repair_ref.run(g, origin, inject, p=p, seed=lc.SEED, period=period, rseed=lc.RSEED, max_rounds=R)
    assert got["rounds"] == R
    first, log = _scalar_long(harness, nbr, origin.tolist(), inject.tolist(), p, lc.SEED, period, lc.RSEED, R)
    want = np.full((g.n, origin.size), 255, np.uint8)
    for k, f in enumerate(first):
        for v, t in f.items():
            want[v, k] = t
    bad = np.argwhere(got["first"] != want)
    assert bad.size == 0, bad[:8]
    assert [(s["new_bits"], s["exchanges"], s["lines"]) for s in got["stats"]] == log
    assert got["repair"].tolist() == [[x, n] for _, x, n in log]
    late, last, _ = ls.late_counts(want)
    print(f"p={p} period={period}: cells>=128: {late} cells==254: {last} lines in rounds>=128: "
          f"{sum(n for _, _, n in log[128:])}")
    assert late > 0 and last > 0 and sum(n for _, _, n in log[128:]) > 0


# -- the conditions -------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(lc.LATE_FLOOR), ids=lambda c: "-".join(map(str, c)))
def test_to_the_ceiling(pkg, case):
    ref = lc.repaired(*case)
    late, last, never = lc.describe("-".join(map(str, case)), ref, case[4])
    assert ref["rounds"] == R
    assert late >= lc.LATE_FLOOR[case] > 0, (late, lc.LATE_FLOOR[case])
    assert any(s["lines"] > 0 for s in ref["stats"][128:])


@pytest.mark.parametrize("case", [lc.CRASHES_LATE, lc.CUT_AFTER_OFFERS, lc.WIDTH_CASES[-1]],
                         ids=lambda c: "-".join(map(str, c)))
def test_first_254_present(pkg, case):
    """the cases used for the ceiling and for the forwards of a run it cut"""
    ref = lc.repaired(*case)
    last = ls.late_counts(ref["first"])[1]
    print(f"{case}: cells==254: {last} new bits in round 253: {ref['stats'][253]['new_bits']}")
    assert last >= 1 and ref["stats"][253]["new_bits"] > 0


SHARE_CASES = lc.CEILING_CASES + lc.LEAVES_CASES + [lc.RECORDS_LATE, lc.WIDTH_CASES[-1]]


@pytest.mark.parametrize("case", SHARE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_repair_matters_late(pkg, case):
    shape, kind, m, p, _ = case
    share = lc.late_share(lc.repaired(*case), lc.plain(shape, kind, m, p))
    print(f"{case}: {share:.3f} of the cells with first >= 128 are never reached by the lossy run "
          f"({lc.plain(shape, kind, m, p)['rounds']} rounds)")
    assert share >= lc.MIN_SHARE


def test_stops_by_the_rule_after_a_long_silence(pkg):
    g, origin, inject = lc.table(*lc.STOPS_BY_RULE[:3])
    ref = lc.repaired(*lc.STOPS_BY_RULE)
    q = lc.quiets(ref, inject, 64)
    nb = [s["new_bits"] for s in ref["stats"]]
    woken = [r for r in range(32, ref["rounds"]) if nb[r] > 0 and not any(nb[r - 32:r])]
    print(f"rounds={ref['rounds']} quiet at the end: {q[-1]}, new bits after >= 32 silent rounds in rounds {woken} "
          f"(silent before: {[next(k for k in range(1, r + 1) if nb[r - k]) - 1 for r in woken]})")
    assert ref["rounds"] == 128 and q[-1] == 64 and max(q[:-1]) < 64
    assert woken == [63] and ref["stats"][63]["lines"] > 0 and ref["stats"][127]["lines"] == 0
    assert ref["stats"][127]["exchanges"] > 0


def test_rule_and_ceiling_coincide(pkg):
    g, origin, inject = lc.table(*lc.COINCIDENCE[:3])
    ref = lc.repaired(*lc.COINCIDENCE)
    q = lc.quiets(ref, inject, 63)
    print(f"rounds={ref['rounds']} quiet first reaches 63 in round {q.index(63)}")
    assert ref["rounds"] == R and q.index(63) == 253


@pytest.mark.parametrize("case", lc.LEAVES_CASES, ids=lambda c: "-".join(map(str, c)))
def test_hubs_get_offers_late(pkg, case):
    shape, kind, m, p, period = case
    g = lc.table(shape, kind, m)[0]
    ref = lc.repaired(*case)
    assert (np.diff(np.asarray(g.row_ptr, np.int64)) > 64).nonzero()[0].tolist() == list(lc.HUBS)
    got = [lc.offer_rounds(g, ref, h, p, period, lc.rseed_of(case)) for h in lc.HUBS]
    print(f"{case}: non-empty offers in rounds >= 128: hub 130: {len(got[0])}, hub 250: {len(got[1])}")
    assert min(len(x) for x in got) >= 8


def test_news_from_offers_alone(pkg):
    ref = lc.repaired(*lc.CUT_AFTER_OFFERS)
    rounds = lc.offers_alone(ref, lc.CUT_AFTER_OFFERS[4])
    print(f"{lc.CUT_AFTER_OFFERS}: repair rounds >= 128 with new bits and no sender: {rounds}")
    assert rounds and all(ref["stats"][r]["lines"] >= ref["stats"][r]["new_bits"] > 0 for r in rounds)
    cut = lc.repaired(*lc.CUT_AFTER_OFFERS, max_rounds=rounds[0] + 1)
    assert cut["rounds"] == rounds[0] + 1 and cut["stats"][-1]["new_bits"] > 0 and cut["stats"][-1]["active"] == 0
    g = lc.table(*lc.CUT_AFTER_OFFERS[:3])[0]
    holders = (cut["first"] != 255).astype(np.int64).T @ np.diff(np.asarray(g.row_ptr, np.int64))
    assert (cut["forwards"].astype(np.int64) <= holders).all() and (cut["forwards"].astype(np.int64) < holders).any()


def test_all_arcs_closed(pkg):
    ref = lc.repaired(*lc.ALL_CLOSED)
    print(f"p=1 period=64: rounds={ref['rounds']}")
    assert ref["rounds"] == 64 and not ref["repair"].any() and ref["repair"].shape == (64, 2)
    assert ref["coverage"].tolist() == [1] * 100


def test_fan_vertex_under_repair(pkg):
    """the records case: FAN_AT's delay distribution holds several distinct columns"""
    g, origin, inject = lc.table(*lc.RECORDS_LATE[:3])
    row = delay_dist_ref.totals(lc.repaired(*lc.RECORDS_LATE), inject)["dist"][ls.FAN_AT]
    cols = np.nonzero(row[1:15])[0] + 1
    print(f"FAN_AT's row: {row.tolist()}; distinct delays in 1 .. 14: {cols.tolist()}")
    assert cols.size >= 4


def test_crashes_late(pkg):
    crashes, helped = lc.late_crashes()
    plain = lc.repaired(*lc.CRASHES_LATE)
    ref = lc.repaired(*lc.CRASHES_LATE, crashes=crashes)
    churn = lc.repaired(*lc.CRASHES_LATE, churn=lc.CHURN)
    late = sum(s["crashed"] for s in churn["stats"][128:])
    changed = int((ref["first"][helped] != plain["first"][helped]).any(axis=1).sum())
    print(f"round 200: exchanges {int(plain['repair'][200, 0])} -> {int(ref['repair'][200, 0])}, {changed} of the "
          f"twenty receivers lose something; churn: {late} crashes at or after round 128, {churn['rounds']} rounds")
    assert ref["stats"][200]["crashed"] == 20 and ref["rounds"] == R
    assert ref["repair"][200, 0] < plain["repair"][200, 0] and changed >= 15
    assert late >= 10 and churn["rounds"] == R and ls.late_counts(churn["first"])[0] >= lc.LATE_FLOOR[lc.CRASHES_LATE]


# -- restart ----------------------------------------------------------------------------

def test_quiet_restarted_in_a_silent_window(pkg):
    """a restore inside a silent window: the same run up to there, a longer one after"""
    g, origin, inject = lc.table(*lc.RESTART[:3])
    period = lc.RESTART[4]
    whole = lc.repaired(*lc.RESTART)
    T = whole["rounds"]
    c = T - 1
    q = lc.quiets(whole, inject, period)
    assert T < R and 0 < q[c - 1] < period and q[-1] == period
    ext = lc.repaired(*lc.RESTART, quiet_reset_at=c)
    nb = [s["new_bits"] for s in ext["stats"]]
    news = [r for r in range(T, ext["rounds"]) if repair_ref.is_repair_round(r, period) and nb[r] > 0]
    differ = int((ext["first"] != whole["first"]).sum())
    print(f"{lc.RESTART}: {T} rounds, quiet = {q[c - 1]} before round {c}; restarted there: {ext['rounds']} rounds, "
          f"repair rounds with news: {news}, {differ} cells differ")
    assert T < ext["rounds"] < R and news and differ > 0
    assert lc.quiets(ext, inject, period, c)[-1] == period
    early = whole["first"] <= c
    assert np.array_equal(ext["first"] <= c, early) and np.array_equal(ext["first"][early], whole["first"][early])
    assert ext["stats"][:T] == whole["stats"]
    assert all(ext["stats"][r]["lines"] > 0 and ext["stats"][r]["active"] == 0 for r in news)
    # (the default changes nothing)
    same = repair_ref.run(g, origin, inject, p=lc.RESTART[3], seed=lc.SEED, period=period,
                          rseed=lc.rseed_of(lc.RESTART), quiet_reset_at=None)
    assert same["rounds"] == T and np.array_equal(same["first"], whole["first"])
