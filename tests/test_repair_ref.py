"""tests/repair_ref.py, the numpy reference of anti-entropy repair (DESIGN.md
§2.2), pinned on the CPU: without a period it is lossy_ref.run, with every arc
open repair changes no first receipt of the C oracle's flood, on a path its
partners and offers follow from the two draws alone, it stops by the silent-
period rule, a crashed partner answers nothing and a crashed receiver asks
nothing.  The last test asserts, on the reference alone, the conditions the
lossy cases of tests/test_gpu_repair.py rely on."""
import numpy as np
import pytest

import lossy_ref
import repair_cases as rc
import repair_ref

KEYS = ("round", "injected", "lost", "new_bits", "receivers", "sends", "active", "crashed")


@pytest.mark.parametrize("p", [0.0, 0.25, 0.5])
def test_no_period_is_the_lossy_run(pkg, oracle, p):
    g, origin, inject, _ = rc.table(4099, 100)
    a = lossy_ref.run(g, origin, inject, p=p, seed=11)
    b = repair_ref.run(g, origin, inject, p=p, seed=11, period=0, rseed=21)
    assert a["rounds"] == b["rounds"]
    for x, y in zip(a["stats"], b["stats"]):
        assert all(x[k] == y[k] for k in KEYS) and y["exchanges"] == 0 and y["lines"] == 0
    for k in ("first", "seenpop", "coverage", "forwards"):
        assert np.array_equal(a[k], b[k]), k
    assert b["repair"].shape == (b["rounds"], 2) and not b["repair"].any()


@pytest.mark.parametrize("period", [1, 2, 4])
@pytest.mark.parametrize("n", [4099, 5])
def test_open_arcs_repair_changes_no_first_receipt(pkg, oracle, n, period):
    """every bit an up neighbour holds was sent to v in the round after the
    neighbour first held it: the offers carry lines, none of them news"""
    g, origin, inject, flood = rc.table(n, 100)
    got = repair_ref.run(g, origin, inject, p=0.0, period=period, rseed=21)
    assert np.array_equal(got["first"], flood["first"])
    assert np.array_equal(got["coverage"], flood["coverage"]) and np.array_equal(got["forwards"], flood["forwards"])
    # the flood's last round is silent; the window of `period` silent rounds ends at most period - 1 later
    assert flood["rounds"] <= got["rounds"] <= flood["rounds"] + period - 1
    for a, b in zip(got["stats"], flood["stats"]):
        assert all(a[k] == b[k] for k in ("injected", "new_bits", "receivers", "sends", "active"))
    rec = got["repair"]
    for r in range(got["rounds"]):
        if not repair_ref.is_repair_round(r, period):
            assert not rec[r].any()
    if n == 4099:   # every arc is open: every vertex with a neighbour exchanges
        linked = int((np.diff(g.row_ptr) > 0).sum())
        assert 0 < linked <= n
        assert all(rec[r, 0] == linked for r in range(got["rounds"]) if repair_ref.is_repair_round(r, period))
        assert rec[:, 1].sum() > 0


def _scalar_run(harness, nbr, origin, inj, p, seed, period, rseed, rounds):
    """one message over an adjacency list, vertex by vertex, in Python integers from the normative text"""
    thr = lossy_ref.threshold(p)
    first = {origin: inj}
    log = []
    for r in range(rounds):
        seen = {v for v, t in first.items() if t <= r}
        frontier = {v for v, t in first.items() if t == r}
        new, ex, lines = set(), 0, 0
        for v, ins in nbr.items():
            for u in ins:
                if u in frontier and harness.draw(seed, 0x200 + r, (u << 32) | v) >= thr and v not in seen:
                    new.add(v)
            if period and (r + 1) % period == 0 and ins:
                q = ins[(harness.draw(rseed, 0x400 + r, v) * len(ins)) >> 64]
                if harness.draw(seed, 0x200 + r, (q << 32) | v) >= thr:
                    ex += 1
                    if q in seen and v not in seen:
                        lines += 1
                        new.add(v)
        for v in new:
            first[v] = r + 1
        log.append((len(new), ex, lines))
    return first, log


@pytest.mark.parametrize("period", [1, 2])
def test_path_by_hand(pkg, harness, period):
    """6-vertex path, one message per vertex-0 injection round: partners and
    offers recomputed per vertex from the two scalar draws"""
    n, p, seed, rseed = 6, 0.5, 11, 21
    i = np.arange(n - 1)
    g = pkg.CSR.from_arcs(n, np.concatenate([i, i + 1]), np.concatenate([i + 1, i]), directed=False)
    rp, col = np.asarray(g.row_ptr), np.asarray(g.col)
    nbr = {v: [int(u) for u in col[rp[v]:rp[v + 1]]] for v in range(n)}
    assert nbr[0] == [1] and nbr[5] == [4] and all(sorted(nbr[v]) == [v - 1, v + 1] for v in range(1, 5))
    # the end vertices have one neighbour: it is their partner in every round
    for r in range(8):
        pr = repair_ref.partners(g, rseed, r)
        assert pr[0] == 1 and pr[5] == 4 and all(pr[v] in nbr[v] for v in range(n))
    origin = np.zeros(8, np.int32)
    inject = np.arange(8, dtype=np.int32)
    got = repair_ref.run(g, origin, inject, p=p, seed=seed, period=period, rseed=rseed, max_rounds=40)
    plain = lossy_ref.run(g, origin, inject, p=p, seed=seed)
    differs = 0
    for k in range(8):
        first, log = _scalar_run(harness, nbr, 0, int(inject[k]), p, seed, period, rseed, got["rounds"])
        want = np.full(n, 255, np.uint8)
        for v, t in first.items():
            want[v] = t
        assert np.array_equal(got["first"][:, k], want), (k, got["first"][:, k], want)
        differs += int((want != plain["first"][:, k]).any())
    assert differs >= 3   # repair carried some message past a closed arc
    # the record: exchanges do not see the message; lines add over the messages
    logs = [_scalar_run(harness, nbr, 0, int(inject[k]), p, seed, period, rseed, got["rounds"])[1] for k in range(8)]
    for r in range(got["rounds"]):
        assert got["repair"][r, 0] == logs[0][r][1] == logs[7][r][1]
        assert got["repair"][r, 1] == sum(lg[r][2] for lg in logs)
        assert got["stats"][r]["new_bits"] == sum(lg[r][0] for lg in logs)


@pytest.mark.parametrize("period", [1, 3])
def test_termination_rule(pkg, oracle, period):
    g, origin, inject, _ = rc.table(4099, 100)
    got = repair_ref.run(g, origin, inject, p=0.5, seed=11, period=period, rseed=21)
    nb = [s["new_bits"] for s in got["stats"]]
    R, last = got["rounds"], int(inject.max())
    assert R < 254 and R - period >= last
    assert all(b == 0 for b in nb[R - period:]) and nb[R - period - 1] > 0
    # no earlier window of `period` silent rounds at or after the last inject round
    for r in range(last + period - 1, R - 1):
        assert any(nb[r - period + 1:r + 1]), r
    if period == 3:   # silent rounds occur before the end: the flood's rule would have stopped too early
        assert any(b == 0 for b in nb[last:R - period])
    assert np.array_equal(repair_ref.run(g, origin, inject, p=0.5, seed=11, period=period, rseed=21,
                                         max_rounds=R + 5)["first"], got["first"])


def test_crashed_partner_and_receiver(pkg):
    """arc 1 -> 2 alone, closed in round 0 and open in round 1: vertex 2 gets
    the message by the exchange of round 1 -- unless its partner or it is down"""
    g = pkg.CSR.from_arcs(3, [1], [2], directed=True)
    seed = next(s for s in range(1000) if not lossy_ref.arc_open(s, 0, 1, 2, 0.5) and lossy_ref.arc_open(s, 1, 1, 2, 0.5))
    # (a second message, injected at vertex 0 in round 1, keeps the run going past the silent round 0)
    origin, inject = np.array([1, 0], np.int32), np.array([0, 1], np.int32)
    base = repair_ref.run(g, origin, inject, p=0.5, seed=seed, period=1, rseed=21)
    assert base["first"][:, 0].tolist() == [255, 0, 2]
    assert base["repair"][:2].tolist() == [[0, 0], [1, 1]] and base["rounds"] == 3
    assert lossy_ref.run(g, origin, inject, p=0.5, seed=seed)["first"][:, 0].tolist() == [255, 0, 255]
    never = 1 << 30
    for down in (1, 2):
        crash_at = np.full(3, never, np.int64)
        crash_at[down] = 1
        got = repair_ref.run(g, origin, inject, p=0.5, seed=seed, period=1, rseed=21, crash_at=crash_at)
        assert got["first"][:, 0].tolist() == [255, 0, 255], down
        assert not got["repair"].any() and got["stats"][1]["crashed"] == 1
    # period 2: round 1 is the first repair round, the same exchange
    assert repair_ref.run(g, origin, inject, p=0.5, seed=seed, period=2, rseed=21)["first"][:, 0].tolist() == [255, 0, 2]
    # a self-loop partner is an exchange that offers nothing
    g = pkg.CSR(2, np.array([0, 1, 1], np.int64), np.array([0], np.int32), True)   # (a raw CSR: vertex 0's in-list is itself)
    got = repair_ref.run(g, np.array([0], np.int32), None, p=0.0, period=1, rseed=21)
    assert got["repair"].tolist() == [[1, 0]] and got["first"][:, 0].tolist() == [0, 255]


@pytest.mark.parametrize("period", rc.PERIODS)
@pytest.mark.parametrize("m", [64, 100, 512, 1000, 2048, 4096])
def test_conditions_of_the_gpu_cases(pkg, oracle, m, period):
    """at the 48-round cut repair has changed at least 0.15 of the first-receipt
    cells against the lossy run without it (the prototype: 0.172 - 0.236)"""
    ref, plain = rc.repaired(4099, m, period), rc.plain(4099, m)
    share = rc.changed_share(ref, plain)
    print(f"m={m} period={period}: {share:.3f} of the cells differ from the lossy run's, {ref['rounds']} rounds")
    assert share >= rc.MIN_SHARE
    assert ref["repair"][:, 1].sum() > 0 and ref["coverage"].sum() > plain["coverage"].sum()
