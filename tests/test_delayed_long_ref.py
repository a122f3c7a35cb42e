"""tests/delayed_ref.py at the 254-round ceiling, pinned on the CPU before
test_gpu_link_delay_long.py compares the engine with it (shapes: long_shapes.py).

A delayed run that the ceiling cuts always has lines in flight: a line whose
receipt round would be 255 or later is simply lost, a receipt round of 254 sits
beside the sentinel 255, and the forwards count the send rounds up to 253.

  dmax = 1        delayed_ref.run is the C oracle's run, cut-run forwards included
  dmax 2 .. 8     first = inject + shortest path under the delays where that is
                  <= 254, else 255
  stopped runs    run(max_rounds=k) is the full run's first k rounds
  lateness        the conditions every case of the GPU file asserts, on every
                  overlay and dmax

Also the cached references and the lateness conditions the GPU file imports.
"""
import functools

import numpy as np
import pytest

import delayed_ref
import load_ref
import long_shapes as ls
from test_delayed_ref import FLOOD_KEYS, _dist
from test_gpu_long_runs import SHAPES, _pkg, _ref as oracle_ref

R = ls.CEILING
SEED = 11              # the delay seed of every case
DMAXES = list(range(2, 9))
STOPS = (1, 127, 128, 200, 253)


@functools.lru_cache(maxsize=None)
def case(shape, kind, m):
    """(g, origin, inject) of table `kind` on overlay `shape`"""
    pkg = _pkg()
    g = SHAPES[shape](pkg)
    origin, inject = ls.table(pkg, g, kind, m)
    return g, origin, inject


@functools.lru_cache(maxsize=None)
def crash_at(n, crashes=(), churn=None):
    """crashes: tuple of (vertex, round); churn: (p_fail, churn_seed)"""
    kw = dict(churn=True, p_fail=churn[0], churn_seed=churn[1]) if churn else {}
    return load_ref.crash_rounds(n, R, list(crashes), **kw)


@functools.lru_cache(maxsize=None)
def dref(shape, kind, m, dmax, p=None, loss_seed=0, crashes=(), churn=None, max_rounds=R):
    """delayed_ref.run of the case, delay seed SEED (read-only: shared by the tests)"""
    g, origin, inject = case(shape, kind, m)
    at = crash_at(g.n, crashes, churn) if crashes or churn else None
    ref = delayed_ref.run(g, origin, inject, dmax=dmax, seed=SEED, p=p, loss_seed=loss_seed, crash_at=at,
                          max_rounds=max_rounds)
    for a in (ref["first"], ref["seenpop"], ref["coverage"], ref["forwards"], ref["by_delay"]):
        a.setflags(write=False)
    return ref


def in_flight(ref, dmax, k=None):
    """send rounds s in [k + 1 - dmax, k - 1] with a sender, after k rounds
    (all of them by default): gp_link_delay_info's count"""
    k = ref["rounds"] if k is None else k
    return sum(1 for s in range(max(k + 1 - dmax, 0), k) if ref["stats"][s]["active"] > 0)


def lateness(tag, ref, dmax, cells=1, every_delay=True):
    """asserted on the reference alone and printed: the run was cut by the
    ceiling with dmax - 1 send rounds in flight and new bits in its last round,
    holds 254 beside 255 and `cells` receipts at or past round 128, and every
    delay value delivered news.  Returns (cells >= 128, cells == 254, in flight)"""
    late, last, never = ls.late_counts(ref["first"])
    flying = in_flight(ref, dmax)
    print(f"{tag} dmax={dmax}: rounds={ref['rounds']} cells>=128: {late} cells==254: {last} never: {never} "
          f"in flight at the cut: {flying} new bits in round 253: {ref['stats'][-1]['new_bits']} "
          f"first deliveries by delay {ref['by_delay'][1:].tolist()}")
    assert ref["rounds"] == R and late >= cells and last > 0 and never > 0, (ref["rounds"], late, last, never)
    assert int(ref["first"][ref["first"] != 255].max()) == R
    assert flying == dmax - 1, flying
    assert ref["stats"][-1]["new_bits"] == last
    if every_delay:
        assert (ref["by_delay"][1:dmax + 1] > 0).all(), ref["by_delay"]
    return late, last, flying


def last_round_messages(g, origin, inject, ref, dmax):
    """asserted on the reference: a message injected in round 253 (lines of
    rounds 246 .. 252 are in flight beside it) is held by its origin with 253
    and by exactly the neighbours behind one-round links with 254.  Returns the
    number of such neighbours over all round-253 messages"""
    delay = delayed_ref.arc_delays(g, dmax, SEED)
    src = np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(np.asarray(g.row_ptr, np.int64)))
    ks = np.nonzero(np.asarray(inject) == 253)[0]
    assert ks.size
    reached = 0
    for k in ks:
        near = dst[(src == origin[k]) & (delay == 1)]
        held = np.nonzero(ref["first"][:, k] != 255)[0]
        assert sorted(held.tolist()) == sorted(set(near.tolist()) | {int(origin[k])})
        assert ref["first"][origin[k], k] == 253 and (ref["first"][near, k] == R).all()
        reached += near.size
    return reached


def hub_commits(ref, origin, inject, v):
    """the rounds in which vertex v receives news (its own injections are no receipts)"""
    got = ref["first"][v]
    own = (np.asarray(origin) == v) & (got == np.asarray(inject))
    return sorted(set((got[(got != 255) & ~own].astype(int) - 1).tolist()))


# -- dmax = 1 at the ceiling --------------------------------------------------------

@pytest.mark.parametrize("kind", ["late", "ends"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_round_links_are_the_oracles_cut_run(pkg, oracle, shape, kind):
    g, origin, inject, _, ref = oracle_ref(shape, kind, 100)
    got = dref(shape, kind, 100, 1)
    late, last, never = ls.late_counts(ref["first"])
    print(f"{shape} {kind} dmax=1: rounds={ref['rounds']} cells>=128: {late} cells==254: {last} never: {never}")
    assert ref["rounds"] == R == got["rounds"] and last > 0 and never > 0
    assert in_flight(got, 1) == 0
    assert np.array_equal(got["first"], ref["first"])
    for a, b in zip(got["stats"], ref["stats"]):
        for k in FLOOD_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    assert np.array_equal(got["coverage"], ref["coverage"])
    # the oracle's forwards of a cut run: the receivers of round 253 have not sent
    assert np.array_equal(got["forwards"], ref["forwards"])
    deg = np.diff(np.asarray(g.row_ptr, np.int64))
    holders = (ref["first"] != 255).astype(np.int64).T @ deg
    cut = (ref["first"] == R).any(axis=0)
    assert cut.any() and (ref["forwards"].astype(np.int64)[cut] < holders[cut]).all()
    assert got["by_delay"][1] == sum(s["new_bits"] for s in ref["stats"])


# -- dmax 2 .. 8: shortest paths, cut at 254 ----------------------------------------

@pytest.mark.parametrize("dmax", DMAXES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_first_receipts_are_shortest_paths_up_to_254(pkg, shape, dmax):
    g, origin, inject = case(shape, "late", 100)
    ref = dref(shape, "late", 100, dmax)
    lateness(f"{shape} late m=100", ref, dmax)
    delay = delayed_ref.arc_delays(g, dmax, SEED)
    assert delay.min() == 1 and delay.max() == dmax
    want = _dist(g, delay, origin) + inject.astype(np.int64)[None, :]
    assert ((want >= 255) & (want < (1 << 39))).any()   # reachable, but past the ceiling: those lines are lost
    want = np.where(want <= R, want, 255).astype(np.uint8)
    assert np.array_equal(ref["first"], want), np.argwhere(ref["first"] != want)[:8]
    assert last_round_messages(g, origin, inject, ref, dmax) > 0


# -- stopped runs ---------------------------------------------------------------------

@pytest.mark.parametrize("shape,dmax", [("path", 3), ("far_hubs", 2), ("thick_ring", 5), ("thick_ring", 8)])
def test_stopped_runs_are_the_full_runs_head(pkg, shape, dmax):
    g, origin, inject = case(shape, "late", 100)
    full = dref(shape, "late", 100, dmax)
    lateness(f"{shape} late m=100", full, dmax)
    deg = np.diff(np.asarray(g.row_ptr, np.int64))
    for k in STOPS:
        cut = dref(shape, "late", 100, dmax, max_rounds=k)
        assert cut["rounds"] == k and cut["stats"] == full["stats"][:k]
        # (receipt round k is round k - 1's expansion; round k's own injections are not made yet)
        want = np.where((full["first"] > k) | ((full["first"] == k) & (inject == k)[None, :]), 255, full["first"])
        assert np.array_equal(cut["first"], want)
        assert np.array_equal(cut["coverage"], (want != 255).sum(axis=0).astype(np.uint64))
        sent = (cut["first"] <= k - 1).astype(np.int64)   # (255 = never: no sender)
        assert np.array_equal(cut["forwards"].astype(np.int64), sent.T @ deg)
        print(f"{shape} dmax={dmax} stopped after {k}: new bits in round {k - 1}: {cut['stats'][-1]['new_bits']} "
              f"in flight: {in_flight(cut, dmax)} forwards {int(cut['forwards'].sum())}")


# -- lateness -------------------------------------------------------------------------

TABLE = {   # (overlay, dmax): (cells >= 128, cells == 254, in flight at the cut), table `late`, m = 100
    ("path", 2): (6125, 83, 1), ("path", 3): (4455, 74, 2), ("path", 8): (2123, 35, 7),
    ("far_hubs", 2): (9725, 138, 1), ("far_hubs", 4): (3660, 54, 3), ("far_hubs", 8): (5523, 35, 7),
    ("thick_ring", 2): (25874, 279, 1), ("thick_ring", 5): (14301, 165, 4), ("thick_ring", 8): (9973, 121, 7),
}


@pytest.mark.parametrize("shape,dmax", list(TABLE), ids=[f"{s}-{d}" for s, d in TABLE])
def test_lateness_counts(pkg, shape, dmax):
    """the counts the GPU cases rest on, as measured (seed 11)"""
    ref = dref(shape, "late", 100, dmax)
    assert lateness(f"{shape} late m=100", ref, dmax) == TABLE[shape, dmax]


def test_hubs_commit_late(pkg):
    """far_hubs: both centres hear news in several distinct rounds at dmax = 2;
    at dmax >= 5 the flood from vertex 0 no longer reaches vertex 130's side of
    the ceiling"""
    for kind, m, dmax, want in (("ends", 1000, 2, (3, 3)), ("late", 100, 2, (6, 3))):
        g, origin, inject = case("far_hubs", kind, m)
        ref = dref("far_hubs", kind, m, dmax)
        a, b = hub_commits(ref, origin, inject, 130), hub_commits(ref, origin, inject, 250)
        print(f"far_hubs {kind} m={m} dmax={dmax}: hub 130 commits in rounds {a}, hub 250 in rounds {b}")
        assert (len(a), len(b)) == want
    g, origin, inject = case("far_hubs", "late", 100)
    assert not hub_commits(dref("far_hubs", "late", 100, 5), origin, inject, 130)
