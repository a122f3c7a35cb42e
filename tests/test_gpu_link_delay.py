"""Delayed links (csrc/delayed.hip, gp_link_delay) on the GPU.

With delay on, the link between u and v takes d(u, v) in [1, dmax] rounds: the
line u sends in round s has receipt round s + d(u, v).  Two references, neither
of them the engine:
 - with dmax = 1 every link takes one round and k_expand_delayed /
   k_hub_delayed must give the C oracle's flood (oracle.run) bit for bit --
   through the ring, the delay bytes and the per-delay tables;
 - with dmax > 1 the numpy round loop of tests/delayed_ref.py (pinned to the
   oracle, to lossy_ref and to shortest paths by tests/test_delayed_ref.py):
   first-receipt matrix, seenpop, the per-round counters, coverage and
   forwards, all exact.
Every delayed case at 4,099 vertices first asserts, on the reference alone,
that at least half of the first-receipt cells differ from the flood's and that
every delay value 1 .. dmax delivered news: a kernel that ignored the delay
bytes, or one ring slot, could not pass.

Shapes are test_gpu_link_loss.py's: 4,099 vertices (no multiple of a wave's 64)
and 5 (fewer than one wave), every row width with partial last words, hubs
split over the hub table (hub_threshold=64: 44 receivers, one of in-degree
913), a directed overlay, a raw CSR with self-loops and repeated arcs.
"""
import functools

import numpy as np
import pytest

import delay_dist_ref
import delay_ref
import delayed_ref
import directed_shapes as ds
import load_ref
import lossy_ref
import raw_csr
from test_delayed_ref import path_case
from test_gpu_curve import MODE_IDS, MODES, _width_ref, check_run, histogram, mode_cfg, overlay
from test_gpu_delay import WIDTH_MS, WORDS
from test_gpu_fresh import _status

pytestmark = pytest.mark.gpu

KEYS = ("injected", "new_bits", "receivers", "sends", "active")
LIVE_KEYS = ("injected", "lost", "new_bits", "receivers", "active", "crashed")


def delayed(pkg, g, origin, inject, dmax, seed=0, p=None, loss_seed=0, track=(), **cfg):
    cfg.setdefault("track_first", 1)
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    eng.link_delay(dmax, seed)
    if p is not None:
        eng.link_loss(p, loss_seed)
    for t in track:
        getattr(eng, t)()
    eng.reset()
    return eng


def run(eng, inject, crashes=(), max_rounds=254):
    """round by round, to the delayed rule: no new bit, no injection left and
    nothing in flight (link_delay_info)"""
    by_round = {}
    for v, r in crashes:
        by_round.setdefault(r, []).append(v)
    last = int(np.max(inject)) if inject is not None and len(inject) else 0
    stats = []
    for r in range(max_rounds):
        if r in by_round:
            eng.crash(by_round[r])
        st = eng.round()
        stats.append(st)
        if st["new_bits"] == 0 and st["round"] >= last and eng.link_delay_info()[3] == 0:
            break
    return stats


@functools.lru_cache(maxsize=None)
def _ref(n, m, dmax, seed, p=None, loss_seed=0):
    g, origin, inject, flood = _width_ref(n, m)
    return g, origin, inject, flood, delayed_ref.run(g, origin, inject, dmax=dmax, seed=seed, p=p, loss_seed=loss_seed)


def assert_delays_matter(ref, flood, dmax):
    """on the reference alone (4,099 vertices, m > 1)"""
    share = float((ref["first"] != flood["first"]).mean())
    print(f"dmax={dmax}: {share:.3f} of the cells differ from the flood's, {ref['rounds']} rounds, "
          f"first deliveries by delay {ref['by_delay'][1:].tolist()}")
    assert share >= 0.5
    assert (ref["by_delay"][1:dmax + 1] > 0).all()


def check_delayed(eng, stats, ref, keys=KEYS, forwards=True):
    """a delayed run against delayed_ref.run's (or lossy_ref.run's) result: all exact"""
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


# -- dmax = 1: the new kernels against the C oracle -------------------------------

def check_flood(eng, stats, ref):
    assert all(s["mode"] == 2 and s["scan"] == 0 for s in stats)
    check_run(eng, stats, ref)
    assert np.array_equal(eng.first(), ref["first"])
    assert np.array_equal(eng.forwards(), ref["forwards"])


@pytest.mark.parametrize("m", WIDTH_MS)
@pytest.mark.parametrize("n", [4099, 5])
def test_one_round_links_are_the_oracles_flood(pkg, oracle, n, m):
    g, origin, inject, ref = _width_ref(n, m)
    with delayed(pkg, g, origin, inject, 1, 3) as eng:
        assert eng.info()[3] == WORDS[m] and eng.link_delay_info() == (True, 1, 3, 0)
        check_flood(eng, run(eng, inject), ref)
        assert (eng.arc_delays() == 1).all()


@pytest.mark.parametrize("hub_threshold", [4096, 64])
def test_one_round_links_four_word_rows(pkg, oracle, hub_threshold):
    """m = 200: W = 4, the one width WIDTH_MS has no table for"""
    g, origin, inject, flood = _width_ref(4099, 200)
    with delayed(pkg, g, origin, inject, 1, hub_threshold=hub_threshold) as eng:
        assert eng.words == 4
        check_flood(eng, run(eng, inject), flood)


@pytest.mark.parametrize("m", WIDTH_MS)
def test_one_round_links_hubs(pkg, oracle, m):
    """hub_threshold=64: 44 receivers go through k_hub_delayed and the push's receiver side"""
    g, origin, inject, ref = _width_ref(4099, m)
    deg = np.diff(g.row_ptr)
    assert (deg > 64).sum() == 44 and deg.max() == 913
    with delayed(pkg, g, origin, inject, 1, hub_threshold=64) as eng:
        check_flood(eng, run(eng, inject), ref)


def _directed(pkg, oracle, m):
    g = ds.oriented_chung_lu(pkg, oracle, 4099, 8, 2.2, 7, "coin")
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 3).astype(np.int32)
    return g, origin, inject


@pytest.mark.parametrize("hub_threshold", [4096, 64])
@pytest.mark.parametrize("m", [100, 4096])
def test_one_round_links_directed(pkg, oracle, m, hub_threshold):
    g, origin, inject = _directed(pkg, oracle, m)
    ref = ds.CachedOracle(oracle).run(g, origin, inject, want_first=True)
    with delayed(pkg, g, origin, inject, 1, hub_threshold=hub_threshold) as eng:
        check_flood(eng, run(eng, inject), ref)


@pytest.mark.parametrize("m", [100, 4096])
def test_raw_csr(pkg, oracle, m):
    """self-loops and repeated arcs: a loop delivers nothing new, parallel arcs share their delay"""
    g = raw_csr.loops_and_repeats(pkg)
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 3).astype(np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    with delayed(pkg, g, origin, inject, 1) as eng:
        check_flood(eng, run(eng, inject), ref)
    dref = delayed_ref.run(g, origin, inject, dmax=4, seed=11)
    assert_delays_matter(dref, ref, 4)
    with delayed(pkg, g, origin, inject, 4, 11) as eng:
        check_delayed(eng, run(eng, inject), dref)


# -- the arc delays ---------------------------------------------------------------

@pytest.mark.parametrize("shape", ["undirected", "directed", "raw"])
def test_arc_delays_are_the_twins(pkg, oracle, shape):
    if shape == "undirected":
        g = overlay(pkg, 4099)
    elif shape == "directed":
        g = ds.oriented_chung_lu(pkg, oracle, 4099, 8, 2.2, 7, "coin")
    else:
        g = raw_csr.loops_and_repeats(pkg)
    origin = np.zeros(1, np.int32)
    for dmax, seed in ((1, 0), (3, 5), (8, 11)):
        with delayed(pkg, g, origin, None, dmax, seed) as eng:
            got = eng.arc_delays()
            assert got.dtype == np.uint8 and got.shape == (g.nnz,)
            assert np.array_equal(got, pkg.lag.arc_delays(g, dmax, seed))
            assert np.array_equal(got.astype(np.int64), delayed_ref.arc_delays(g, dmax, seed))
            assert np.array_equal(eng.graph().col, g.col)   # GP_ROW_PTR / GP_COL order is the loaded CSR's


# -- against delayed_ref ----------------------------------------------------------

DELAYED_CASES = [(d, m) for d in (2, 4, 8) for m in (64, 100, 512, 1000)] + [(4, 2048), (4, 4096)]


@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("dmax,m", DELAYED_CASES)
def test_delayed_run(pkg, oracle, dmax, m, seed):
    g, origin, inject, flood, ref = _ref(4099, m, dmax, seed)
    assert_delays_matter(ref, flood, dmax)
    with delayed(pkg, g, origin, inject, dmax, seed) as eng:
        assert eng.link_delay_info() == (True, dmax, seed, 0)
        check_delayed(eng, run(eng, inject), ref)
        assert eng.link_delay_info()[3] == 0
        assert np.array_equal(eng.coverage(), flood["coverage"])   # slower, and as far
        if m == 64:   # the digest is still a pure function of the first-receipt matrix
            assert np.array_equal(eng.digest(), oracle.digest_from_first(ref["first"], origin))


@pytest.mark.parametrize("hub_threshold", [4096, 64])
def test_four_word_rows(pkg, oracle, hub_threshold):
    g, origin, inject, flood, ref = _ref(4099, 200, 4, 11)
    assert_delays_matter(ref, flood, 4)
    with delayed(pkg, g, origin, inject, 4, 11, hub_threshold=hub_threshold) as eng:
        assert eng.words == 4
        check_delayed(eng, run(eng, inject), ref)


def test_delayed_hubs(pkg, oracle):
    """hub_threshold=64 at dmax = 4: every hub's receipts come in over several
    rounds, each through k_hub_delayed's items and one commit"""
    g, origin, inject, flood, ref = _ref(4099, 1000, 4, 11)
    assert_delays_matter(ref, flood, 4)
    hubs = np.nonzero(np.diff(g.row_ptr) > 64)[0]
    assert hubs.size == 44
    for v in hubs:
        got = ref["first"][v]
        rounds = set(got[(got != 255) & ~((origin == v) & (got == inject))].tolist())   # (its own injections are no receipts)
        assert len(rounds) >= 3, (v, rounds)
    with delayed(pkg, g, origin, inject, 4, 11, hub_threshold=64) as eng:
        check_delayed(eng, run(eng, inject), ref)


@pytest.mark.parametrize("hub_threshold", [4096, 64])
def test_delayed_directed(pkg, oracle, hub_threshold):
    g, origin, inject = _directed(pkg, oracle, 100)
    ref = delayed_ref.run(g, origin, inject, dmax=4, seed=11)
    assert_delays_matter(ref, ds.CachedOracle(oracle).run(g, origin, inject, want_first=True), 4)
    with delayed(pkg, g, origin, inject, 4, 11, hub_threshold=hub_threshold) as eng:
        check_delayed(eng, run(eng, inject), ref)


def test_path(pkg):
    """a 6-vertex path, one message at vertex 0, dmax = 4: first[i] is the prefix
    sum of the path's delays (from the twin alone), rounds pass without a new
    bit, and the run lasts sum(d) + dmax rounds"""
    g, origin, inject, seed, d = path_case(pkg)
    want = np.concatenate([[0], np.cumsum(d)])
    with delayed(pkg, g, origin, inject, 4, seed) as eng:
        stats = run(eng, inject)
        assert np.array_equal(eng.first()[:, 0].astype(np.int64), want)
        quiet = [s["round"] for s in stats if s["new_bits"] == 0]
        assert quiet and min(quiet) + 1 < want[-1]
        assert len(stats) == int(d.sum()) + 4
        check_delayed(eng, stats, delayed_ref.run(g, origin, inject, dmax=4, seed=seed))
        eng.reset()
        assert len(eng.run()) == int(d.sum()) + 4   # gp_run stops by the same rule
        assert np.array_equal(eng.first()[:, 0].astype(np.int64), want)


@pytest.mark.parametrize("n,m", [(5, 1), (5, 100), (4099, 1), (5, 4096)])
def test_delayed_run_small(pkg, oracle, n, m):
    """fewer vertices than a wave, one message (no share asserted there)"""
    g, origin, inject, _, ref = _ref(n, m, 4, 11)
    with delayed(pkg, g, origin, inject, 4, 11) as eng:
        check_delayed(eng, run(eng, inject), ref)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", [100, 4096])
def test_tuning_fields_change_nothing(pkg, oracle, m, mode):
    g, origin, inject, flood, ref = _ref(4099, m, 4, 11)
    assert_delays_matter(ref, flood, 4)
    with delayed(pkg, g, origin, inject, 4, 11, **mode_cfg(mode)) as eng:
        check_delayed(eng, run(eng, inject), ref)


@pytest.mark.parametrize("blocks", [2, 8])
def test_message_blocks(pkg, oracle, blocks):
    """the delay does not see the message: a table run in blocks gives the columns of the whole run"""
    g, origin, inject, flood, ref = _ref(4099, 4096, 4, 11)
    assert_delays_matter(ref, flood, 4)
    step = 4096 // blocks
    cols = []
    for k in range(blocks):
        with pkg.GossipEngine(0, track_first=1) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, k * step, (k + 1) * step)
            assert eng.words == step // 64
            eng.link_delay(4, 11)
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
    ref = delayed_ref.run(g, origin, inject, dmax=4, seed=11)
    assert_delays_matter(ref, flood, 4)
    with delayed(pkg, g, origin, inject, 4, 11) as eng:
        check_delayed(eng, run(eng, inject), ref)


def test_lifecycle(pkg, oracle):
    g, origin, inject, flood, ref = _ref(4099, 100, 4, 11)
    ref12 = _ref(4099, 100, 4, 12)[4]
    ref2 = _ref(4099, 100, 2, 11)[4]
    ref8 = _ref(4099, 100, 8, 3)[4]
    for r, d in ((ref, 4), (ref12, 4), (ref2, 2), (ref8, 8)):
        assert_delays_matter(r, flood, d)
    assert not np.array_equal(ref["first"], ref12["first"])
    with delayed(pkg, g, origin, inject, 4, 11) as eng:
        stats = run(eng, inject)
        check_delayed(eng, stats, ref)
        a = outputs(eng, stats)
        eng.reset()                      # the same setting twice: identical
        stats = run(eng, inject)
        assert same(a, outputs(eng, stats))
        eng.link_delay(4, 12)            # another seed differs
        eng.reset()
        stats = run(eng, inject)
        check_delayed(eng, stats, ref12)
        assert not same(a, outputs(eng, stats))
        eng.link_delay(2, 11)            # another dmax: a smaller ring
        eng.reset()
        assert eng.link_delay_info() == (True, 2, 11, 0)
        eng.round()
        eng.link_delay(8, 3)             # a setting made mid-run changes nothing before the reset
        assert eng.link_delay_info()[:3] == (True, 2, 11)
        stats = [s for s in eng.run()]
        assert len(stats) + 1 == ref2["rounds"]
        assert np.array_equal(eng.first(), ref2["first"])
        eng.reset()                      # now it does: a larger ring
        assert eng.link_delay_info() == (True, 8, 3, 0)
        check_delayed(eng, run(eng, inject), ref8)
        eng.link_delay(None)             # back to the planner's flood
        eng.reset()
        assert eng.link_delay_info() == (False, 1, 0, 0)
        stats = eng.run()
        assert all(s["mode"] in (0, 1) for s in stats)
        check_run(eng, stats, flood)
        assert np.array_equal(eng.first(), flood["first"])
        assert _status(pkg, eng.arc_delays) == pkg._lib.GP_ENOTRACK


def test_in_flight(pkg, oracle):
    """link_delay_info()[3]: the rounds s in [round + 1 - dmax, round - 1] with a sender"""
    g, origin, inject, flood, ref = _ref(4099, 100, 4, 11)
    assert_delays_matter(ref, flood, 4)
    with delayed(pkg, g, origin, inject, 4, 11) as eng:
        active = []
        for r in range(ref["rounds"]):
            active.append(eng.round()["active"])
            want = sum(1 for s in range(r + 2 - 4, r + 1) if s >= 0 and active[s] > 0)
            assert eng.link_delay_info()[3] == want, r
        assert eng.link_delay_info()[3] == 0


def test_sweep(pkg, oracle):
    """lag.sweep: one reset and run per dmax"""
    g, origin, inject, flood, ref = _ref(4099, 100, 4, 11)
    assert_delays_matter(ref, flood, 4)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        out = pkg.lag.sweep(eng, [1, 4], seed=11)
        assert eng.link_delay_info() == (True, 4, 11, 0)
    assert [o["dmax"] for o in out] == [1, 4]
    for o, r in zip(out, (flood, ref)):
        assert o["rounds"] == r["rounds"] and np.array_equal(o["coverage"], r["coverage"])
        held = r["first"] != 255
        delays = (r["first"].astype(np.int64) - inject[None, :])[held]
        assert o["mean_delay"] == float(delays.sum()) / int((delays > 0).sum())
    assert out[1]["mean_delay"] > out[0]["mean_delay"]


# -- loss with delay --------------------------------------------------------------

def test_loss_with_delay(pkg, oracle):
    g, origin, inject, flood, ref = _ref(4099, 100, 4, 11, 0.5, 21)
    assert_delays_matter(ref, flood, 4)
    loss_only = lossy_ref.run(g, origin, inject, p=0.5, seed=21)
    assert float((ref["first"] != loss_only["first"]).mean()) >= 0.2
    with delayed(pkg, g, origin, inject, 4, 11, p=0.5, loss_seed=21) as eng:
        assert eng.link_loss_info() == (True, 0.5, 21)
        check_delayed(eng, run(eng, inject), ref)


@pytest.mark.parametrize("hub_threshold", [4096, 64])
def test_loss_with_delay_wide(pkg, oracle, hub_threshold):
    g, origin, inject, flood, ref = _ref(4099, 1000, 4, 11, 0.5, 21)
    assert_delays_matter(ref, flood, 4)
    with delayed(pkg, g, origin, inject, 4, 11, p=0.5, loss_seed=21, hub_threshold=hub_threshold) as eng:
        check_delayed(eng, run(eng, inject), ref)


@pytest.mark.parametrize("m", [100, 1000])
def test_loss_with_one_round_links_is_lossy_ref(pkg, oracle, m):
    g, origin, inject, flood = _width_ref(4099, m)
    ref = lossy_ref.run(g, origin, inject, p=0.5, seed=11)
    assert float((ref["first"] != flood["first"]).mean()) >= 0.2
    with delayed(pkg, g, origin, inject, 1, 7, p=0.5, loss_seed=11) as eng:
        check_delayed(eng, run(eng, inject), ref)


def test_every_arc_closed(pkg, oracle):
    g, origin, inject, flood = _width_ref(4099, 100)
    with delayed(pkg, g, origin, inject, 4, 11, p=1.0, loss_seed=5) as eng:
        stats = run(eng, inject)
        assert all(s["new_bits"] == 0 for s in stats) and sum(s["rows_gathered"] for s in stats) == 0
        check_delayed(eng, stats, delayed_ref.run(g, origin, inject, dmax=4, seed=11, p=1.0, loss_seed=5))
        assert (eng.coverage() == 1).all()


# -- liveness ---------------------------------------------------------------------
# (`sends` is left out: deg_live follows the seed's removals, the engine's
# unchanged removal path, which delayed_ref does not model; forwards likewise)

def _picked(plain):
    picked = np.nonzero((plain["first"] == 3).any(axis=1))[0][:20]
    assert picked.size == 20
    return picked


def test_crash_with_lines_in_flight(pkg, oracle):
    """20 peers with a first receipt in round 3 crash in round 5: what they sent
    in rounds 3 and 4 over slow links arrives after they are gone"""
    g, origin, inject, flood, plain = _ref(4099, 100, 4, 11)
    assert_delays_matter(plain, flood, 4)
    picked = _picked(plain)
    crashes = [(int(v), 5) for v in picked]
    ref = delayed_ref.run(g, origin, inject, dmax=4, seed=11, crash_at=load_ref.crash_rounds(g.n, 64, crashes))
    assert ref["rounds"] < 64 and not np.array_equal(ref["first"], plain["first"])
    # on the reference: a line of round 3 over a link of 3 or 4 rounds is the first to arrive somewhere
    delay = delayed_ref.arc_delays(g, 4, 11)
    dst = np.repeat(np.arange(g.n), np.diff(g.row_ptr))
    late = [j for j in np.nonzero(np.isin(g.col, picked) & (delay >= 3))[0]
            if ((ref["first"][g.col[j]] == 3) & (ref["first"][dst[j]] == 3 + delay[j])).any()]
    assert late
    with delayed(pkg, g, origin, inject, 4, 11) as eng:
        check_delayed(eng, run(eng, inject, crashes), ref, LIVE_KEYS, forwards=False)


def test_crash_right_after_receipt(pkg, oracle):
    """the same 20 peers crash in round 3: they never send"""
    g, origin, inject, flood, plain = _ref(4099, 100, 4, 11)
    assert_delays_matter(plain, flood, 4)
    picked = _picked(plain)
    crashes = [(int(v), 3) for v in picked]
    ref = delayed_ref.run(g, origin, inject, dmax=4, seed=11, crash_at=load_ref.crash_rounds(g.n, 64, crashes))
    assert ref["rounds"] < 64 and (ref["first"][picked] == 3).any()
    assert ref["stats"][3]["active"] == plain["stats"][3]["active"] - 20
    with delayed(pkg, g, origin, inject, 4, 11) as eng:
        check_delayed(eng, run(eng, inject, crashes), ref, LIVE_KEYS, forwards=False)


def test_churn(pkg, oracle):
    g, origin, inject, flood, plain = _ref(4099, 100, 4, 11)
    assert_delays_matter(plain, flood, 4)
    crash_at = load_ref.crash_rounds(g.n, 64, churn=True, p_fail=0.01, churn_seed=5)
    ref = delayed_ref.run(g, origin, inject, dmax=4, seed=11, crash_at=crash_at)
    assert ref["rounds"] < 64 and sum(s["crashed"] for s in ref["stats"]) > 100
    assert not np.array_equal(ref["first"], plain["first"])
    with delayed(pkg, g, origin, inject, 4, 11, churn=1, p_fail=0.01, churn_seed=5) as eng:
        check_delayed(eng, run(eng, inject), ref, LIVE_KEYS, forwards=False)


# -- records that survive ---------------------------------------------------------

@pytest.mark.parametrize("fwd", [0, 1], ids=["plain", "msg-forwards"])
@pytest.mark.parametrize("m", [100, 1000])
def test_records_of_the_receivers_rows(pkg, oracle, m, fwd):
    """track_curve, track_delay, track_delay_dist read only the receivers' new
    rows: exact for the delayed run, where a delay is no longer a hop count"""
    g, origin, inject, flood, ref = _ref(4099, m, 4, 11)
    assert_delays_matter(ref, flood, 4)
    with delayed(pkg, g, origin, inject, 4, 11, track=("track_curve", "track_delay", "track_delay_dist"),
                 track_msg_forwards=fwd) as eng:
        stats = run(eng, inject)
        assert np.array_equal(eng.curve(), histogram(ref["first"], ref["rounds"] + 1))
        d = delay_ref.totals(ref, inject)
        assert np.array_equal(eng.delay_sum().astype(np.int64), d["sum"])
        assert np.array_equal(eng.delay_max().astype(np.int64), d["max"])
        assert np.array_equal(eng.delay_dist().astype(np.int64), delay_dist_ref.totals(ref, inject)["dist"])
        check_delayed(eng, stats, ref)


# -- refusals ---------------------------------------------------------------------

def test_refusals(pkg, oracle):
    g, origin, inject, flood, ref = _ref(4099, 100, 4, 11)
    assert_delays_matter(ref, flood, 4)
    lib = pkg._lib
    with pkg.GossipEngine(0, track_first=1) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.link_delay(4, 11)
        for bad in (0, 9, -1):
            assert _status(pkg, lambda: eng.link_delay(bad, 3)) == lib.GP_EINVAL
        for name, on, off in (("track_load", eng.track_load, lambda: eng.track_load(False)),
                              ("track_fresh", eng.track_fresh, lambda: eng.track_fresh(False)),
                              ("track_fresh_curve", eng.track_fresh_curve, lambda: eng.track_fresh_curve(False)),
                              ("track_link_fresh", eng.track_link_fresh, lambda: eng.track_link_fresh(False)),
                              ("track_mult", eng.track_mult, lambda: eng.track_mult(False)),
                              ("watch", lambda: eng.watch([1, 2]), lambda: eng.watch([]))):
            on()
            with pytest.raises(pkg.GossipError) as e:
                eng.reset()
            assert e.value.status == lib.GP_EINVAL and name in str(e.value) and "delay" in str(e.value), \
                (name, str(e.value))
            off()
        eng.reset()   # the bad dmaxes left the request as it was
        assert eng.link_delay_info() == (True, 4, 11, 0)
        check_delayed(eng, run(eng, inject), ref)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.link_delay(4, 11)
        with pytest.raises(pkg.GossipError) as e:
            eng.reset()
        assert e.value.status == lib.GP_EINVAL and "partition" in str(e.value)
        eng.link_delay(None)
        eng.reset()


def test_shard_job_is_refused_by_name(pkg, oracle):
    """a message-shard job (gp_shard_*): refused at reset() with its name, and a
    transport joined after the reset of a delayed run stops the rounds"""
    g, origin, inject, flood, ref = _ref(4099, 100, 4, 11)
    assert_delays_matter(ref, flood, 4)
    lib = pkg._lib
    with pkg.GossipEngine(0, track_first=1) as eng:   # joined first: the reset refuses
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        eng.shard_host_init(lambda b: [b], 1, 0)   # (records the callback, no collective call)
        assert eng.shard_info() == (1, 0, 2)
        eng.link_delay(4, 11)
        with pytest.raises(pkg.GossipError) as e:
            eng.reset()
        assert e.value.status == lib.GP_EINVAL and "shard" in str(e.value) and "delay" in str(e.value), str(e.value)
        assert eng.link_delay_info() == (False, 1, 0, 0)   # nothing changed: the flood's run goes on
        stats = eng.run()
        assert all(s["mode"] in (0, 1) for s in stats)
        check_run(eng, stats, flood)
        eng.link_delay(None)
        eng.reset()
    with delayed(pkg, g, origin, inject, 4, 11) as eng:   # joined after a delayed reset: the rounds stop
        head = [eng.round() for _ in range(4)]
        flying = eng.link_delay_info()[3]
        assert flying > 0
        first = eng.first()
        eng.shard_host_init(lambda b: [b], 1, 0)
        for _ in range(2):
            with pytest.raises(pkg.GossipError) as e:
                eng.round()
            assert e.value.status == lib.GP_ESTATE and "shard" in str(e.value), str(e.value)
        assert _status(pkg, eng.run) == lib.GP_ESTATE
        # the refused rounds changed nothing, and the lines under way are still counted
        assert eng.link_delay_info() == (True, 4, 11, flying)
        assert np.array_equal(eng.first(), first)
        assert [s["round"] for s in head] == [0, 1, 2, 3]


def test_checkpoint(pkg, oracle):
    """refused with dmax > 1 in force (the lines in flight are not in the blob);
    dmax = 1 saves and continues as a lossy run does"""
    g, origin, inject, flood, ref = _ref(4099, 100, 4, 11)
    assert_delays_matter(ref, flood, 4)
    with delayed(pkg, g, origin, inject, 4, 11) as eng:
        head = [eng.round() for _ in range(3)]
        assert _status(pkg, eng.checkpoint) == pkg._lib.GP_ESTATE
        check_delayed(eng, head + run(eng, inject)[:], ref)   # the refusal changed nothing
    with delayed(pkg, g, origin, inject, 1, 11) as eng:
        head = [eng.round() for _ in range(3)]
        blob = eng.checkpoint()
    with delayed(pkg, g, origin, inject, 1, 11) as eng:
        eng.restore(blob)
        check_flood(eng, head + eng.run(), flood)
        eng.link_delay(4, 11)   # requested: the load would reset into it
        assert _status(pkg, lambda: eng.restore(blob)) == pkg._lib.GP_ESTATE
        # a blob that is none is reported as that, not as a delay problem
        assert _status(pkg, lambda: eng.restore(blob[:16])) == pkg._lib.GP_EINVAL
        assert _status(pkg, lambda: eng.restore(np.zeros_like(blob))) == pkg._lib.GP_EINVAL
