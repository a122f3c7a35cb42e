"""The whole-job record of a message-shard run (csrc/shard.hip)
at its edges and through its lifecycle, on the product library.

P ranks run as P threads of this process over the host transport
(gp_shard_host_init): every rank spreads its word-aligned block of the message
table over the whole overlay, stops when its own messages quiesce and joins
gp_shard_combine.  What the reference keeps per peer -- its whole receive
record (Peer.py:175-216, the forward loop at :402-404) -- is then spread over
the ranks, and the job record must equal the oracle's run of the whole table
bit for bit: per-round counters (receivers / active as unions over the
ranks), digest, coverage, forwards, the dead-node reports of the ranks
together, and the same record on every rank.  There are no tolerances here.

The shapes are the smallest that reach the paths the larger shard tests
(tests/rccl_standin_driver.py --shards) never do: a run of more than 64
rounds (the history grows 16 -> 32 -> 64 -> 128), ranks whose runs end 50
rounds apart, an overlay of fewer vertices and bitmap words than ranks,
blocks held out of rank order, jobs that are not one job, and a rank that is
checkpointed and restored inside a job.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAT_KEYS = ("injected", "lost", "new_bits", "receivers", "sends", "active", "crashed",
             "reports", "removals", "dup_reports")
BARRIER_S = 20   # a rank left alone in a collective fails the test instead of stalling it


class HostAllGather:
    """In-process all-gather of byte strings among P threads.  A rank that
    waits alone breaks the barrier after BARRIER_S: its callback raises, the
    engine's transport fails (GP_ERCCL) and the test with it."""

    def __init__(self, P):
        self.parts = [None] * P
        self.bar = threading.Barrier(P, timeout=BARRIER_S)

    def fn(self, k):
        def all_gather(b):
            self.parts[k] = b
            self.bar.wait()
            out = list(self.parts)
            self.bar.wait()
            return out
        return all_gather


class Job:
    """P contexts of one shard job.  blocks[k] = (lo, hi) of rank k (default:
    dist.message_shard); graphs / cfgs / origins may differ per rank for the
    jobs that are not one job."""

    def __init__(self, pkg, g, origin, inject, P, cfg=None, blocks=None, graphs=None, cfgs=None, origins=None):
        self.pkg, self.P, self.m = pkg, P, len(origin)
        self.origin = np.asarray(origin, np.int32)
        self.inject = np.zeros(self.m, np.int32) if inject is None else np.asarray(inject, np.int32)
        self.blocks = blocks or [pkg.dist.message_shard(self.m, P, k) for k in range(P)]
        self.hag = HostAllGather(P)
        self.engs = []
        for k in range(P):
            e = pkg.GossipEngine(0, **(cfgs[k] if cfgs else (cfg or {})))
            e.load_graph(graphs[k] if graphs else g)
            lo, hi = self.blocks[k]
            e.set_message_shard(origins[k] if origins else self.origin, self.inject, lo, hi)
            e.reset()
            self.engs.append(e)

    def last(self, k):
        lo, hi = self.blocks[k]
        return int(self.inject[lo:hi].max())

    def join(self, k):
        self.engs[k].shard_host_init(self.hag.fn(k), self.P, k)
        assert self.engs[k].shard_info() == (self.P, k, 2)

    def run(self, body):
        """body(k, engine) on P threads; [result or exception per rank].  No
        thread may outlive the barrier's timeout by much."""
        out = [None] * self.P

        def rank(k):
            try:
                out[k] = body(k, self.engs[k])
            except BaseException as exc:   # looked at by the caller, after every thread ended
                out[k] = exc

        ts = [threading.Thread(target=rank, args=(k,)) for k in range(self.P)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=3 * BARRIER_S)
        assert not any(t.is_alive() for t in ts), "a rank is stuck in the job"
        return out

    def close(self):
        for e in self.engs:
            e.close()


def rounds_to_quiescence(e, last, stats, reports):
    """gp_round until the rank's own messages quiesce (dist.py's stop rule)."""
    for r in range(len(stats), 254):
        st = e.round()
        assert st["round"] == r
        stats.append(st)
        rep, nrep = e.reports()
        assert nrep == len(rep)
        reports |= set(map(tuple, rep.tolist()))
        if st["new_bits"] == 0 and r >= last:
            return
    raise AssertionError("no quiescence in 254 rounds")


def record(job, e, cap=254):
    """finalize + combine + the job's outputs as this rank holds them."""
    pkg = job.pkg
    e.finalize()
    rounds, _ = e.combine(cap)
    out = dict(job=rounds, cov=e.job_coverage(job.m))
    for name, read in (("digest", e.job_digest), ("fwd", lambda: e.job_forwards(job.m))):
        try:
            out[name] = read()
        except pkg.GossipError as x:
            assert x.status == pkg._lib.GP_ENOTRACK, x
            out[name] = None
    return out


def full_run(job, k, e, cap=254):
    """Rank k's whole life in a job: join, run, combine."""
    job.join(k)
    stats, reports = [], set()
    rounds_to_quiescence(e, job.last(k), stats, reports)
    out = record(job, e, cap)
    out.update(stats=stats, reports=reports)
    return out


def raise_failures(out):
    bad = [(k, repr(o)) for k, o in enumerate(out) if isinstance(o, BaseException)]
    if bad:
        raise AssertionError(f"rank failures: {bad}")


def check_record(out, ref, digest=True, fwd=True):
    """Every rank's job record equals the oracle's whole run and the other
    ranks' record."""
    raise_failures(out)
    for o in out:
        assert len(o["job"]) == ref["rounds"], (len(o["job"]), ref["rounds"])
        for a, b in zip(o["job"], ref["stats"]):
            for key in STAT_KEYS:
                assert a[key] == b[key], (key, a["round"], a[key], b[key])
        if digest:
            assert np.array_equal(o["digest"], ref["digest"])
        else:
            assert o["digest"] is None
        assert np.array_equal(o["cov"], ref["coverage"])
        if fwd:
            assert np.array_equal(o["fwd"], ref["forwards"])
        assert o["job"] == out[0]["job"], "the ranks hold different records"
    if "reports" in out[0]:
        reports = set().union(*(o["reports"] for o in out))
        assert reports == set(map(tuple, ref["reports"].tolist()))


def statuses(out):
    return [o.status if hasattr(o, "status") else o for o in out]


def expect_status(pkg, out, status):
    """Every rank failed with `status` (and none with a broken transport)."""
    assert all(isinstance(o, pkg.GossipError) for o in out), out
    assert statuses(out) == [status] * len(out), [repr(o) for o in out]


# ---------------------------------------------------------------------------
# overlays and their oracle runs, computed once

def _ring_edges():
    return [(i, (i + 1) % 131) for i in range(131)]


@pytest.fixture(scope="module")
def ring(pkg, oracle):
    """A ring of 131 vertices x 130 messages: 68 rounds."""
    g = pkg.CSR.from_edges(131, _ring_edges())
    origin = pkg.overlay.random_origins(131, 130, seed=7)
    inject = (np.arange(130) % 3).astype(np.int32)
    return g, origin, inject, oracle.run(g, origin, inject)


@pytest.fixture(scope="module")
def ring_path(pkg):
    """n = 134 (n % 64 != 0, 3 bitmap words): the ring and the path
    131-132-133; messages 0-63 start on the path, 64-129 on the ring."""
    g = pkg.CSR.from_edges(134, _ring_edges() + [(131, 132), (132, 133)])
    rng = np.random.Generator(np.random.PCG64(11))
    origin = np.concatenate([rng.integers(131, 134, 64), rng.integers(0, 131, 66)]).astype(np.int32)
    return g, origin, (np.arange(130) % 3).astype(np.int32)


@pytest.fixture(scope="module")
def ba(pkg):
    g = pkg.overlay.barabasi_albert(3001, 2, seed=8)
    origin = pkg.overlay.random_origins(g.n, 200, seed=8)
    return g, origin


@pytest.fixture(scope="module")
def ba_ref(ba, oracle):
    g, origin = ba
    return oracle.run(g, origin, None)


BA_CHURN = dict(churn=True, p_fail=0.02, churn_seed=3)


@pytest.fixture(scope="module")
def ba4(ba, oracle):
    """BA(3001, 2) x 200 at the reference cadence of 4 inject rounds: the whole
    table's run and each P = 2 block's own run, without and with churn."""
    g, origin = ba
    inject = (np.arange(200) % 4).astype(np.int32)
    refs = {}
    for churn in (False, True):
        kw = BA_CHURN if churn else {}
        refs[churn] = dict(whole=oracle.run(g, origin, inject, **kw),
                           blocks=[oracle.run(g, origin[lo:hi], inject[lo:hi], want_first=True, **kw)
                                   for lo, hi in ((0, 128), (128, 200))])
    return g, origin, inject, refs


def ba4_cfg(churn):
    if not churn:
        return dict(track_first=1)
    return dict(track_first=1, track_msg_forwards=1, churn=1, p_fail=0.02, churn_seed=3)


@pytest.fixture(scope="module")
def chung_lu(pkg, oracle):
    rp, col = oracle.chung_lu(60_000, 12, 2.4, 43)
    return pkg.CSR(60_000, rp, col, False)


# ---------------------------------------------------------------------------
# the record at its edges

@pytest.mark.timeout(120)
@pytest.mark.parametrize("P", [1, 2, 3])
def test_history_growth(pkg, ring, P):
    """68 rounds on every rank: the per-round bitmap history (16 rounds at
    first) doubles three times, each time copying the rounds recorded so far.
    A wrong copy length or stride shows as wrong receivers / active."""
    g, origin, inject, ref = ring
    assert ref["rounds"] > 64
    job = Job(pkg, g, origin, inject, P)
    out = job.run(lambda k, e: full_run(job, k, e))
    job.close()
    check_record(out, ref)
    assert all(len(o["stats"]) > 64 for o in out)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("churn", [False, True])
def test_unequal_runs(pkg, oracle, ring_path, churn):
    """Rank 0's messages live on a 3-vertex path and quiesce in 5 rounds (3
    under churn), rank 1's take the ring's 68 (60): rank 0's history never
    grows, its rounds past its own read as zero bitmaps (k_shard_pack) and as
    rounds it did not run (F_RAN), and the liveness counters of the late rounds
    come from rank 1 alone."""
    g, origin, inject = ring_path
    kw = dict(churn=True, p_fail=0.004, churn_seed=5) if churn else {}
    cfg = dict(churn=1, p_fail=0.004, churn_seed=5, track_msg_forwards=1) if churn else {}
    ref = oracle.run(g, origin, inject, **kw)
    job = Job(pkg, g, origin, inject, 2, cfg)
    assert job.blocks == [(0, 64), (64, 130)]
    out = job.run(lambda k, e: full_run(job, k, e))
    job.close()
    check_record(out, ref)
    own = [len(o["stats"]) for o in out]
    assert abs(own[0] - own[1]) > 16 and min(own) < 16 < max(own), own
    assert max(own) == ref["rounds"]
    if churn:
        assert sum(s["removals"] for s in ref["stats"]) > 0


@pytest.mark.timeout(120)
@pytest.mark.parametrize("P", [4, 8])
def test_overlay_smaller_than_the_job(pkg, oracle, P):
    """5 vertices (one isolated), 502 messages: one bitmap word for P ranks
    (ranks past 0 hold an empty slice of the OR reduce-scatter and launch no
    k_shard_union) and, at P = 8, digest slices of one vertex with ranks 5-7
    empty (their zero-word sends and receives are skipped on both sides)."""
    g = pkg.CSR.from_edges(5, [(0, 1), (1, 2), (2, 3)])
    origin = pkg.overlay.random_origins(5, 502, seed=3)
    ref = oracle.run(g, origin, None)
    assert ref["rounds"] == 4
    job = Job(pkg, g, origin, None, P)
    out = job.run(lambda k, e: full_run(job, k, e))
    job.close()
    check_record(out, ref)


@pytest.mark.timeout(120)
def test_blocks_out_of_rank_order(pkg, ba, ba_ref):
    """Rank 0 holds messages [128, 200), rank 1 [0, 128): the record is in
    table order whatever rank holds which block."""
    g, origin = ba
    job = Job(pkg, g, origin, None, 2, blocks=[(128, 200), (0, 128)])
    out = job.run(lambda k, e: full_run(job, k, e))
    job.close()
    check_record(out, ref=ba_ref)


@pytest.mark.timeout(120)
def test_job_without_digests(pkg, ba, ba_ref):
    """track_digest = 0: the combine skips the XOR reduce-scatter; counters,
    coverage and forwards equal the oracle's, the job's digest is not tracked."""
    g, origin = ba
    job = Job(pkg, g, origin, None, 2, dict(track_digest=0))
    out = job.run(lambda k, e: full_run(job, k, e))
    raise_failures(out)
    for e in job.engs:
        with pytest.raises(pkg.GossipError) as x:
            e.job_digest()
        assert x.value.status == pkg._lib.GP_ENOTRACK
    job.close()
    check_record(out, ba_ref, digest=False)


@pytest.mark.timeout(120)
def test_job_reads_outside_a_record(pkg, ba, ba_ref):
    """The job's outputs exist between a combine and the next gp_reset only."""
    g, origin = ba
    job = Job(pkg, g, origin, None, 1)
    e = job.engs[0]
    job.join(0)

    def refused():
        for read in (e.job_digest, lambda: e.job_coverage(job.m)):
            with pytest.raises(pkg.GossipError) as x:
                read()
            assert x.value.status == pkg._lib.GP_ESTATE

    refused()
    stats, reports = [], set()
    rounds_to_quiescence(e, 0, stats, reports)
    refused()
    out = record(job, e)
    check_record([out], ba_ref)
    e.reset()
    refused()
    job.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", ["same_block", "gap", "other_overlay", "other_churn_seed"])
def test_jobs_that_are_not_one_job(pkg, ba, case):
    """Ranks whose runs do not make one job fail the combine with GP_EINVAL on
    every rank (all of them check the same all-gathered headers), and none
    waits for another."""
    g, origin = ba
    kw = {}
    if case == "same_block":
        kw["blocks"] = [(0, 128), (0, 128)]
    elif case == "gap":
        kw["blocks"] = [(0, 100), (128, 200)]
    elif case == "other_overlay":
        g1 = pkg.overlay.barabasi_albert(3000, 2, seed=8)
        kw["graphs"] = [g, g1]
        kw["origins"] = [origin, np.minimum(origin, g1.n - 1)]
    else:
        kw["cfgs"] = [dict(churn=1, p_fail=0.02, churn_seed=s) for s in (3, 4)]
    job = Job(pkg, g, origin, None, 2, **kw)
    out = job.run(lambda k, e: full_run(job, k, e))
    job.close()
    expect_status(pkg, out, pkg._lib.GP_EINVAL)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("caps", [(2, 2), (254, 2)])
def test_cap_below_the_jobs_rounds(pkg, ba, ba_ref, caps):
    """A caller's buffer shorter than the job's rounds fails the combine on
    every rank, whichever rank passed it: the ranks exchange their caps in the
    header, so the one with room does not go on into a collective alone."""
    g, origin = ba
    assert ba_ref["rounds"] > 2
    job = Job(pkg, g, origin, None, 2)
    out = job.run(lambda k, e: full_run(job, k, e, cap=caps[k]))
    expect_status(pkg, out, pkg._lib.GP_EINVAL)
    # the same contexts, with room: the record
    out = job.run(lambda k, e: record(job, e))
    job.close()
    check_record(out, ba_ref)


@pytest.mark.timeout(120)
def test_a_context_reused_on_a_larger_overlay(pkg, ba, ba_ref):
    """The history is sized by the overlay: contexts that recorded a job on 5
    vertices record the next one on 3001 in a history allocated for it."""
    g, origin = ba
    small = pkg.CSR.from_edges(5, [(0, 1), (1, 2), (2, 3)])
    job = Job(pkg, small, pkg.overlay.random_origins(5, 200, seed=3), None, 2)
    raise_failures(job.run(lambda k, e: full_run(job, k, e)))
    job.origin = np.asarray(origin, np.int32)
    for k, e in enumerate(job.engs):
        e.load_graph(g)
        e.set_message_shard(origin, None, *job.blocks[k])
        e.reset()
    out = job.run(lambda k, e: full_run(job, k, e))
    job.close()
    check_record(out, ba_ref)


# ---------------------------------------------------------------------------
# lifecycle: checkpoints and late transports inside a job

def check_own_outputs(job, k, e, stats, ref, from_round):
    """Rank k's own outputs equal the oracle's run of its block alone."""
    lo, _ = job.blocks[k]
    assert len(stats) == ref["rounds"], (k, len(stats), ref["rounds"])
    for a, b in zip(stats[from_round:], ref["stats"][from_round:]):
        for key in STAT_KEYS:
            assert a[key] == b[key], (k, key, a["round"], a[key], b[key])
    assert np.array_equal(e.seen(), ref["seen"][:, :e.words])
    assert np.array_equal(e.first(), ref["first"])
    assert np.array_equal(e.coverage(), ref["coverage"])
    assert np.array_equal(e.forwards(), ref["forwards"])
    if lo == 0:   # (the oracle numbers a block's words from 0)
        assert np.array_equal(e.digest(), ref["digest"])
    return e.digest()


def combine_status(pkg, e):
    try:
        e.combine()
    except pkg.GossipError as x:
        return x.status
    return 0


@pytest.mark.timeout(120)
@pytest.mark.parametrize("churn", [False, True])
@pytest.mark.parametrize("restored", ["both", "rank1"])
def test_restore_inside_a_shard_job(pkg, ba4, churn, restored):
    """A shard rank is checkpointed after round 2 and restored: its rounds go
    on and its own outputs stay exact; the job record needs every rank's run
    complete since gp_reset, so gp_shard_combine fails with GP_ESTATE on every
    rank -- also on the one that was not restored.  After gp_reset the same
    contexts run and combine the whole job."""
    g, origin, inject, refs = ba4
    whole, blocks = refs[churn]["whole"], refs[churn]["blocks"]
    job = Job(pkg, g, origin, inject, 2, ba4_cfg(churn))

    def body(k, e):
        job.join(k)
        stats, reports = [], set()
        for _ in range(2):
            stats.append(e.round())
        if restored == "both" or k == 1:
            blob = e.checkpoint()
            e.restore(blob)
        rounds_to_quiescence(e, job.last(k), stats, reports)
        e.finalize()
        dg = check_own_outputs(job, k, e, stats, blocks[k], 2)
        return dict(digest=dg, status=combine_status(pkg, e))

    out = job.run(body)
    raise_failures(out)
    assert [o["status"] for o in out] == [pkg._lib.GP_ESTATE] * 2
    assert np.array_equal(out[0]["digest"] ^ out[1]["digest"], whole["digest"])
    for e in job.engs:   # no record behind a refused combine
        with pytest.raises(pkg.GossipError) as x:
            e.job_coverage(job.m)
        assert x.value.status == pkg._lib.GP_ESTATE

    def again(k, e):
        e.reset()
        return full_run(job, k, e)

    out = job.run(again)
    job.close()
    check_record(out, whole)


@pytest.mark.timeout(120)
def test_restore_at_round_zero_keeps_the_record(pkg, ba4):
    """A checkpoint taken right after gp_reset and loaded back at once leaves
    the run complete: the combine refuses no more than it has to."""
    g, origin, inject, refs = ba4
    job = Job(pkg, g, origin, inject, 2, ba4_cfg(False))

    def body(k, e):
        job.join(k)
        e.restore(e.checkpoint())
        stats, reports = [], set()
        rounds_to_quiescence(e, job.last(k), stats, reports)
        out = record(job, e)
        out.update(stats=stats, reports=reports)
        return out

    out = job.run(body)
    job.close()
    check_record(out, refs[False]["whole"])


@pytest.mark.timeout(120)
def test_transport_joined_in_mid_run(pkg, ba4):
    """gp_shard_host_init after round 2: the rounds before it were not
    recorded, so the rounds go on (exact) and the combine refuses."""
    g, origin, inject, refs = ba4
    whole, blocks = refs[False]["whole"], refs[False]["blocks"]
    job = Job(pkg, g, origin, inject, 2, ba4_cfg(False))

    def body(k, e):
        stats, reports = [], set()
        for _ in range(2):
            stats.append(e.round())
        job.join(k)
        rounds_to_quiescence(e, job.last(k), stats, reports)
        e.finalize()
        dg = check_own_outputs(job, k, e, stats, blocks[k], 0)
        return dict(digest=dg, status=combine_status(pkg, e))

    out = job.run(body)
    job.close()
    raise_failures(out)
    assert [o["status"] for o in out] == [pkg._lib.GP_ESTATE] * 2
    assert np.array_equal(out[0]["digest"] ^ out[1]["digest"], whole["digest"])


# ---------------------------------------------------------------------------
# aliased receivers in the job's counters

ALIAS_CFG = dict(push_ratio=0.0, compact_rows=0, arc_mask_permille=0)


@pytest.mark.timeout(120)
def test_aliased_in_the_job_record_one_rank(pkg, oracle, chung_lu):
    """W = 64 early-exit rounds commit completed receivers as aliases of their
    component row: rows_written leaves them out, `aliased`
    counts them, and the job record carries both as the rank counted them."""
    g = chung_lu
    origin = pkg.overlay.random_origins(g.n, 4096, seed=43)
    ref = oracle.run(g, origin, None)
    job = Job(pkg, g, origin, None, 1, ALIAS_CFG)
    out = job.run(lambda k, e: full_run(job, k, e))
    job.close()
    check_record(out, ref)
    o = out[0]
    assert sum(s["aliased"] for s in o["stats"]) > 0, "precondition: no aliasing at this shape"
    assert sum(r["aliased"] for r in o["job"]) > 0
    for a, b in zip(o["job"], o["stats"]):
        assert a["aliased"] == b["aliased"], (a["round"], a["aliased"], b["aliased"])
        assert a["rows_written"] == b["rows_written"], a["round"]


@pytest.mark.timeout(120)
def test_aliased_in_the_job_record_two_ranks(pkg, oracle, chung_lu):
    """Two ranks of 4096 messages each (aliasing needs W = 64 per rank): the
    job's aliased / rows_written are the sums over the ranks, round by round;
    the additive counters, coverage and forwards are those of the two blocks'
    oracle runs (the oracle runs at most 4096 messages at once)."""
    g = chung_lu
    origin = pkg.overlay.random_origins(g.n, 8192, seed=43)
    refs = [oracle.run(g, origin[lo:hi], None, nthreads=4) for lo, hi in ((0, 4096), (4096, 8192))]
    job = Job(pkg, g, origin, None, 2, ALIAS_CFG)
    assert job.blocks == [(0, 4096), (4096, 8192)]
    out = job.run(lambda k, e: full_run(job, k, e))
    job.close()
    raise_failures(out)
    assert all(sum(s["aliased"] for s in o["stats"]) > 0 for o in out), "precondition: no aliasing at this shape"
    R = max(r["rounds"] for r in refs)
    for k, o in enumerate(out):
        assert len(o["stats"]) == refs[k]["rounds"]
        assert o["job"] == out[0]["job"]
        assert len(o["job"]) == R
        assert np.array_equal(o["cov"], np.concatenate([r["coverage"] for r in refs]))
        assert np.array_equal(o["fwd"], np.concatenate([r["forwards"] for r in refs]))
    for r, row in enumerate(out[0]["job"]):
        for key in ("aliased", "rows_written"):
            assert row[key] == sum(o["stats"][r][key] for o in out if r < len(o["stats"])), (key, r)
        for key in ("injected", "lost", "new_bits", "sends"):
            assert row[key] == sum(x["stats"][r][key] for x in refs if r < x["rounds"]), (key, r)
