"""The spread curve of a whole message-shard job (gp_read_curve(job = 1) after
gp_shard_combine, csrc/shard.hip step 6) against the oracle's run of the whole
message table.

Messages never interact, so the job's curve is the ranks' curves side by side
at their blocks of the job's message order, ranks that ran fewer rounds
zero-padded.  Ranks run as threads of this process over the host transport
(gp_shard_host_init), as in tests/test_gpu_shard_job.py; the reference is the
histogram of the oracle's first-receipt matrix of the whole table
(Peer.py:175-216: each peer's arrival log), compared exactly, with the same
three sums as tests/test_gpu_curve.py.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BARRIER_S = 20   # a rank left alone in a collective fails the test instead of stalling it
STAT_KEYS = ("injected", "lost", "new_bits", "receivers", "sends", "active")


class Gather:
    """all-gather of byte strings among P threads"""

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


def run_job(pkg, g, origin, inject, blocks, track):
    """One rank per block (rank k holds blocks[k]); track[k]: the rank tracks
    its curve.  Every rank runs to its own quiescence, combines, and reads the
    job record.  Returns [dict per rank]."""
    P, m = len(blocks), len(origin)
    gather = Gather(P)
    engs = []
    for k, (lo, hi) in enumerate(blocks):
        e = pkg.GossipEngine(0)
        e.load_graph(g)
        e.set_message_shard(origin, inject, lo, hi)
        if track[k]:
            e.track_curve()
        e.reset()
        engs.append(e)
    out = [None] * P

    def rank(k):
        try:
            e = engs[k]
            lo, hi = blocks[k]
            e.shard_host_init(gather.fn(k), P, k)
            stats = e.run()
            assert stats[-1]["new_bits"] == 0 and stats[-1]["round"] >= int(inject[lo:hi].max())
            own = e.curve() if track[k] else None
            e.finalize()
            job, _ = e.combine(254)
            res = dict(own_rounds=len(stats), own=own, job=job, cov=e.job_coverage(m))
            try:
                res["curve"] = e.job_curve(m)
            except pkg.GossipError as x:
                res["curve"] = x.status
            out[k] = res
        except BaseException as exc:   # looked at by the caller, after every thread ended
            out[k] = exc

    ts = [threading.Thread(target=rank, args=(k,)) for k in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=3 * BARRIER_S)
    assert not any(t.is_alive() for t in ts), "a rank is stuck in the job"
    for e in engs:
        e.close()
    for r in out:
        if isinstance(r, BaseException):
            raise r
    return out


def histogram(first, rows):
    return np.stack([(first == r).sum(axis=0) for r in range(rows)]).astype(np.uint64)


def check_curve(curve, ref, inject):
    R, m = ref["rounds"], len(inject)
    assert curve.dtype == np.uint64 and curve.shape == (R + 1, m)
    assert np.array_equal(curve, histogram(ref["first"], R + 1))
    for r in range(R + 1):
        assert int(curve[r, inject != r].sum()) == (ref["stats"][r - 1]["new_bits"] if r >= 1 else 0), r
        assert int(curve[r, inject == r].sum()) == (ref["stats"][r]["injected"] if r < R else 0), r
    assert np.array_equal(curve.sum(axis=0), ref["coverage"])


@pytest.fixture(scope="module")
def table(pkg, oracle):
    """229 messages = 3 words + 37: the last block is no multiple of 64.  The
    first 64 messages are injected late (up to round 6), the others in round
    0, so the rank holding them runs rounds the others never see."""
    rp, col = oracle.chung_lu(4099, 8, 2.2, 7)
    g = pkg.CSR(4099, rp, col, False)
    m = 229
    origin = pkg.overlay.random_origins(g.n, m, seed=17)
    inject = np.zeros(m, np.int32)
    inject[:64] = np.arange(64) % 7
    ref = oracle.run(g, origin, inject, want_first=True)
    return g, origin, inject, ref


BLOCKS = {
    "2-ranks": [(0, 128), (128, 229)],
    "4-ranks": [(0, 64), (64, 128), (128, 192), (192, 229)],
    "4-ranks-out-of-order": [(128, 192), (0, 64), (192, 229), (64, 128)],
}


@pytest.mark.parametrize("case", list(BLOCKS))
def test_job_curve_is_the_whole_run(pkg, table, case):
    g, origin, inject, ref = table
    blocks = BLOCKS[case]
    out = run_job(pkg, g, origin, inject, blocks, [True] * len(blocks))
    rounds = [r["own_rounds"] for r in out]
    assert min(rounds) < max(rounds) == ref["rounds"], rounds   # a rank ended rounds earlier
    for k, r in enumerate(out):
        lo, hi = blocks[k]
        assert len(r["job"]) == ref["rounds"]
        for a, b in zip(r["job"], ref["stats"]):
            for key in STAT_KEYS:
                assert a[key] == b[key], (k, key, a["round"])
        assert np.array_equal(r["cov"], ref["coverage"])
        check_curve(r["curve"], ref, inject)
        # the rank's own curve is its block, over its own rounds
        assert np.array_equal(r["own"], r["curve"][:r["own_rounds"] + 1, lo:hi])
        assert not r["curve"][r["own_rounds"] + 1:, lo:hi].any()


@pytest.mark.parametrize("missing", [0, 2])
def test_a_rank_without_a_curve(pkg, table, missing):
    """One rank does not track: no rank has a job curve (GP_ENOTRACK on each),
    and the rest of the job record is what it was."""
    g, origin, inject, ref = table
    blocks = BLOCKS["4-ranks"]
    track = [k != missing for k in range(4)]
    out = run_job(pkg, g, origin, inject, blocks, track)
    for k, r in enumerate(out):
        assert r["curve"] == pkg._lib.GP_ENOTRACK, k
        assert np.array_equal(r["cov"], ref["coverage"])
        assert len(r["job"]) == ref["rounds"]
        for a, b in zip(r["job"], ref["stats"]):
            for key in STAT_KEYS:
                assert a[key] == b[key], (k, key, a["round"])
