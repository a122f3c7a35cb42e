"""GossipEngine: host driver of the MI355X gossip hot path over the C-ABI.

Replaces, for all peers at once, the reference's per-peer threads:
gossip_sender (Peer.py:395-408), the receive handlers (Peer.py:175-216,
258-296), the heartbeat monitor (Peer.py:298-393) and the seed's dead-node
removal (Seed.py:358-406).  One `round()` = liveness + injection + pull
expansion (+ RCCL exchange on multi-GPU), all on the device.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import check


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class GossipEngine:
    def __init__(self, device=0, **config):
        self._lib = _lib.load()
        self._ctx = ctypes.c_void_p()
        check(self._lib.gp_create(int(device), ctypes.byref(self._ctx)))
        self.device = device
        self.cfg = _lib.Config()
        self._lib.gp_default_config(ctypes.byref(self.cfg))
        self.n = 0
        self.m = 0
        self.words = 0
        self.origin = None
        self.inject_round = None
        self.nranks = 1
        if config:
            self.configure(**config)

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if self._ctx:
            self._lib.gp_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def configure(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.cfg, k):
                raise KeyError(f"unknown config field {k}")
            setattr(self.cfg, k, v)
        check(self._lib.gp_configure(self._ctx, ctypes.byref(self.cfg)))

    # -- overlay -----------------------------------------------------------
    def load_graph(self, csr, out_csr=None):
        """out_csr=(out_row_ptr, out_col): the out-CSR of a directed overlay
        (the transpose of csr, rows in any order); None lets gp_load_graph
        transpose the in-CSR itself."""
        rp = np.ascontiguousarray(csr.row_ptr, dtype=np.int64)
        col = np.ascontiguousarray(csr.col, dtype=np.int32)
        orp = ocol = None
        if out_csr is not None:
            if not csr.directed:
                raise ValueError("an out-CSR goes with a directed overlay")
            orp = np.ascontiguousarray(out_csr[0], dtype=np.int64)
            ocol = np.ascontiguousarray(out_csr[1], dtype=np.int32)
            if orp.shape != rp.shape or ocol.shape != col.shape:
                raise ValueError("out-CSR and in-CSR differ in size")
        check(self._lib.gp_load_graph(self._ctx, int(csr.n), int(col.size), _ptr(rp), _ptr(col),
                                      1 if csr.directed else 0, _ptr(orp), _ptr(ocol)))
        self.n = int(csr.n)

    def build_chung_lu(self, n, dbar, gamma, seed):
        check(self._lib.gp_build_chung_lu(self._ctx, int(n), float(dbar), float(gamma), int(seed)))
        self.n = int(n)

    def graph(self):
        """The overlay as loaded / built (global CSR).  A partitioned context
        keeps only its local CSR: see local_graph()."""
        from .overlay import CSR
        if self.nranks > 1:
            raise RuntimeError("a partitioned context holds its local CSR only (local_graph())")
        n, nnz = self.info()[:2]
        rp = np.empty(n + 1, dtype=np.int64)
        col = np.empty(nnz, dtype=np.int32)
        check(self._lib.gp_read(self._ctx, _lib.ROW_PTR, _ptr(rp), rp.nbytes))
        check(self._lib.gp_read(self._ctx, _lib.COL, _ptr(col), col.nbytes))
        return CSR(n, rp, col, False)

    def local_info(self):
        """(nloc, nghost, nextra, nnz_local, n_boundary) of this context."""
        v = [ctypes.c_int64() for _ in range(5)]
        check(self._lib.gp_local_info(self._ctx, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def local_graph(self):
        """(row_ptr, col, l2g) of the context's local CSR: owned vertices
        [0, nloc) with their full in-lists, ghosts with their owned neighbours,
        origin extras with none; l2g maps local ids to global ids."""
        nloc, ng, nx, nnz_l, _ = self.local_info()
        nv = nloc + ng + nx if self.nranks > 1 else self.n
        rp = self._read(_lib.ROW_PTR, np.empty(nv + 1, dtype=np.int64))
        col = self._read(_lib.COL, np.empty(nnz_l, dtype=np.int32))
        l2g = self._read(_lib.L2G, np.empty(nv, dtype=np.int32))
        return rp, col, l2g

    def degrees(self):
        """Degree of every vertex of the loaded overlay (in-degree of the
        in-CSR; = degree for undirected overlays), from row_ptr alone."""
        if self.nranks > 1:
            raise RuntimeError("degrees() needs the global overlay (check it before partitioning)")
        n = self.info()[0]
        rp = np.empty(n + 1, dtype=np.int64)
        check(self._lib.gp_read(self._ctx, _lib.ROW_PTR, _ptr(rp), rp.nbytes))
        return np.diff(rp)

    def check_degree(self, gamma, tol=0.15):
        """SURVEY.md §8a A9 on the overlay this context holds: discrete MLE
        gamma_hat with KS-chosen kmin against the generator's gamma (the
        reference's intent, degree-weighted selection, demonstrate_powerlaw.py:19-27)."""
        from . import degree
        return degree.check_powerlaw(self.degrees(), gamma, tol)

    def info(self):
        n, nnz = ctypes.c_int64(), ctypes.c_int64()
        m, w = ctypes.c_int32(), ctypes.c_int32()
        check(self._lib.gp_info(self._ctx, ctypes.byref(n), ctypes.byref(nnz), ctypes.byref(m), ctypes.byref(w)))
        return n.value, nnz.value, m.value, w.value

    # -- partition / RCCL --------------------------------------------------
    def set_partition(self, rank, nranks):
        """Vertex partition: keep the owned slice of rank `rank`
        of `nranks` plus ghost rows; nranks > 1 drops the global CSR and the
        message table (set_messages again, in global ids)."""
        check(self._lib.gp_set_partition(self._ctx, int(rank), int(nranks)))
        self.nranks = int(nranks)
        if nranks > 1:
            self.m = self.words = 0

    def partition(self):
        b, e = ctypes.c_int64(), ctypes.c_int64()
        check(self._lib.gp_get_partition(self._ctx, ctypes.byref(b), ctypes.byref(e)))
        return b.value, e.value

    @staticmethod
    def comm_unique_id():
        buf = ctypes.create_string_buffer(128)
        check(_lib.load().gp_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, nranks, rank):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(self._lib.gp_comm_init(self._ctx, buf, int(nranks), int(rank)))

    # -- message-shard jobs (csrc/shard.hip) -----------------
    def shard_comm_init(self, unique_id, nranks, rank):
        """Join an nranks-rank message-shard job over RCCL (one GPU per rank;
        rank 0 makes the id with comm_unique_id())."""
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(self._lib.gp_shard_comm_init(self._ctx, buf, int(nranks), int(rank)))

    def shard_host_init(self, all_gather_bytes, nranks, rank):
        """Join a message-shard job whose combine moves its chunks through the
        host: all_gather_bytes(bytes) -> [bytes of rank 0, ..., rank nranks-1]
        (ranks sharing a GPU, which RCCL refuses)."""
        def fn(_user, send, nbytes, recv):
            try:
                parts = all_gather_bytes(ctypes.string_at(send, nbytes))
                if len(parts) != nranks or any(len(p) != nbytes for p in parts):
                    return -1
                ctypes.memmove(recv, b"".join(parts), nranks * nbytes)
                return 0
            except Exception:   # (a C caller cannot take a Python exception)
                return -1
        self._shard_cb = _lib.AllGatherFn(fn)   # kept alive as long as the context
        check(self._lib.gp_shard_host_init(self._ctx, self._shard_cb, None, int(nranks), int(rank)))

    def shard_info(self):
        """(nranks, rank, transport) as the job's transport reports them:
        ncclCommCount / ncclCommUserRank for RCCL (transport 1), the host
        all-gather's (2), or (0, 0, 0) outside a shard job."""
        v = [ctypes.c_int32() for _ in range(3)]
        check(self._lib.gp_shard_info(self._ctx, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def combine(self, max_rounds=254):
        """gp_shard_combine after run(): the job's per-round counters (list of
        dicts, every rank the same) and the combine's device time in ms.  The
        job's digest / coverage / forwards are then job_digest() etc."""
        buf = (_lib.RoundStats * max_rounds)()
        k = ctypes.c_int32()
        ms = ctypes.c_double()
        check(self._lib.gp_shard_combine(self._ctx, buf, int(max_rounds), ctypes.byref(k), ctypes.byref(ms)))
        return [buf[i].as_dict() for i in range(k.value)], ms.value

    def job_digest(self):
        return self._read(_lib.JOB_DIGEST, np.empty(self.n, dtype=np.uint64))

    def job_coverage(self, m_total):
        return self._read(_lib.JOB_COVERAGE, np.empty(int(m_total), dtype=np.uint64))

    def job_forwards(self, m_total):
        return self._read(_lib.JOB_FORWARDS, np.empty(int(m_total), dtype=np.uint64))

    # -- messages / run ----------------------------------------------------
    def set_messages(self, origin, inject_round=None):
        o = np.ascontiguousarray(origin, dtype=np.int32)
        r = None if inject_round is None else np.ascontiguousarray(inject_round, dtype=np.int32)
        if r is not None and r.shape != o.shape:
            raise ValueError("origin and inject_round differ in length")
        check(self._lib.gp_set_messages(self._ctx, int(o.size), _ptr(o), _ptr(r)))
        self.origin = o
        self.inject_round = r if r is not None else np.zeros_like(o)
        _, _, self.m, self.words = self.info()

    def spread_keys(self, origin, hops=2):
        """gp_spread_keys: arc endpoints within `hops` of each origin (the
        global overlay; call before a vertex partition)."""
        o = np.ascontiguousarray(origin, dtype=np.int32)
        keys = np.zeros(o.size, np.uint64)
        check(self._lib.gp_spread_keys(self._ctx, int(hops), int(o.size), _ptr(o), _ptr(keys)))
        return keys

    def spread_order(self, origin, inject_round=None, hops=2):
        """Permutation p that orders a message table by spread speed
        (overlay.spread_order): run origin[p] (and inject_round[p]); per-message
        outputs of that run are those of message p[k] at index k."""
        from .overlay import spread_order
        return spread_order(self.spread_keys(origin, hops), inject_round)

    def set_message_shard(self, origin, inject_round, lo, hi):
        """Take messages [lo, hi) of a larger message table as this context's
        shard: local message k is global message lo + k.  lo must
        be word aligned so that digests of the shards XOR into the digest of
        the whole table, and first/coverage/forwards concatenate."""
        if lo % 64:
            raise ValueError("message shards start on a 64-message word boundary")
        self.configure(msg_word_base=lo // 64)
        r = None if inject_round is None else np.asarray(inject_round)[lo:hi]
        self.set_messages(np.asarray(origin)[lo:hi], r)

    def reset(self):
        check(self._lib.gp_reset(self._ctx))

    def crash(self, verts):
        v = np.ascontiguousarray(verts, dtype=np.int32)
        check(self._lib.gp_crash(self._ctx, int(v.size), _ptr(v)))

    def round(self):
        st = _lib.RoundStats()
        check(self._lib.gp_round(self._ctx, ctypes.byref(st)))
        return st.as_dict()

    @staticmethod
    def round_group(engines):
        """One round over single-process contexts engines[k] owning partition k
        (device-to-device exchange, no RCCL); returns the summed counters."""
        arr = (ctypes.c_void_p * len(engines))(*[e._ctx.value for e in engines])
        st = _lib.RoundStats()
        check(_lib.load().gp_round_group(arr, len(engines), ctypes.byref(st)))
        return st.as_dict()

    @staticmethod
    def run_group(engines, max_rounds=254):
        out = []
        last = max(int(engines[0].inject_round.max()), 0) if engines[0].m else -1
        for _ in range(max_rounds):
            st = GossipEngine.round_group(engines)
            out.append(st)
            if st["new_bits"] == 0 and st["round"] >= last:
                break
        return out

    def run(self, max_rounds=254):
        buf = (_lib.RoundStats * max_rounds)()
        k = ctypes.c_int32()
        check(self._lib.gp_run(self._ctx, int(max_rounds), buf, ctypes.byref(k)))
        return [buf[i].as_dict() for i in range(k.value)]

    def synchronize(self):
        check(self._lib.gp_synchronize(self._ctx))

    # -- checkpoints ----------------------------------
    def checkpoint(self):
        """The context's whole per-run state between rounds, as an opaque
        uint8 blob (gp_checkpoint_save)."""
        nb = ctypes.c_int64()
        check(self._lib.gp_checkpoint_size(self._ctx, ctypes.byref(nb)))
        blob = np.empty(nb.value, dtype=np.uint8)
        check(self._lib.gp_checkpoint_save(self._ctx, _ptr(blob), blob.nbytes))
        return blob

    def restore(self, blob):
        """Continue the run a checkpoint() blob captured: same overlay,
        messages, partition and tracked outputs (gp_checkpoint_load)."""
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        check(self._lib.gp_checkpoint_load(self._ctx, _ptr(b), b.nbytes))

    def save_checkpoint(self, path):
        """Write the checkpoint() blob to `path` as a .npy file, straight into a
        memory map of the file: host memory stays bounded by the page cache
        even for the 32 GiB of Message-List rows of a 2^26 x 4096 run.  The
        blob goes to `path`.tmp first and replaces `path` only once it is
        complete, so a failed save leaves the previous checkpoint intact."""
        nb = ctypes.c_int64()
        check(self._lib.gp_checkpoint_size(self._ctx, ctypes.byref(nb)))
        path = os.fspath(path)
        tmp = path + ".tmp"
        out = np.lib.format.open_memmap(tmp, mode="w+", dtype=np.uint8, shape=(nb.value,))
        ok = False
        try:
            check(self._lib.gp_checkpoint_save(self._ctx, _ptr(out), out.nbytes))
            out.flush()
            ok = True
        finally:
            del out
            if not ok:
                try:
                    os.unlink(tmp)
                except OSError:
                    pass
        os.replace(tmp, path)

    def load_checkpoint(self, path):
        """Restore a save_checkpoint() file (memory-mapped, read-only).  The
        blob's header names its overlay, messages, partition and tracked
        outputs; a mismatch raises and leaves the current run untouched."""
        blob = np.load(path, mmap_mode="r", allow_pickle=False)
        try:
            if blob.dtype != np.uint8 or blob.ndim != 1:
                raise ValueError(f"{path}: not a gossip checkpoint")
            check(self._lib.gp_checkpoint_load(self._ctx, ctypes.c_void_p(blob.ctypes.data), blob.nbytes))
        finally:
            del blob

    # -- outputs -----------------------------------------------------------
    def _read(self, what, arr):
        check(self._lib.gp_read(self._ctx, what, _ptr(arr), arr.nbytes))
        return arr

    def nloc(self):
        b, e = self.partition()
        return e - b

    def seen(self):
        return self._read(_lib.SEEN, np.empty((self.nloc(), self.words), dtype=np.uint64))

    def first(self):
        return self._read(_lib.FIRST, np.empty((self.nloc(), self.m), dtype=np.uint8))

    def digest(self):
        return self._read(_lib.DIGEST, np.empty(self.nloc(), dtype=np.uint64))

    def finalize(self):
        """gp_finalize_messages: coverage() and forwards() of the run so far.
        After a run that stopped before quiescence (the 254-round limit, a
        caller that stops early) the last round's receivers have not sent:
        forwards() leaves their sends out, and raises GP_ENOTRACK on a context
        that keeps neither frontier rows nor track_msg_forwards."""
        check(self._lib.gp_finalize_messages(self._ctx))

    def coverage(self):
        return self._read(_lib.COVERAGE, np.empty(self.m, dtype=np.uint64))

    def forwards(self):
        return self._read(_lib.FORWARDS, np.empty(self.m, dtype=np.uint64))

    # -- spread curves (csrc/curve.hip; helpers in spread.py) ----------------
    def track_curve(self, on=True):
        """gp_track_curve: count first receipts per (receipt round, message)
        from the next reset() on."""
        check(self._lib.gp_track_curve(self._ctx, 1 if on else 0))

    def _read_curve(self, job, m):
        buf = np.zeros((255, int(m)), dtype=np.uint64)   # receipt rounds 0 .. 254
        rows = ctypes.c_int32()
        check(self._lib.gp_read_curve(self._ctx, job, _ptr(buf), buf.shape[0], ctypes.byref(rows)))
        return buf[:rows.value].copy()

    def curve(self):
        """u64 [rounds run + 1][m]: curve[r][k] = owned vertices whose first
        receipt of message k has receipt round r (an origin's own receipt at
        its inject round included) -- the column histograms of first().  With
        spread_order's permutation p the columns are those of message p[k], as
        for coverage()."""
        return self._read_curve(0, self.m)

    def job_curve(self, m_total):
        """The whole shard job's curve after combine(): u64 [job rounds + 1][m_total]."""
        return self._read_curve(1, m_total)

    # -- per-peer traffic record (csrc/load.hip; helpers in load.py) --------
    def track_load(self, on=True):
        """gp_track_load: keep the gossip lines every peer sent and received
        (duplicates included) from the next reset() on."""
        check(self._lib.gp_track_load(self._ctx, 1 if on else 0))

    def load_sent(self):
        """u64 [n]: lines peer u put on the wire since reset(), over all its
        links; sums to the rounds' `sends`."""
        return self._read(_lib.LOAD_SENT, np.empty(self.n, dtype=np.uint64))

    def load_recv(self):
        """u64 [n]: lines that arrived at peer v since reset(), duplicates
        included (load.duplicates turns them into duplicates alone)."""
        return self._read(_lib.LOAD_RECV, np.empty(self.n, dtype=np.uint64))

    def seenpop(self):
        """u32 per owned vertex: |Message-List(v)|, the messages v holds."""
        return self._read(_lib.SEENPOP, np.empty(self.nloc(), dtype=np.uint32))

    # -- per-peer fresh deliveries (csrc/fresh.hip; helpers in redundancy.py) --
    def track_fresh(self, on=True):
        """gp_track_fresh: keep, per peer, the sends and arrivals that carried
        a first receipt from the next reset() on."""
        check(self._lib.gp_track_fresh(self._ctx, 1 if on else 0))

    def fresh_sent(self):
        """u64 [n]: peer u's sends since reset() that delivered a message the
        receiver did not hold (load_sent() - fresh_sent(): its wasted sends)."""
        return self._read(_lib.FRESH_SENT, np.empty(self.n, dtype=np.uint64))

    def fresh_recv(self):
        """u64 [n]: arrivals at peer v since reset() of a message it did not
        hold at the start of the round (load_recv() - fresh_recv(): its stale
        arrivals)."""
        return self._read(_lib.FRESH_RECV, np.empty(self.n, dtype=np.uint64))

    # -- fresh-delivery curves (csrc/fresh_curve.hip; helpers in redundancy.py) --
    def track_fresh_curve(self, on=True):
        """gp_track_fresh_curve: count, per (receipt round, message), the sends
        that delivered a first receipt from the next reset() on."""
        check(self._lib.gp_track_fresh_curve(self._ctx, 1 if on else 0))

    def fresh_curve(self):
        """u64 [rounds run + 1][m]: fresh_curve[R][k] = the sends of message k
        in round R - 1 that delivered a first receipt (row 0 is zero), the
        deliverers behind curve()[R][k]; the columns are curve()'s."""
        buf = np.zeros((255, int(self.m)), dtype=np.uint64)   # receipt rounds 0 .. 254
        rows = ctypes.c_int32()
        check(self._lib.gp_read_fresh_curve(self._ctx, _ptr(buf), buf.shape[0], ctypes.byref(rows)))
        return buf[:rows.value].copy()

    # -- per-link fresh deliveries (csrc/link.hip; helpers in links.py) ------
    def track_link_fresh(self, on=True):
        """gp_track_link_fresh: keep, per arc of the in-CSR, the first receipts
        it delivered from the next reset() on."""
        check(self._lib.gp_track_link_fresh(self._ctx, 1 if on else 0))

    def link_fresh(self):
        """u16 [nnz]: link_fresh[j] = the messages arc j of graph() (sender
        col[j], receiver the row of j) delivered since reset() to a receiver
        that did not hold them; its row sums are fresh_recv(), its sums by
        col are fresh_sent()."""
        return self._read(_lib.LINK_FRESH, np.empty(self.info()[1], dtype=np.uint16))

    def link_hist(self):
        """u64 [4097]: link_hist[c] = arcs with link_fresh() == c, computed on
        the device (links.hist is its numpy twin)."""
        buf = np.zeros(_lib.LINK_BINS, dtype=np.uint64)
        check(self._lib.gp_read_link_hist(self._ctx, _ptr(buf), buf.size))
        return buf

    # -- per-peer receipt delays (csrc/delay.hip; helpers in latency.py) -----
    def track_delay(self, on=True):
        """gp_track_delay: keep, per owned peer, the sum and the maximum of its
        receipt delays (receipt round - inject round) from the next reset() on."""
        check(self._lib.gp_track_delay(self._ctx, 1 if on else 0))

    def delay_sum(self):
        """u32 per owned vertex: the sum of v's receipt delays since reset(),
        over the seenpop()[v] messages it holds (latency.mean_delay divides)."""
        return self._read(_lib.DELAY_SUM, np.empty(self.nloc(), dtype=np.uint32))

    def delay_max(self):
        """u8 per owned vertex: v's largest receipt delay since reset() (0 for
        a peer that holds nothing, or only what was injected at it)."""
        return self._read(_lib.DELAY_MAX, np.empty(self.nloc(), dtype=np.uint8))

    def delay_bins(self):
        """u64 [32][5]: the record by degree bin, computed on the device
        (latency.bins is its numpy twin, latency.by_degree reads it): peers,
        peers reached, receipts, sum of delay_sum, max of delay_max."""
        buf = np.zeros((_lib.DELAY_BINS, _lib.DELAY_COLS), dtype=np.uint64)
        check(self._lib.gp_read_delay_bins(self._ctx, _ptr(buf), buf.shape[0]))
        return buf

    # -- per-peer delay distributions (csrc/delay_dist.hip; helpers in latency.py)
    def track_delay_dist(self, on=True):
        """gp_track_delay_dist: keep, per owned peer, its receipts per delay
        value (receipt round - inject round) from the next reset() on.
        Independent of track_delay()."""
        check(self._lib.gp_track_delay_dist(self._ctx, 1 if on else 0))

    def delay_dist(self):
        """u16 [owned vertices][16]: v's receipts since reset() with delay d in
        column d -- 0: injected at v, 1 .. 14 exact, 15: 15 rounds or later.
        Every row sums to seenpop()[v] (latency.dist_quantile reads it)."""
        return self._read(_lib.DELAY_DIST, np.empty((self.nloc(), _lib.DELAY_DIST_BINS), dtype=np.uint16))

    def delay_dist_bins(self):
        """u64 [32][16]: the rows summed by degree bin, computed on the device
        (latency.dist_bins is its numpy twin, latency.dist_by_degree reads it)."""
        buf = np.zeros((_lib.DELAY_BINS, _lib.DELAY_DIST_BINS), dtype=np.uint64)
        check(self._lib.gp_read_delay_dist_bins(self._ctx, _ptr(buf), buf.shape[0]))
        return buf

    # -- delivery multiplicity (csrc/mult.hip; helpers in fragility.py) -------
    def track_mult(self, on=True):
        """gp_track_mult: keep, from the next reset() on, how many in-neighbours
        delivered each first receipt -- the histogram of that number and the
        per-peer counts of receipts with a single deliverer."""
        check(self._lib.gp_track_mult(self._ctx, 1 if on else 0))

    def sole_sent(self):
        """u64 [n]: the first receipts, over all of u's out-arcs, for which u was
        the only deliverer since reset()."""
        return self._read(_lib.SOLE_SENT, np.empty(self.n, dtype=np.uint64))

    def sole_recv(self):
        """u32 [n]: v's first receipts since reset() that had one deliverer."""
        return self._read(_lib.SOLE_RECV, np.empty(self.n, dtype=np.uint32))

    def mult_hist(self):
        """u64 [17]: first receipts by deliverer count -- hist[c] for c = 1 .. 15,
        16 or more in hist[16], the injections at up origins in hist[0]
        (fragility.sole_share / at_least read it)."""
        buf = np.zeros(_lib.MULT_BINS, dtype=np.uint64)
        check(self._lib.gp_read_mult_hist(self._ctx, _ptr(buf), buf.size))
        return buf

    def sole_bins(self):
        """u64 [32][4]: the record by degree bin, computed on the device
        (fragility.bins is its numpy twin, fragility.by_degree reads it):
        peers, receipts, sum of sole_recv, sum of sole_sent."""
        buf = np.zeros((_lib.SOLE_BINS, _lib.SOLE_COLS), dtype=np.uint64)
        check(self._lib.gp_read_sole_bins(self._ctx, _ptr(buf), buf.shape[0]))
        return buf

    # -- watched peers (csrc/watch.hip; helpers in watch.py) -------------------
    def watch(self, verts, max_bytes=0):
        """gp_watch: keep, from the next reset() on, the arrival log of the
        peers `verts` (distinct vertex ids; an empty list turns the record off)
        -- one byte per (in-arc, message) and per (peer, message).  max_bytes
        bounds the two arrays (0: 1 GiB); a refused call leaves the previous
        list in force."""
        v = np.ascontiguousarray(verts, dtype=np.int32).reshape(-1)
        check(self._lib.gp_watch(self._ctx, int(v.size), _ptr(v) if v.size else None, int(max_bytes)))

    def watch_info(self):
        """(peers, arcs, bytes) of the list in force for the current run; 0s
        when none is."""
        k, a, b = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        check(self._lib.gp_watch_info(self._ctx, ctypes.byref(k), ctypes.byref(a), ctypes.byref(b)))
        return k.value, a.value, b.value

    def watch_ptr(self):
        """i64 [K + 1]: slot s's watched arcs are [ptr[s], ptr[s + 1]), the
        in-arcs of its peer in the in-CSR's order (watch.arcs is its numpy twin)."""
        return self._read(_lib.WATCH_PTR, np.empty(self.watch_info()[0] + 1, dtype=np.int64))

    def watch_first(self):
        """u8 [K][m]: the watched peers' first-receipt rows, 255 = never."""
        return self._read(_lib.WATCH_FIRST, np.empty((self.watch_info()[0], self.m), dtype=np.uint8))

    def watch_arrival(self):
        """u8 [A][m]: the receipt round of every message over every watched
        in-arc since reset(), 255 = never (watch.lines reads it)."""
        return self._read(_lib.WATCH_ARRIVAL, np.empty((self.watch_info()[1], self.m), dtype=np.uint8))

    def watch_peer(self, slot):
        """(first_row u8 [m], arrival u8 [deg][m]) of one slot, without reading
        the whole record."""
        ptr = self.watch_ptr()
        slot = int(slot)
        deg = int(ptr[slot + 1] - ptr[slot]) if 0 <= slot < ptr.size - 1 else 0
        first = np.empty(self.m, dtype=np.uint8)
        arr = np.empty((deg, self.m), dtype=np.uint8)
        check(self._lib.gp_read_watch_peer(self._ctx, slot, _ptr(first), _ptr(arr), arr.nbytes))
        return first, arr

    # -- lossy links (csrc/lossy.hip; helpers in loss.py) ----------------------
    def link_loss(self, p, seed=0):
        """gp_link_loss: from the next reset() on, every link drops the lines of
        a round with probability p, by a draw of the ordered pair of peers and
        the round (loss.arc_open is its numpy twin); link_loss(None) turns
        loss off.  A dropped line is lost for good.  reset() refuses loss
        together with a record that walks arcs (track_load, track_fresh,
        track_fresh_curve, track_link_fresh, track_mult, watch) or a vertex
        partition.  A p outside [0, 1] raises and leaves the request as it was."""
        if p is None:
            check(self._lib.gp_link_loss(self._ctx, 0, 0.0, 0))
        else:
            check(self._lib.gp_link_loss(self._ctx, 1, float(p), int(seed) & ((1 << 64) - 1)))

    def link_loss_info(self):
        """(on, p, seed) of the setting in force for the current run."""
        on, p, seed = ctypes.c_int32(), ctypes.c_double(), ctypes.c_uint64()
        check(self._lib.gp_link_loss_info(self._ctx, ctypes.byref(on), ctypes.byref(p), ctypes.byref(seed)))
        return bool(on.value), p.value, seed.value

    # -- delayed links (csrc/delayed.hip; helpers in lag.py) -------------------
    def link_delay(self, dmax, seed=0):
        """gp_link_delay: from the next reset() on, the link between peers u
        and v takes d(u, v) in [1, dmax] rounds, dmax <= 8, by a draw of the
        unordered pair (lag.arc_delay is its numpy twin); link_delay(None)
        turns delay off, link_delay(1) is the flood through the delayed
        kernels.  Rounds without a new bit occur while lines are in flight:
        run() stops by the delayed rule, a loop over round() reads
        link_delay_info()[3].  reset() refuses delay together with a record
        that walks arcs (track_load, track_fresh, track_fresh_curve,
        track_link_fresh, track_mult, watch), a vertex partition or a
        message-shard job; checkpoint() refuses with dmax > 1 in force.  A dmax
        outside [1, 8] raises and leaves the request as it was."""
        if dmax is None:
            check(self._lib.gp_link_delay(self._ctx, 0, 1, 0))
        else:
            check(self._lib.gp_link_delay(self._ctx, 1, int(dmax), int(seed) & ((1 << 64) - 1)))

    def link_delay_info(self):
        """(on, dmax, seed, in_flight) of the setting in force for the current
        run; in_flight counts the past rounds whose lines may still arrive (0:
        nothing is under way)."""
        on, dmax, seed, fl = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_int32()
        check(self._lib.gp_link_delay_info(self._ctx, ctypes.byref(on), ctypes.byref(dmax), ctypes.byref(seed),
                                           ctypes.byref(fl)))
        return bool(on.value), dmax.value, seed.value, fl.value

    def arc_delays(self):
        """u8 [nnz]: d(u, v) of arc j of graph() (sender col[j], receiver the
        row of j) while delay is in force (lag.arc_delays is its numpy twin)."""
        return self._read(_lib.ARC_DELAY, np.empty(self.info()[1], dtype=np.uint8))

    # -- anti-entropy repair (csrc/repair.hip; helpers in repair.py) -----------
    def repair(self, period, seed=0):
        """gp_repair: from the next reset() on, every round r with
        (r + 1) % period == 0 is a repair round, in which each up peer pulls
        the whole Message-List of one in-neighbour drawn from the peer and the
        round (repair.partners is its numpy twin) over that link, if the
        round's loss draw leaves it open; repair(None) turns it off.  What it
        brings is a first receipt like any other and is forwarded once.  run()
        stops after `period` silent rounds, a loop over round() reads
        repair_info()[3]; a silent period is the stopping rule, not
        convergence.  reset() refuses repair together with link_delay, a
        record that walks arcs (track_load, track_fresh, track_fresh_curve,
        track_link_fresh, track_mult, watch), a vertex partition or a
        message-shard job.  A period outside [1, 64] raises and leaves the
        request as it was."""
        if period is None:
            check(self._lib.gp_repair(self._ctx, 0, 1, 0))
        else:
            check(self._lib.gp_repair(self._ctx, 1, int(period), int(seed) & ((1 << 64) - 1)))

    def repair_info(self):
        """(on, period, seed, quiet) of the setting in force for the current
        run; quiet counts the most recent consecutive rounds at or after the
        last inject round without a new bit."""
        on, period, seed, quiet = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_int32()
        check(self._lib.gp_repair_info(self._ctx, ctypes.byref(on), ctypes.byref(period), ctypes.byref(seed),
                                       ctypes.byref(quiet)))
        return bool(on.value), period.value, seed.value, quiet.value

    def repair_record(self):
        """u64 [R][2]: per round run since reset(), the exchanges that happened
        and the Message-List entries they carried (both 0 outside the repair
        rounds)."""
        buf = np.zeros((254, 2), dtype=np.uint64)
        k = ctypes.c_int32()
        check(self._lib.gp_read_repair(self._ctx, _ptr(buf), 254, ctypes.byref(k)))
        return buf[:k.value].copy()

    def _nv(self):   # per-vertex reads: the owned slice of a partitioned context
        return self.nloc() if self.nranks > 1 else self.n

    def state(self):
        return self._read(_lib.STATE, np.empty(self._nv(), dtype=np.uint8))

    def miss(self):
        return self._read(_lib.MISS, np.empty(self._nv(), dtype=np.uint8))

    def deg_live(self):
        return self._read(_lib.DEG_LIVE, np.empty(self._nv(), dtype=np.int32))

    def frontier(self):
        return self._read(_lib.FRONTIER, np.empty((self._nv(), self.words), dtype=np.uint64))

    def reports(self, cap=1 << 20):
        """Reports of the last round as int32 [k, 3] (dead, reporter, round),
        unordered, plus the exact total (k < total if the buffer overflowed).
        gp_reports copies at most min(total, cap, report_capacity) rows: only
        those are returned."""
        buf = np.empty((cap, 3), dtype=np.int32)
        n = ctypes.c_int64()
        check(self._lib.gp_reports(self._ctx, ctypes.cast(buf.ctypes.data, ctypes.POINTER(_lib.Report)),
                                   int(cap), ctypes.byref(n)))
        k = min(n.value, cap, max(int(self.cfg.report_capacity), 1))
        return buf[:k].copy(), n.value
