"""Directed overlays large enough to reach the hub, liveness and late-round
paths, shared by test_oracle_directed.py (CPU) and test_gpu_directed.py.

Oriented Chung-Lu: the undirected Chung-Lu overlay of the oracle with one
rule for keeping an arc u -> v (CSR order: u = col[j], v = the row of j):
  coin   np.random.default_rng(seed).random(nnz) < p
  down   deg[u] > deg[v], ties by u < v   (hubs only send)
  up     the reverse of down               (hubs only receive)
Two-tier: undirected Chung-Lu overlays A and B side by side with one-way arcs
A -> B between their giant components only.  B's giant then receives every
message of A's giant and of its own and completes; A's giant holds its own
messages for ever and never completes, though both lie in one weak component.

Overlays and oracle runs are cached per process and handed out read-only.
"""
import numpy as np

_cache = {}


def _freeze(g):
    g.row_ptr.setflags(write=False)
    g.col.setflags(write=False)
    return g


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def oriented_chung_lu(pkg, oracle, n, dbar, gamma, seed, kind, p=0.6):
    def build():
        rp, col = oracle.chung_lu(n, dbar, gamma, seed)
        und = pkg.CSR(n, rp, col, False)
        u, v = und.arcs()
        deg = np.diff(rp)
        if kind == "coin":
            keep = np.random.default_rng(seed).random(u.size) < p
        else:
            keep = (deg[u] > deg[v]) | ((deg[u] == deg[v]) & (u < v))
            if kind == "up":
                keep = ~keep
            elif kind != "down":
                raise ValueError(kind)
        return _freeze(pkg.CSR.from_arcs(n, u[keep], v[keep], directed=True))
    return cached(("ocl", n, dbar, gamma, seed, kind, p), build)


def first3(pkg, n):
    return cached(("first3", n), lambda: _freeze(pkg.overlay.first3_overlay(n)))


def giant(oracle, g):
    """Vertices of the component of g's top hub (g undirected): the coverage
    of one oracle run with a single message there."""
    hub = int(np.argmax(np.diff(g.row_ptr)))
    ref = oracle.run(g, np.array([hub], np.int32), want_first=True)
    return np.nonzero(ref["first"][:, 0] != 255)[0]


def two_tier(pkg, oracle, na=12_000, nb=36_000, dbar=10, gamma=2.4, seed_a=21, seed_b=22, seed=23,
             cross=2000, hub_arcs=700, hubs=4):
    """(g, A_giant, B_giant), ids of B shifted by na."""
    def build():
        rpa, cola = oracle.chung_lu(na, dbar, gamma, seed_a)
        rpb, colb = oracle.chung_lu(nb, dbar, gamma, seed_b)
        a, b = pkg.CSR(na, rpa, cola, False), pkg.CSR(nb, rpb, colb, False)
        ga, gb = giant(oracle, a), giant(oracle, b)
        rng = np.random.default_rng(seed)
        top_a = ga[np.argsort(-np.diff(rpa)[ga], kind="stable")[:hubs]]
        top_b = gb[np.argsort(-np.diff(rpb)[gb], kind="stable")[:hubs]]
        src = [rng.choice(ga, cross)]
        dst = [rng.choice(gb, cross)]
        for h in top_a:
            src.append(np.full(hub_arcs, h))
            dst.append(rng.choice(gb, hub_arcs, replace=False))
        for h in top_b:
            src.append(rng.choice(ga, hub_arcs, replace=False))
            dst.append(np.full(hub_arcs, h))
        sa, da = a.arcs()
        sb, db = b.arcs()
        s = np.concatenate([sa, sb + na] + src)
        d = np.concatenate([da, db + na] + [x + na for x in dst])
        g = _freeze(pkg.CSR.from_arcs(na + nb, s, d, directed=True))
        ga, gb = ga.astype(np.int64), gb.astype(np.int64) + na
        ga.setflags(write=False)
        gb.setflags(write=False)
        return g, ga, gb
    return cached(("two_tier", na, nb, dbar, gamma, seed_a, seed_b, seed, cross, hub_arcs, hubs), build)


def two_tier_origins(g, A, B, m, seed):
    """A third of the origins in A's giant, m/64 in the small components, the
    rest in B's giant, in shuffled order."""
    rng = np.random.default_rng(seed)
    small = np.setdiff1d(np.arange(g.n), np.concatenate([A, B]))
    k_a, k_s = m // 3, m // 64
    o = np.concatenate([rng.choice(A, k_a), rng.choice(small, k_s), rng.choice(B, m - k_a - k_s)])
    return rng.permutation(o).astype(np.int32)


def two_tier_counts(origin, A, B):
    """(mA, mB): messages born in A's giant, in B's giant."""
    return int(np.isin(origin, A).sum()), int(np.isin(origin, B).sum())


def two_tier_masks(origin, A, B, words):
    """Message-List rows of a complete A-giant / B-giant vertex."""
    in_a, in_b = np.isin(origin, A), np.isin(origin, B)
    rows = []
    for sel in (in_a, in_a | in_b):
        row = np.zeros(words, np.uint64)
        for k in np.nonzero(sel)[0]:
            row[k >> 6] |= np.uint64(1) << np.uint64(k & 63)
        rows.append(row)
    return rows


class CachedOracle:
    """The oracle module with run() memoised on its arguments (the overlay by
    identity: overlays come from this module's cache and live as long as the
    process).  Results are read-only."""

    def __init__(self, oracle):
        self._oracle = oracle

    def __getattr__(self, name):
        return getattr(self._oracle, name)

    def run(self, g, origin, inject_round=None, **kw):
        origin = np.ascontiguousarray(origin, np.int32)
        inj = None if inject_round is None else np.ascontiguousarray(inject_round, np.int32).tobytes()
        kk = dict(kw)
        kk["crashes"] = tuple((int(v), int(r)) for v, r in kk.get("crashes", ()))
        kk.pop("nthreads", None)
        key = ("run", id(g), origin.tobytes(), inj, tuple(sorted(kk.items())))
        if key not in _cache:
            ref = self._oracle.run(g, origin, inject_round, **kw)
            for a in ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            _cache[key] = (g, ref)   # (holds g: its id stays taken)
        return _cache[key][1]


def held_before_round(ref):
    """Bits held at the start of each round of an oracle run."""
    got = np.array([s["new_bits"] + s["injected"] for s in ref["stats"]], np.int64)
    return np.concatenate([[0], np.cumsum(got)[:-1]])
