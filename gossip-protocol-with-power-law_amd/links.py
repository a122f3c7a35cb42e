"""Reading the per-link fresh deliveries (GossipEngine.link_fresh() /
link_hist(), csrc/link.hip).

link_fresh[j] is the first receipts arc j of the in-CSR delivered: sender
col[j], receiver the row of j -- the arrival lines of the reference's logs that
were news (Peer.py:206, Peer.py:286), grouped by the connection they came
over.  fresh_sent() and fresh_recv() (redundancy.py) are its sums by sender and
by receiver.  These helpers answer what a designer of the overlay asks: which
links never deliver anything first, how few carry a given share of the news,
and whether a link works in both directions.  Pure numpy; every function
validates its shapes and raises ValueError on arrays that cannot belong to one
run.
"""
import numpy as np

BINS = 4097   # counts 0 .. 4096: a link delivers each of at most 4096 messages once


def _counts(link_fresh, nnz=None):
    lf = np.asarray(link_fresh)
    if lf.ndim != 1 or lf.dtype.kind not in "ui":
        raise ValueError("link_fresh must be an integer array [nnz]")
    lf = lf.astype(np.int64)
    if nnz is not None and lf.size != int(nnz):
        raise ValueError(f"link_fresh has {lf.size} entries, the overlay {int(nnz)} arcs: arrays of different runs")
    if lf.size and (lf.min() < 0 or lf.max() >= BINS):
        raise ValueError("a link delivers at most 4096 messages: not a link_fresh array")
    return lf


def _share(share):
    share = float(share)
    if not 0.0 <= share <= 1.0:
        raise ValueError("share must lie in [0, 1]")
    return share


def ends(csr):
    """(src, dst) int64 [nnz]: arc j goes from src[j] = col[j] to dst[j], the
    row of j."""
    rp = np.asarray(csr.row_ptr, np.int64)
    col = np.asarray(csr.col, np.int64)
    n = int(csr.n)
    if rp.shape != (n + 1,) or rp[0] != 0 or (np.diff(rp) < 0).any() or rp[-1] != col.size:
        raise ValueError("row_ptr is not the row pointer of col")
    if col.size and (col.min() < 0 or col.max() >= n):
        raise ValueError("col names a vertex out of range")
    return col, np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))


def fold_peers(csr, link_fresh):
    """(fresh_sent, fresh_recv) int64 [n]: the record summed by sender and by
    receiver -- exactly GossipEngine.fresh_sent() / fresh_recv() of the run."""
    src, dst = ends(csr)
    lf = _counts(link_fresh, src.size)
    n = int(csr.n)
    sent = np.bincount(src, weights=lf, minlength=n).astype(np.int64)
    recv = np.bincount(dst, weights=lf, minlength=n).astype(np.int64)
    return sent, recv


def undirected(csr, link_fresh):
    """(u, v, uv, vu): every link {u, v} of an undirected overlay once, u < v,
    in (u, v) order, with the news it carried u -> v and v -> u (int64).  Raises
    on a directed overlay and on an arc without its reverse."""
    if getattr(csr, "directed", False):
        raise ValueError("a directed overlay has arcs, not links")
    src, dst = ends(csr)
    lf = _counts(link_fresh, src.size)
    n = int(csr.n)
    if (src == dst).any():
        raise ValueError("a self-loop is no link")
    fwd = np.nonzero(src < dst)[0]
    bwd = np.nonzero(src > dst)[0]
    fwd = fwd[np.argsort(src[fwd] * n + dst[fwd], kind="stable")]
    bwd = bwd[np.argsort(dst[bwd] * n + src[bwd], kind="stable")]
    ku, kv = src[fwd] * n + dst[fwd], dst[bwd] * n + src[bwd]
    if ku.size != kv.size or not np.array_equal(ku, kv) or (np.diff(ku) == 0).any():
        raise ValueError("an arc without its reverse (or a repeated arc): not an undirected overlay")
    return src[fwd], dst[fwd], lf[fwd], lf[bwd]


def idle_share(link_fresh):
    """The share of the arcs that never delivered a first receipt (0.0 for an
    overlay without arcs)."""
    lf = _counts(link_fresh)
    return float((lf == 0).sum()) / lf.size if lf.size else 0.0


def backbone(link_fresh, share=0.5):
    """Indices (int64) of the fewest arcs whose counts reach `share` of the
    total, by count descending, then by arc index -- so the answer is unique.
    Empty when nothing was delivered or share is 0."""
    lf = _counts(link_fresh)
    share = _share(share)
    total = int(lf.sum())
    if total == 0 or share == 0.0:
        return np.zeros(0, np.int64)
    order = np.argsort(-lf, kind="stable")   # (stable: ties stay in arc order)
    run = np.cumsum(lf[order])
    k = int(np.searchsorted(run, share * total, side="left")) + 1
    return order[:min(k, lf.size)].astype(np.int64)


def hist(link_fresh):
    """uint64 [4097]: hist[c] = arcs with link_fresh == c, the numpy twin of
    GossipEngine.link_hist()."""
    return np.bincount(_counts(link_fresh), minlength=BINS).astype(np.uint64)


def hist_backbone(hist, share=0.5):
    """(arcs, least): how many arcs backbone() would return and the smallest
    count among them, from the histogram alone.  (0, 0) when nothing was
    delivered or share is 0."""
    h = np.asarray(hist)
    if h.shape != (BINS,) or h.dtype.kind not in "ui" or (h.dtype.kind == "i" and (h < 0).any()):
        raise ValueError(f"hist must be [{BINS}] counts")
    share = _share(share)
    h = [int(x) for x in h]
    total = sum(c * k for c, k in enumerate(h))
    if total == 0 or share == 0.0:
        return 0, 0
    need = share * total
    arcs = carried = 0
    for c in range(BINS - 1, 0, -1):
        if not h[c]:
            continue
        if carried + c * h[c] >= need:
            # the fewest arcs of this bin that reach `need` (backbone's comparison, run >= share * total)
            take = max(1, int((need - carried) // c))
            while carried + c * take < need:
                take += 1
            while take > 1 and carried + c * (take - 1) >= need:
                take -= 1
            return arcs + take, c
        arcs += h[c]
        carried += c * h[c]
    return arcs, 1   # (unreachable: the total is reached at the last non-empty bin)
