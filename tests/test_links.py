"""links.py's helpers on hand-made arrays (CPU)."""
import numpy as np
import pytest

import _gossip_pkg

links = _gossip_pkg.load().links   # (the module under test: its absence fails the file)


def triangle(pkg):
    """0 - 1, 0 - 2, 1 - 2, undirected.  Arcs in CSR order: 1>0 2>0 | 0>1 2>1 | 0>2 1>2"""
    return pkg.CSR(3, np.array([0, 2, 4, 6], np.int64), np.array([1, 2, 0, 2, 0, 1], np.int32), False)


LF = np.array([5, 0, 7, 0, 2, 2], np.uint16)


def test_ends_and_fold_peers(pkg):
    g = triangle(pkg)
    src, dst = links.ends(g)
    assert src.dtype == dst.dtype == np.int64
    assert src.tolist() == [1, 2, 0, 2, 0, 1] and dst.tolist() == [0, 0, 1, 1, 2, 2]
    sent, recv = links.fold_peers(g, LF)
    assert sent.dtype == recv.dtype == np.int64
    assert sent.tolist() == [9, 7, 0] and recv.tolist() == [5, 7, 4]
    assert sent.sum() == recv.sum() == int(LF.sum())
    empty = pkg.CSR(2, np.zeros(3, np.int64), np.zeros(0, np.int32), False)
    s, r = links.fold_peers(empty, np.zeros(0, np.uint16))
    assert s.tolist() == r.tolist() == [0, 0]
    with pytest.raises(ValueError):
        links.fold_peers(g, LF[:5])                                 # the array of another overlay
    with pytest.raises(ValueError):
        links.fold_peers(g, LF.astype(np.float64))
    with pytest.raises(ValueError):
        links.fold_peers(g, LF.reshape(2, 3))
    with pytest.raises(ValueError):
        links.fold_peers(g, np.array([5, 0, 7, 0, 2, 4097]))        # more than a link can deliver
    with pytest.raises(ValueError):
        links.fold_peers(g, np.array([5, 0, 7, 0, 2, -1]))
    with pytest.raises(ValueError):
        links.ends(pkg.CSR(3, np.array([0, 2, 4, 5], np.int64), g.col, False))   # row_ptr of another col
    with pytest.raises(ValueError):
        links.ends(pkg.CSR(3, g.row_ptr, np.array([1, 2, 0, 2, 0, 3], np.int32), False))


def test_undirected(pkg):
    g = triangle(pkg)
    u, v, uv, vu = links.undirected(g, LF)
    assert u.tolist() == [0, 0, 1] and v.tolist() == [1, 2, 2]
    assert uv.tolist() == [7, 2, 2] and vu.tolist() == [5, 0, 0]
    assert uv.dtype == vu.dtype == np.int64
    assert int(uv.sum() + vu.sum()) == int(LF.sum())
    # rows in any column order fold the same way
    g2 = pkg.CSR(3, g.row_ptr, np.array([2, 1, 2, 0, 1, 0], np.int32), False)
    u2, v2, uv2, vu2 = links.undirected(g2, np.array([0, 5, 0, 7, 2, 2], np.uint16))
    assert (u2.tolist(), v2.tolist(), uv2.tolist(), vu2.tolist()) == (u.tolist(), v.tolist(), uv.tolist(), vu.tolist())
    with pytest.raises(ValueError):
        links.undirected(pkg.CSR(3, g.row_ptr, g.col, True), LF)    # directed
    one_way = pkg.CSR(3, np.array([0, 1, 2, 2], np.int64), np.array([1, 2], np.int32), False)
    with pytest.raises(ValueError):
        links.undirected(one_way, np.zeros(2, np.uint16))           # 1>0 without 0>1
    lopsided = pkg.CSR(3, np.array([0, 1, 2, 2], np.int64), np.array([1, 0], np.int32), False)
    assert [x.tolist() for x in links.undirected(lopsided, np.array([3, 4], np.uint16))] == [[0], [1], [4], [3]]
    doubled = pkg.CSR(2, np.array([0, 2, 4], np.int64), np.array([1, 1, 0, 0], np.int32), False)
    with pytest.raises(ValueError):
        links.undirected(doubled, np.zeros(4, np.uint16))
    with pytest.raises(ValueError):
        links.undirected(g, LF[:4])


def test_idle_share_and_hist(pkg):
    assert links.idle_share(LF) == pytest.approx(2 / 6)
    assert links.idle_share(np.zeros(0, np.uint16)) == 0.0
    assert links.idle_share(np.zeros(4, np.uint16)) == 1.0
    h = links.hist(LF)
    assert h.dtype == np.uint64 and h.shape == (4097,)
    assert h[0] == 2 and h[2] == 2 and h[5] == 1 and h[7] == 1 and int(h.sum()) == 6
    top = links.hist(np.array([4096, 0], np.uint16))
    assert top[4096] == 1 and top[0] == 1
    assert not links.hist(np.zeros(0, np.uint16)).any()
    with pytest.raises(ValueError):
        links.hist(np.array([4097]))
    with pytest.raises(ValueError):
        links.idle_share(np.zeros((2, 2), np.uint16))


def test_backbone_and_its_tie_order(pkg):
    # total 16, half = 8: 7 alone is short, 7 + 5 reaches it
    assert links.backbone(LF).tolist() == [2, 0]
    assert links.backbone(LF, 7 / 16).tolist() == [2]                # reached exactly: no arc more
    assert links.backbone(LF, 1.0).tolist() == [2, 0, 4, 5]          # the idle arcs are never needed
    assert links.backbone(LF, 13 / 16).tolist() == [2, 0, 4]         # equal counts: the lower arc index first
    assert links.backbone(LF, 0.0).size == 0
    assert links.backbone(np.zeros(5, np.uint16)).size == 0
    ties = np.array([3, 3, 3, 3], np.uint16)
    assert links.backbone(ties, 0.5).tolist() == [0, 1]
    assert links.backbone(ties[::-1].copy(), 0.75).tolist() == [0, 1, 2]
    assert links.backbone(LF).dtype == np.int64
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            links.backbone(LF, bad)


def test_hist_backbone_agrees_with_backbone(pkg):
    rng = np.random.default_rng(5)
    arrays = [LF, np.array([3, 3, 3, 3], np.uint16), np.array([4096, 4096, 0, 1], np.uint16),
              rng.integers(0, 60, 500).astype(np.uint16), (rng.random(300) < 0.1).astype(np.uint16),
              rng.integers(0, 4097, 200).astype(np.uint16)]
    for lf in arrays:
        for share in (0.01, 0.25, 0.5, 0.75, 0.9, 1.0):
            idx = links.backbone(lf, share)
            arcs, least = links.hist_backbone(links.hist(lf), share)
            assert arcs == idx.size, (share, arcs, idx.size)
            assert least == int(lf[idx].min()), share
    assert links.hist_backbone(links.hist(LF)) == (2, 5)
    assert links.hist_backbone(links.hist(LF), 0.0) == (0, 0)
    assert links.hist_backbone(np.zeros(4097, np.uint64)) == (0, 0)
    with pytest.raises(ValueError):
        links.hist_backbone(np.zeros(4096, np.uint64))
    with pytest.raises(ValueError):
        links.hist_backbone(np.zeros(4097))
    with pytest.raises(ValueError):
        links.hist_backbone(links.hist(LF), 2.0)
