"""Launch order of k_expand's 64-vertex blocks (csrc/block_order.h), on the CPU.

build_hubs (csrc/setup.hip) orders the blocks of a context's owned vertices so
that the blocks with a long non-hub in-list are launched first; this test
drives the builder, compiled with g++ through a test-only shim
(tests/native/block_order_shim.cpp), on synthetic row_ptr arrays against an
independent restatement: a permutation of the blocks, blocks over the cut
first (longest first, ties by id), the rest in natural order, hubs not
counted, partial last blocks.  The order only schedules the pull, whose result
is the reference's send loop over every link (Peer.py:402-404) whatever the
order.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "block_order_shim.cpp")

LL = ctypes.c_longlong
P_LL = ctypes.POINTER(LL)
P_I = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def bo(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("block_order") / "libblock_order_shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", CSRC, SHIM, "-o", so])
    lib = ctypes.CDLL(so)
    lib.bo_order.argtypes = [P_LL, LL, LL, LL, P_I]
    lib.bo_order.restype = LL
    return lib


def order(bo, deg, hub_thr, cut):
    deg = np.asarray(deg, np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nloc = len(deg)
    nb = (nloc + 63) // 64
    out = np.full(nb + 1, -7, np.int32)   # one guard entry behind the order
    got = bo.bo_order(rp.ctypes.data_as(P_LL), nloc, hub_thr, cut, out.ctypes.data_as(P_I))
    assert got == nb and out[nb] == -7
    return out[:nb]


def block_len(deg, hub_thr):
    """longest non-hub in-list of every block"""
    deg = np.asarray(deg, np.int64)
    nb = (len(deg) + 63) // 64
    d = np.where(deg <= hub_thr, deg, 0)
    d = np.concatenate([d, np.zeros(nb * 64 - len(d), np.int64)])
    return d.reshape(nb, 64).max(axis=1)


def check(o, deg, hub_thr, cut):
    ln = block_len(deg, hub_thr)
    nb = len(ln)
    assert sorted(o.tolist()) == list(range(nb))                      # a permutation of the blocks
    heavy = [b for b in range(nb) if ln[b] > cut]
    want = sorted(heavy, key=lambda b: (-ln[b], b)) + [b for b in range(nb) if ln[b] <= cut]
    assert o.tolist() == want
    return len(heavy)


@pytest.mark.parametrize("nloc", [1, 40, 63, 64, 65, 64 * 50, 64 * 50 + 37])
@pytest.mark.parametrize("cut", [0, 100, 1024])
def test_order_on_power_law_degrees(bo, nloc, cut):
    rng = np.random.default_rng(nloc * 7 + cut)
    deg = np.minimum((rng.pareto(1.2, nloc) * 8).astype(np.int64) + 1, 20_000)
    hub_thr = 4096
    nh = check(order(bo, deg, hub_thr, cut), deg, hub_thr, cut)
    if cut == 0:
        assert nh == (nloc + 63) // 64   # a whole sort: every block has an in-list


def test_heavy_first_longest_first_ties_by_id(bo):
    deg = np.full(64 * 10, 3, np.int64)
    deg[64 * 7 + 5] = 2000
    deg[64 * 2 + 63] = 3000
    deg[64 * 9] = 2000
    deg[64 * 4 + 1] = 1024   # at the cut: not over it
    o = order(bo, deg, 4096, 1024)
    assert o.tolist() == [2, 7, 9, 0, 1, 3, 4, 5, 6, 8]


def test_hubs_do_not_count(bo):
    deg = np.full(64 * 6, 10, np.int64)
    deg[64 * 1 + 3] = 5000    # a hub: the hub kernels scan it
    deg[64 * 3 + 3] = 4096    # the longest in-list that is not a hub
    deg[64 * 5 + 9] = 100_000
    deg[64 * 5 + 10] = 1500
    o = order(bo, deg, 4096, 1024)
    assert o.tolist() == [3, 5, 0, 1, 2, 4]
    # with the threshold out of reach they count like any other vertex
    o = order(bo, deg, 1 << 30, 1024)
    assert o.tolist() == [5, 1, 3, 0, 2, 4]


def test_equal_degrees_keep_the_identity(bo):
    for nloc in (40, 64 * 9, 64 * 9 + 1):
        for d in (2, 2000):
            o = order(bo, np.full(nloc, d, np.int64), 4096, 1024)
            nb = (nloc + 63) // 64
            assert o.tolist() == list(range(nb))   # (all over the cut: equal lengths, ties by id)


def test_partial_last_block_and_single_block(bo):
    nloc = 64 * 1000 + 37
    deg = np.full(nloc, 4, np.int64)
    deg[nloc - 1] = 3000            # in the last, partial block
    o = order(bo, deg, 1 << 30, 1024)
    assert o[0] == 1000 and o[1:].tolist() == list(range(1000))
    deg = np.full(40, 4, np.int64)
    deg[39] = 3000
    assert order(bo, deg, 1 << 30, 1024).tolist() == [0]
    assert order(bo, np.zeros(5, np.int64), 64, 0).tolist() == [0]   # no arcs at all
