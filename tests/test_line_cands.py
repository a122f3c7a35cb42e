"""Candidates of the per-line done-neighbour rule (csrc/line_cands.h), on the CPU.

build_hubs (csrc/setup.hip) lists the owned vertices of in-degree >= the
minimum degree; k_line_done notes their complete Message-List lines before an
early-exit pull.  This test drives the builder, compiled with g++ through a
test-only shim (tests/native/line_cands_shim.cpp), on synthetic row_ptr arrays:
the threshold edge, no candidates, all vertices, ascending order.  The list
only decides which row loads the pull may drop; the pull's result is the
reference's send loop over every link (Peer.py:402-404) whatever it holds.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "line_cands_shim.cpp")

LL = ctypes.c_longlong
P_LL = ctypes.POINTER(LL)
P_I = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def lc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("line_cands") / "libline_cands_shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", CSRC, SHIM, "-o", so])
    lib = ctypes.CDLL(so)
    lib.lc_cands.argtypes = [P_LL, LL, LL, P_I, LL]
    lib.lc_cands.restype = LL
    lib.lc_default_min_deg.restype = ctypes.c_int
    return lib


def cands(lc, deg, min_deg):
    deg = np.asarray(deg, np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    out = np.full(len(deg) + 1, -7, np.int32)   # one guard entry behind the list
    k = lc.lc_cands(rp.ctypes.data_as(P_LL), len(deg), min_deg, out.ctypes.data_as(P_I), len(deg))
    assert 0 <= k <= len(deg) and out[len(deg)] == -7
    assert (out[k:len(deg)] == -7).all()
    return out[:k].tolist()


def test_threshold_edge(lc):
    deg = [0, 15, 16, 17, 16, 3, 1000, 15]
    assert cands(lc, deg, 16) == [2, 3, 4, 6]
    assert cands(lc, deg, 17) == [3, 6]
    assert cands(lc, deg, 1000) == [6]


def test_no_candidates(lc):
    assert cands(lc, [0, 1, 2, 3], 4) == []
    assert cands(lc, [], 1) == []
    assert cands(lc, [0, 0, 0], 1) == []


def test_all_vertices(lc):
    deg = [1, 5, 2, 9, 1]
    assert cands(lc, deg, 1) == [0, 1, 2, 3, 4]
    # a minimum below 1 counts as 1: vertices without in-arcs stay out
    assert cands(lc, [0, 2, 0, 1], 0) == [1, 3]
    assert cands(lc, [0, 2, 0, 1], -5) == [1, 3]


def test_random_against_numpy(lc):
    rng = np.random.Generator(np.random.PCG64(3))
    deg = rng.zipf(2.0, 5000).clip(0, 10_000)
    for t in (1, 2, 16, 64, 256, 20_000):
        assert cands(lc, deg, t) == np.nonzero(deg >= t)[0].tolist()


def test_default_is_a_documented_threshold(lc):
    assert lc.lc_default_min_deg() in (64, 256, 1024)   # the three the ledger's estimate prices
