"""Bit-sliced row counting of the spread curve (csrc/curve_planes.h), on the CPU.

k_curve (csrc/curve.hip) counts the frontier rows of a round's receivers per
message: each lane adds its word of up to eight rows through a carry-save tree
into ones / twos / fours / eights planes and expands them to per-bit counts
only when they are full (2047 rows) or its range ends.  This test compiles the
same header with g++ through tests/native/curve_planes_shim.cpp and compares
it with per-bit counting: random rows at exactly the capacity and one row
either side of it, all-ones rows, empty rows, both entry paths.  What is
counted is the aggregate of each reference peer's arrival log
(Peer.py:175-216).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "curve_planes_shim.cpp")

P_U64 = ctypes.POINTER(ctypes.c_ulonglong)
P_U32 = ctypes.POINTER(ctypes.c_uint)


@pytest.fixture(scope="module")
def cp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("curve_planes") / "libcurve_planes_shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", CSRC, SHIM, "-o", so])
    lib = ctypes.CDLL(so)
    lib.cp_count.argtypes = [P_U64, ctypes.c_longlong, ctypes.c_int, P_U32]
    lib.cp_count.restype = ctypes.c_int
    lib.cp_raw.argtypes = [P_U64, ctypes.c_longlong, P_U32]
    lib.cp_raw.restype = None
    return lib


def per_bit(rows):
    rows = np.asarray(rows, np.uint64)
    return np.array([int(((rows >> np.uint64(b)) & np.uint64(1)).sum()) for b in range(64)], np.int64)


def count(cp, rows, group):
    rows = np.ascontiguousarray(rows, np.uint64)
    out = np.zeros(65, np.uint32)
    out[64] = 0xDEAD   # one guard entry behind the counts
    flushes = cp.cp_count(rows.ctypes.data_as(P_U64), len(rows), group, out.ctypes.data_as(P_U32))
    assert out[64] == 0xDEAD
    return out[:64].astype(np.int64), flushes


def test_capacity_is_what_eleven_planes_hold(cp):
    assert cp.cp_capacity() == 2047 == 2 ** (3 + 8) - 1
    assert cp.cp_group() == 8


@pytest.mark.parametrize("group", [1, 8])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_random_rows_around_the_capacity(cp, group, delta):
    cap = cp.cp_capacity()
    n = cap + delta
    rng = np.random.Generator(np.random.PCG64(100 + delta))
    rows = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    got, flushes = count(cp, rows, group)
    assert np.array_equal(got, per_bit(rows))
    # single rows fill the planes exactly; groups of eight book eight rows a step
    if group == 1:
        assert flushes == (1 if n <= cap else 2)
    else:
        steps = -(-n // 8)
        assert flushes == -(-steps // (cap // 8))


@pytest.mark.parametrize("group", [1, 8])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_all_ones_rows(cp, group, delta):
    n = cp.cp_capacity() + delta
    rows = np.full(n, np.uint64(0xFFFFFFFFFFFFFFFF))
    got, _ = count(cp, rows, group)
    assert (got == n).all()


@pytest.mark.parametrize("group", [1, 8])
def test_empty_rows_and_no_rows(cp, group):
    got, flushes = count(cp, np.zeros(5000, np.uint64), group)
    assert (got == 0).all()
    got, flushes = count(cp, np.zeros(0, np.uint64), group)
    assert (got == 0).all() and flushes == 0


@pytest.mark.parametrize("group", [1, 8])
def test_sparse_and_single_column_rows(cp, group):
    rng = np.random.Generator(np.random.PCG64(7))
    n = 3 * cp.cp_capacity() + 5
    rows = (np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64)) * (rng.random(n) < 0.3).astype(np.uint64)
    got, _ = count(cp, rows, group)
    assert np.array_equal(got, per_bit(rows))
    col = np.full(n, np.uint64(1) << np.uint64(63))
    got, _ = count(cp, col, group)
    assert got[63] == n and got[:63].sum() == 0


def test_planes_hold_exactly_the_capacity(cp):
    """Without an expansion in between the planes are exact up to the capacity
    and wrap one row later: the capacity constant is the true bound."""
    cap = cp.cp_capacity()
    out = np.zeros(64, np.uint32)
    ones = np.full(cap + 1, np.uint64(0xFFFFFFFFFFFFFFFF))
    cp.cp_raw(ones.ctypes.data_as(P_U64), cap, out.ctypes.data_as(P_U32))
    assert (out == cap).all()
    cp.cp_raw(ones.ctypes.data_as(P_U64), cap + 1, out.ctypes.data_as(P_U32))
    assert (out == 0).all()
