"""Bit-sliced inject-round arithmetic of the receipt delays
(csrc/delay_planes.h), on the CPU.

k_delay (csrc/delay.hip) turns a receiver's new row into its share of
delay_sum and delay_max without a per-bit loop: plane b of a word is the mask
of its messages whose inject round has bit b set, the sum of the inject rounds
of a word's bits is sum_b popc(x & P_b) << b, and their minimum comes from an
8-step descent from bit 7.  This test compiles the same header with g++ through
tests/native/delay_planes_shim.cpp and compares each step with per-bit
arithmetic: random and single-bit words, tables whose inject rounds are all
equal, rounds 0 and 253 in one word, every plane exercised.  What is computed
is the time column of each reference peer's arrival log (Peer.py:206,
Peer.py:286), relative to the message's own start.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "delay_planes_shim.cpp")

P_U8 = ctypes.POINTER(ctypes.c_ubyte)
P_U64 = ctypes.POINTER(ctypes.c_ulonglong)
P_U32 = ctypes.POINTER(ctypes.c_uint)


@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("delay_planes") / "libdelay_planes_shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", CSRC, SHIM, "-o", so])
    lib = ctypes.CDLL(so)
    lib.dp_no_min.restype = ctypes.c_uint
    lib.dp_build.argtypes = [P_U8, ctypes.c_int, ctypes.c_int, P_U64]
    lib.dp_build.restype = None
    lib.dp_uniform.argtypes = [P_U8, ctypes.c_int]
    lib.dp_uniform.restype = ctypes.c_int
    lib.dp_word.argtypes = [ctypes.c_ulonglong, P_U64, ctypes.c_int, ctypes.c_int, P_U32, P_U32]
    lib.dp_word.restype = None
    lib.dp_row.argtypes = [P_U64, P_U64, ctypes.c_int, ctypes.c_uint, P_U32]
    lib.dp_row.restype = None
    lib.dp_bin.argtypes = [ctypes.c_longlong]
    lib.dp_bin.restype = ctypes.c_int
    return lib


def words_of(m):
    w = 1
    while w * 64 < m:
        w <<= 1
    return w


def build(dp, inject):
    inject = np.ascontiguousarray(inject, np.uint8)
    W = words_of(inject.size)
    planes = np.full(8 * W + 1, 0xDEAD, np.uint64)   # one guard word behind the planes
    dp.dp_build(inject.ctypes.data_as(P_U8), inject.size, W, planes.ctypes.data_as(P_U64))
    assert planes[-1] == 0xDEAD
    return planes[:-1].copy(), W


def bits_of(x):
    return [b for b in range(64) if (int(x) >> b) & 1]


def word(dp, x, planes, W, w):
    s, mn = ctypes.c_uint(), ctypes.c_uint()
    dp.dp_word(int(x), planes.ctypes.data_as(P_U64), W, w, ctypes.byref(s), ctypes.byref(mn))
    return s.value, mn.value


def check_words(dp, inject, xs_by_word):
    """every (w, x) against the inject rounds of x's bits, one by one"""
    planes, W = build(dp, inject)
    m = len(inject)
    for w, x in xs_by_word:
        ks = [w * 64 + b for b in bits_of(x)]
        assert all(k < m for k in ks)
        s, mn = word(dp, x, planes, W, w)
        assert s == sum(int(inject[k]) for k in ks), (w, hex(int(x)))
        assert mn == (min(int(inject[k]) for k in ks) if ks else dp.dp_no_min()), (w, hex(int(x)))


def test_constants(dp):
    assert dp.dp_planes_per_word() == 8        # inject rounds are <= 253 (gp_set_messages)
    assert dp.dp_no_min() > 254                # above every receipt round: a min-reduction ignores empty words


@pytest.mark.parametrize("m", [1, 64, 100, 512, 1000, 2048, 4096])
def test_plane_construction(dp, m):
    rng = np.random.Generator(np.random.PCG64(m))
    inject = rng.integers(0, 254, m).astype(np.uint8)
    planes, W = build(dp, inject)
    assert W == words_of(m)
    for b in range(8):
        for w in range(W):
            exp = 0
            for k in range(w * 64, min(m, w * 64 + 64)):
                if (int(inject[k]) >> b) & 1:
                    exp |= 1 << (k - w * 64)
            assert int(planes[b * W + w]) == exp, (b, w)   # (bits past m stay clear)


@pytest.mark.parametrize("m", [64, 100, 1000, 4096])
def test_random_words(dp, m):
    rng = np.random.Generator(np.random.PCG64(10 + m))
    inject = rng.integers(0, 254, m).astype(np.uint8)
    W = words_of(m)
    cases = []
    for w in range(W):
        valid = max(0, min(64, m - w * 64))
        mask = (1 << valid) - 1
        for dens in (0.5, 0.05):
            x = 0
            for b in np.nonzero(rng.random(64) < dens)[0]:
                x |= 1 << int(b)
            cases.append((w, x & mask))
        cases.append((w, mask))       # every valid message of the word
        cases.append((w, 0))          # an empty word
    check_words(dp, inject, cases)


def test_single_bit_words(dp):
    m = 200
    inject = ((np.arange(m) * 37) % 254).astype(np.uint8)
    check_words(dp, inject, [(k >> 6, 1 << (k & 63)) for k in range(m)])


@pytest.mark.parametrize("j", [0, 2, 128, 253])
def test_all_equal_inject_rounds(dp, j):
    m = 130
    inject = np.full(m, j, np.uint8)
    assert dp.dp_uniform(inject.ctypes.data_as(P_U8), m) == j
    planes, W = build(dp, inject)
    rng = np.random.Generator(np.random.PCG64(j))
    for w in range(3):
        valid = min(64, m - w * 64)
        x = int(rng.integers(1, 1 << 62)) & ((1 << valid) - 1) or 1
        s, mn = word(dp, x, planes, W, w)
        assert s == j * bin(x).count("1") and mn == j
    moved = inject.copy()
    moved[77] = j ^ 1
    assert dp.dp_uniform(moved.ctypes.data_as(P_U8), m) == -1
    assert dp.dp_uniform(inject.ctypes.data_as(P_U8), 1) == j


def test_rounds_0_and_253_in_one_word(dp):
    inject = np.full(64, 253, np.uint8)
    inject[17] = 0
    both = (1 << 17) | (1 << 40)
    check_words(dp, inject, [(0, both), (0, 1 << 40), (0, 1 << 17), (0, (1 << 64) - 1)])
    planes, W = build(dp, inject)
    assert word(dp, both, planes, W, 0) == (253, 0)
    assert word(dp, (1 << 64) - 1, planes, W, 0) == (63 * 253, 0)


def test_every_plane_decides_the_minimum(dp):
    """two messages whose inject rounds differ in bit b alone, for every b: the
    descent must take the one with the bit clear; and rounds 1 << b alone"""
    for b in range(8):
        lo = 0x55 & ~(1 << b) & 0xFF
        hi = lo | (1 << b)
        if hi > 253:
            lo, hi = 0, 1 << b
        inject = np.array([hi, lo, hi], np.uint8)
        planes, W = build(dp, inject)
        assert word(dp, 0b111, planes, W, 0) == (2 * hi + lo, lo), b
        assert word(dp, 0b101, planes, W, 0) == (2 * hi, hi), b
        single = np.array([1 << b], np.uint8)
        planes, W = build(dp, single)
        assert int(planes[b]) == 1 and sum(int(p) for p in planes) == 1
        assert word(dp, 1, planes, W, 0) == (1 << b, 1 << b)


@pytest.mark.parametrize("m", [100, 4096])
def test_rows(dp, m):
    """a whole new row of receipt round rr: its share of delay_sum and its
    largest delay, as the W lanes of a row and their reduction give them"""
    rng = np.random.Generator(np.random.PCG64(20 + m))
    W = words_of(m)
    inject = rng.integers(0, 40, m).astype(np.uint8)
    planes, _ = build(dp, inject)
    rr = 41
    for dens in (0.5, 0.01, 1.0):
        held = rng.random(m) < dens
        if not held.any():
            held[m // 2] = True
        row = np.zeros(W, np.uint64)
        for k in np.nonzero(held)[0]:
            row[k >> 6] |= np.uint64(1) << np.uint64(k & 63)
        out = np.zeros(2, np.uint32)
        dp.dp_row(row.ctypes.data_as(P_U64), planes.ctypes.data_as(P_U64), W, rr, out.ctypes.data_as(P_U32))
        d = rr - inject[held].astype(np.int64)
        assert out[0] == d.sum() and out[1] == d.max()


def test_degree_bins(dp):
    for deg, b in [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (7, 2), (8, 3), (913, 9), (1023, 9), (1024, 10),
                   (2 ** 31 - 1, 30)]:
        assert dp.dp_bin(deg) == b, deg
