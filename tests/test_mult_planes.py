"""Saturating bit-sliced deliverer counter of the delivery multiplicity record
(csrc/mult_planes.h), on the CPU.

k_mult (csrc/mult.hip) counts, for the 64 messages of a word at once, how many
in-neighbours delivered each first receipt: four count planes and a sticky
"16 or more" plane, an add per gathered row, a bit-sliced merge of the row
slots' counters, and the masks of the positions whose count is exactly c.  This
test compiles the same header with g++ through
tests/native/mult_planes_shim.cpp and compares every operation with plain
integer counting per bit position: random words, up to 40 adds per position
(saturation and the wrap of the four planes both occur), merges of saturated
with unsaturated counters, and the order of adds and merges.  What is counted is
the number of arrival lines of one message at one peer in the round it was news
(Peer.py:206, Peer.py:286).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "mult_planes_shim.cpp")

P_U64 = ctypes.POINTER(ctypes.c_ulonglong)


@pytest.fixture(scope="module")
def mp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mult_planes") / "libmult_planes_shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", CSRC, SHIM, "-o", so])
    lib = ctypes.CDLL(so)
    lib.mp_zero.argtypes = [P_U64]
    lib.mp_zero.restype = None
    lib.mp_add.argtypes = [P_U64, P_U64, ctypes.c_int]
    lib.mp_add.restype = None
    lib.mp_add4.argtypes = [P_U64, P_U64, ctypes.c_int]
    lib.mp_add4.restype = None
    lib.mp_merge.argtypes = [P_U64, P_U64]
    lib.mp_merge.restype = None
    lib.mp_masks.argtypes = [P_U64, P_U64]
    lib.mp_masks.restype = None
    return lib


def ptr(a):
    return a.ctypes.data_as(P_U64)


def counter(mp, xs=()):
    """a counter (5 words and a guard word behind them) after one add per word of xs"""
    c = np.full(6, 0xDEAD, np.uint64)
    mp.mp_zero(ptr(c))
    xs = np.ascontiguousarray(xs, np.uint64)
    if xs.size:
        mp.mp_add(ptr(c), ptr(xs), xs.size)
    assert c[5] == 0xDEAD
    return c


def merged(mp, a, b):
    out = a.copy()
    mp.mp_merge(ptr(out), ptr(b))
    assert out[5] == 0xDEAD
    return out


def masks(mp, c):
    out = np.full(18, 0xBEEF, np.uint64)
    mp.mp_masks(ptr(c), ptr(out))
    assert out[17] == 0xBEEF
    return out[:17]


def counts_of(xs):
    """per-bit integer counting: how many of the words have bit b set"""
    cnt = np.zeros(64, np.int64)
    for x in xs:
        for b in range(64):
            cnt[b] += (int(x) >> b) & 1
    return cnt


def expected_masks(cnt):
    out = [0] * 17
    for b in range(64):
        out[min(int(cnt[b]), 16)] |= 1 << b
    return np.array(out, np.uint64)


def check(mp, c, cnt):
    got = masks(mp, c)
    exp = expected_masks(cnt)
    assert np.array_equal(got, exp), [(k, hex(int(got[k])), hex(int(exp[k]))) for k in range(17) if got[k] != exp[k]]
    # the 17 masks partition the word
    assert int(np.bitwise_or.reduce(got)) == (1 << 64) - 1
    assert sum(bin(int(x)).count("1") for x in got) == 64


def words_with_counts(rng, cnt):
    """a shuffled list of words in which bit b is set in exactly cnt[b] of them"""
    n = int(max(cnt.max(), 1))
    xs = [0] * n
    for b in range(64):
        for i in rng.choice(n, int(cnt[b]), replace=False):
            xs[int(i)] |= 1 << b
    return np.array(xs, np.uint64)


def test_constants(mp):
    assert mp.mp_planes() == 4 and mp.mp_words() == 5
    assert mp.mp_sat() == 16 and mp.mp_bins() == 17     # GP_MULT_BINS of the C-ABI
    check(mp, counter(mp), np.zeros(64, np.int64))


def test_random_words(mp):
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 7, 15, 16, 17, 31, 40):
        for _ in range(20):
            xs = rng.integers(0, 1 << 64, n, dtype=np.uint64)
            check(mp, counter(mp, xs), counts_of(xs))


def test_every_count_up_to_40(mp):
    """bit b is added (b % 41) times, and the other way round: every count 0 .. 40
    occurs, so the planes saturate (16), wrap (32) and go on counting"""
    rng = np.random.default_rng(2)
    for flip in (False, True):
        cnt = np.array([(63 - b if flip else b) % 41 for b in range(64)], np.int64)
        xs = words_with_counts(rng, cnt)
        assert np.array_equal(counts_of(xs), cnt) and xs.size == 40
        check(mp, counter(mp, xs), cnt)
    # the same word 40 times: all positions together through 15 -> 16 -> 32 -> 40
    x = 0xF0F0_1234_8000_0001
    for n in range(1, 41):
        check(mp, counter(mp, [x] * n), counts_of([x] * n))


def counter4(mp, xs, start=None):
    """the same adds, four words at a time (mult_add4), on top of the counter `start`"""
    c = counter(mp) if start is None else start.copy()
    xs = np.ascontiguousarray(xs, np.uint64)
    mp.mp_add4(ptr(c), ptr(xs), xs.size)
    assert c[5] == 0xDEAD
    return c


def test_add4_is_four_adds(mp):
    """the carry-save batch of k_mult's gather against one add per word and
    against counting: every batch fill (1 .. 4 words), every count up to 40,
    batches on top of counters at 12 .. 15 (the carry out of plane 3) and of
    saturated ones"""
    rng = np.random.default_rng(7)
    ones = (1 << 64) - 1
    for n in list(range(1, 9)) + [15, 16, 17, 39, 40]:
        for _ in range(10):
            xs = rng.integers(0, 1 << 64, n, dtype=np.uint64)
            assert np.array_equal(counter4(mp, xs), counter(mp, xs))
            check(mp, counter4(mp, xs), counts_of(xs))
    for flip in (False, True):
        cnt = np.array([(63 - b if flip else b) % 41 for b in range(64)], np.int64)
        xs = words_with_counts(rng, cnt)
        check(mp, counter4(mp, xs), cnt)
    for base in range(0, 41):
        start = counter(mp, [ones] * base)
        for k in range(5):                                         # 0 .. 4 of the batch's words hold the position
            batch = [ones] * k + [0] * (4 - k)
            for order in (batch, batch[::-1]):
                got = counter4(mp, order, start)
                check(mp, got, np.full(64, base + k))
                assert np.array_equal(got, counter(mp, [ones] * (base + k)))


def test_add_order(mp):
    rng = np.random.default_rng(3)
    xs = rng.integers(0, 1 << 64, 40, dtype=np.uint64)
    a = counter(mp, xs)
    for _ in range(10):
        got, want = masks(mp, counter(mp, rng.permutation(xs))), masks(mp, a)
        assert np.array_equal(got, want)


def test_merge_against_counting(mp):
    """two counters of up to 40 adds each: the merge holds the sum of the counts,
    whichever of the two is saturated at a position (none, one, both)"""
    rng = np.random.default_rng(4)
    seen = set()
    for _ in range(60):
        ca = rng.integers(0, 41, 64)
        cb = rng.integers(0, 41, 64)
        # some positions stay low so that unsaturated + unsaturated occurs on both sides of 16
        low = rng.random(64) < 0.4
        ca[low] = rng.integers(0, 16, int(low.sum()))
        cb[low] = rng.integers(0, 16, int(low.sum()))
        a, b = counter(mp, words_with_counts(rng, ca)), counter(mp, words_with_counts(rng, cb))
        check(mp, merged(mp, a, b), ca + cb)
        check(mp, merged(mp, b, a), ca + cb)
        for x, y in zip(ca, cb):
            seen.add((x >= 16, y >= 16, x + y >= 16))
    assert seen == {(False, False, False), (False, False, True), (True, False, True), (False, True, True),
                    (True, True, True)}


def test_merge_saturated_with_unsaturated(mp):
    """a saturated counter whose planes have wrapped (count 32: planes 0) merged
    with a small one stays saturated; 15 + 1 saturates; 15 + 0 does not"""
    ones = (1 << 64) - 1
    sat32 = counter(mp, [ones] * 32)
    assert not sat32[:4].any() and int(sat32[4]) == ones          # planes wrapped to 0, sticky set
    for k in (0, 1, 5, 15):
        small = counter(mp, [ones] * k)
        check(mp, merged(mp, sat32, small), np.full(64, 32 + k))
        check(mp, merged(mp, small, sat32), np.full(64, 32 + k))
    fifteen = counter(mp, [ones] * 15)
    check(mp, merged(mp, fifteen, counter(mp)), np.full(64, 15))
    check(mp, merged(mp, fifteen, counter(mp, [ones])), np.full(64, 16))
    check(mp, merged(mp, counter(mp, [ones] * 8), counter(mp, [ones] * 8)), np.full(64, 16))
    check(mp, merged(mp, counter(mp, [ones] * 8), counter(mp, [ones] * 7)), np.full(64, 15))


def test_merge_order_invariance(mp):
    """the words of a long in-list dealt over 8 partial counters, as the row slots
    of a wave or the items of a hub hold them: every merge order and every
    tree shape gives the counter of the plain sequence of adds"""
    rng = np.random.default_rng(5)
    xs = rng.integers(0, 1 << 64, 40, dtype=np.uint64)
    xs[::3] |= np.uint64(0xFFFF)                                    # some positions saturate
    whole = masks(mp, counter(mp, xs))
    assert whole[16] != 0 and whole[1:16].any()
    for _ in range(10):
        deal = rng.integers(0, 8, xs.size)
        parts = [counter(mp, xs[deal == k]) for k in range(8)]
        order = rng.permutation(8)
        acc = counter(mp)
        for k in order:                                             # a chain
            acc = merged(mp, acc, parts[k])
        assert np.array_equal(masks(mp, acc), whole)
        level = [parts[k] for k in order]                           # a butterfly, as over shuffles
        while len(level) > 1:
            level = [merged(mp, level[i], level[i + 1]) for i in range(0, len(level), 2)]
        assert np.array_equal(masks(mp, level[0]), whole)
        check(mp, level[0], counts_of(xs))
