"""spread.py on hand-made curves: the helpers that turn a spread curve
(GossipEngine.curve(): first receipts per receipt round and message, the
aggregate of each reference peer's arrival log, Peer.py:175-216) into coverage
per round and rounds-to-reach, counted from each message's inject round."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def spread(pkg):
    return pkg.spread


# 10 vertices.  Message 0: injected in round 0, reaches all by round 3.
# Message 1: injected in round 2, reaches 8.  Message 2: lost (never exists).
# Message 3: injected in round 1, stuck at its origin.
CURVE = np.array([[1, 0, 0, 0],
                  [3, 0, 0, 1],
                  [4, 1, 0, 0],
                  [2, 2, 0, 0],
                  [0, 5, 0, 0]], dtype=np.uint64)
INJECT = np.array([0, 2, 0, 1])


def test_cumulative(spread):
    cum = spread.cumulative(CURVE)
    assert cum.dtype == np.int64 and cum.shape == CURVE.shape
    assert cum[:, 0].tolist() == [1, 4, 8, 10, 10]
    assert cum[:, 1].tolist() == [0, 0, 1, 3, 8]
    assert cum[:, 2].tolist() == [0, 0, 0, 0, 0]
    assert cum[-1].tolist() == [10, 8, 0, 1]
    with pytest.raises(ValueError):
        spread.cumulative(np.zeros(4))


def test_rounds_to_reach_final_with_staggered_injects(spread):
    # half of the final coverage: 5 of 10 at round 2; 4 of 8 at round 4, 2 after its inject round
    assert spread.rounds_to_reach(CURVE, INJECT, 0.5).tolist() == [2, 2, -1, 0]
    assert spread.rounds_to_reach(CURVE, INJECT, 1.0).tolist() == [3, 2, -1, 0]
    # 90 % of 10 is 9 -> round 3; 90 % of 8 is 7.2 -> 8 vertices, round 4
    assert spread.rounds_to_reach(CURVE, INJECT, 0.9, of="final").tolist() == [3, 2, -1, 0]
    # the smallest share still needs one holder: the inject round itself
    assert spread.rounds_to_reach(CURVE, INJECT, 0.01).tolist() == [0, 0, -1, 0]


def test_rounds_to_reach_of_n(spread):
    # of n = 10: message 1 stops at 8 (never 90 %), message 3 at 1 (10 % only)
    assert spread.rounds_to_reach(CURVE, INJECT, 0.9, of=10).tolist() == [3, -1, -1, -1]
    assert spread.rounds_to_reach(CURVE, INJECT, 0.8, of=10).tolist() == [2, 2, -1, -1]
    assert spread.rounds_to_reach(CURVE, INJECT, 0.1, of=10).tolist() == [0, 0, -1, 0]
    assert spread.rounds_to_reach(CURVE, None, 0.8, of=10).tolist() == [2, 4, -1, -1]


def test_lost_message_and_bad_arguments(spread):
    lost = np.zeros((6, 3), np.uint64)
    assert spread.rounds_to_reach(lost, [0, 1, 2], 0.5).tolist() == [-1, -1, -1]
    assert spread.rounds_to_reach(lost, [0, 1, 2], 0.5, of=4).tolist() == [-1, -1, -1]
    with pytest.raises(ValueError):
        spread.rounds_to_reach(CURVE, INJECT[:3], 0.5)
    with pytest.raises(ValueError):
        spread.rounds_to_reach(CURVE, INJECT, 0.0)
    with pytest.raises(ValueError):
        spread.rounds_to_reach(CURVE, INJECT, 0.5, of="n")
    with pytest.raises(ValueError):
        spread.rounds_to_reach(CURVE, INJECT, 0.5, of=0)


def test_uint64_counts_do_not_wrap(spread):
    big = np.array([[2 ** 40], [2 ** 40]], dtype=np.uint64)
    assert spread.cumulative(big)[-1, 0] == 2 ** 41
    assert spread.rounds_to_reach(big, [0], 0.75).tolist() == [1]
