"""The protocol parallel.GridExchange and parallel.WLWindows share through parallel.PairExchange: the log u of an attempt
as a function of seed and attempt, disjoint pairs per move, the attempted / accepted counts, and the one device attempt
(`attempt`) on a stand-in engine that records what it is given.  The moves themselves are pinned class by class in
tests/test_grid_exchange_host.py and tests/test_wl_windows_host.py."""

import numpy as np
import pytest

from smol_amd import parallel

MAKE = {
    "grid": lambda seed: parallel.GridExchange(np.linspace(1000.0, 2000.0, 3), np.zeros((4, 1, 2)), replicas=2, seed=seed),
    "windows": lambda seed: parallel.WLWindows(0, 24, 1, 5, copies=3, seed=seed),
}
CALL = {"grid": "exchange_grid", "windows": "exchange_wl"}
pytestmark = pytest.mark.parametrize("kind", sorted(MAKE))


def test_log_u_is_a_function_of_seed_and_attempt(kind):
    a, b, other = MAKE[kind](5), MAKE[kind](5), MAKE[kind](6)
    assert isinstance(a, parallel.PairExchange) and a.philox_seed == 5
    for attempt in (0, 1, 2, 7, 2 ** 40):
        for n in (0, 1, 4, 9):
            u = a.log_u(attempt, n)
            assert u.shape == (n,) and u.dtype == np.float64 and np.array_equal(u, b.log_u(attempt, n))
            assert np.array_equal(u, np.log(parallel._philox_uniforms(5, attempt, max(n, 1)))[:n])
            assert (u <= 0).all()
        assert not np.array_equal(a.log_u(attempt, 4), a.log_u(attempt + 1, 4))
        assert not np.array_equal(a.log_u(attempt, 4), other.log_u(attempt, 4))
    assert np.array_equal(a.log_u(3, 9)[:4], a.log_u(3, 4))  # (fewer pairs: the first draws of the same attempt)


def test_pairs_of_every_move_are_disjoint(kind):
    x = MAKE[kind](0)
    n = x.npoints if kind == "grid" else x.R
    assert len(x.MOVES) >= 2 and [x.move_of(k) for k in range(2 * len(x.MOVES))] == list(x.MOVES) * 2
    for move in x.MOVES:
        pairs = x.pairs(move)
        assert pairs.dtype == np.int32 and pairs.shape == (len(pairs), 2) and len(pairs) > 0
        assert pairs.min() >= 0 and pairs.max() < n
        assert len(np.unique(pairs)) == pairs.size
        assert x.attempted[move].shape == x.accepted[move].shape == (len(pairs),)
        assert x.pairs(list(move) if kind == "grid" else np.int64(move)) is pairs  # (the key is normalised per class)


def test_record_then_acceptance_is_accepted_over_attempted(kind):
    x = MAKE[kind](0)
    assert x.acceptance == 0.0 and x.calls == 0
    rng = np.random.default_rng(3)
    attempted = accepted = 0
    for k in range(11):
        move = x.move_of(k)
        flags = rng.random(len(x.pairs(move))) < 0.4
        before = x.accepted[move].copy()
        x.record(move, flags)
        assert np.array_equal(x.accepted[move], before + flags)
        attempted, accepted = attempted + len(flags), accepted + int(flags.sum())
    assert accepted > 0 and x.acceptance == accepted / attempted
    for m, move in enumerate(x.MOVES):  # 11 attempts over the moves in turn
        assert np.array_equal(x.attempted[move], np.full(len(x.pairs(move)), len(range(m, 11, len(x.MOVES)))))
    assert x.calls == 0  # (record counts pairs; the attempt counter belongs to whoever drives the attempts)


class _Engine:
    """takes the call of one kind of exchange, keeps its arguments and answers with the given accept flags"""

    def __init__(self, kind, flags):
        self.flags, self.seen = flags, []
        setattr(self, CALL[kind], self._exchange)

    def _exchange(self, pairs, log_u, stats):
        assert stats.dtype == np.int64 and stats.shape == (len(pairs), 2) and not stats.any()
        self.seen.append((np.array(pairs), np.array(log_u)))
        stats[:, 0] += 1
        stats[:, 1] += self.flags[:len(pairs)]


@pytest.mark.parametrize("reindexed", [False, True])
def test_attempt_is_one_call_of_the_move_whose_turn_it_is(kind, reindexed):
    x, ref = MAKE[kind](9), MAKE[kind](9)
    n = x.npoints if kind == "grid" else x.R
    entry = np.random.default_rng(1).permutation(n) if reindexed else None
    flags = (np.arange(n) % 3 == 0).astype(np.int64)
    eng = _Engine(kind, flags)
    for k in range(2 * len(x.MOVES) + 1):
        x.attempt(eng, entry) if reindexed else x.attempt(eng)
        move = ref.move_of(k)
        pairs, log_u = eng.seen[-1]
        assert len(eng.seen) == k + 1 == x.calls
        assert np.array_equal(pairs, entry[ref.pairs(move)] if reindexed else ref.pairs(move))
        assert np.array_equal(log_u, ref.log_u(k, len(ref.pairs(move))))
        ref.record(move, flags[:len(pairs)])
    for move in x.MOVES:
        assert np.array_equal(x.attempted[move], ref.attempted[move]) and np.array_equal(x.accepted[move], ref.accepted[move])
    assert x.acceptance == ref.acceptance > 0
