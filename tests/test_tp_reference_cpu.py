"""tests/tp_reference.py without a GPU: the rank-ordered fp32 sum on the special values, and the greedy rule over the
ranks' pairs against a brute-force argmax over the whole row."""
import numpy as np
import pytest

from tests import tp_reference as T

F32 = np.float32


def test_rank_ordered_sum_on_the_specials():
    x0, x1 = T.specials(2)
    got = T.rank_ordered_sum([x0, x1])
    assert got.dtype == F32
    # element by element against the float64 sum rounded to fp32: 0 + x_0 is x_0 (but for -0, which becomes +0), and a
    # sum of two fp32 values rounded to 53 bits and then to 24 is the correctly rounded fp32 sum (53 >= 2 * 24 + 2)
    with np.errstate(over="ignore", invalid="ignore"):
        want = ((0.0 + x0.astype(np.float64)) + x1.astype(np.float64)).astype(F32)
    assert T.same_bits(got, want)
    by_pair = {(a.tobytes(), b.tobytes()): g for a, b, g in zip(x0, x1, got)}
    at = lambda a, b: by_pair[(F32(a).tobytes(), F32(b).tobytes())]  # noqa: E731
    big, least = np.finfo(F32).max, np.nextafter(F32(0), F32(1))
    assert at(-0.0, -0.0) == 0 and not np.signbit(at(-0.0, -0.0))  # the sum starts at +0
    assert not np.signbit(at(0.0, -0.0)) and not np.signbit(at(1.0, -1.0))
    assert at(least, least) == 2 * least and at(1e-42, 1e-42) == F32(1e-42) * 2  # subnormals are kept
    assert at(big, big) == np.inf and at(-big, -big) == -np.inf and at(big, -big) == 0
    assert at(big, 2.0 ** 103) == np.inf and at(big, 2.0 ** 102) == big  # half an ulp ties to even: over; below: stays
    assert np.isnan(at(np.inf, -np.inf)) and np.isnan(at(-np.inf, np.inf)) and at(np.inf, -big) == np.inf
    assert np.isnan(at(np.nan, 1.0)) and np.isnan(at(1.0, np.nan)) and np.isnan(at(np.nan, np.inf))
    assert at(1.0, 2.0 ** -24) == 1 and at(1.0, 2.0 ** -24 + 2.0 ** -40) == np.nextafter(F32(1), F32(2))
    assert T.same_bits(got, got) and not T.same_bits(got, np.where(np.isnan(got), F32(0), got))
    neg0 = np.array([-0.0], F32)
    assert not T.same_bits(neg0, np.array([0.0], F32))  # bits, not values


def test_rank_order_matters_from_three_addends_on():
    rng = np.random.default_rng(0)
    xs = [(rng.standard_normal(4096) * np.exp2(rng.uniform(-60, 60, 4096))).astype(F32) for _ in range(4)]
    fwd, rev = T.rank_ordered_sum(xs), T.rank_ordered_sum(xs[::-1])
    assert not np.array_equal(fwd, rev)
    assert np.array_equal(T.rank_ordered_sum(xs[:2]), T.rank_ordered_sum(xs[1::-1]))  # two addends commute
    x64 = np.sum([x.astype(np.float64) for x in xs], axis=0)
    scale = np.sum([np.abs(x).astype(np.float64) for x in xs], axis=0)
    assert (np.abs(fwd - x64) <= 3 * 2.0 ** -24 * scale).all()
    four = T.specials(4)
    assert len(four) == 4 and T.same_bits(T.rank_ordered_sum(four), T.rank_ordered_sum(four[:2]))


def _brute(row):
    """lowest index of the largest number of the row; NaN and -inf never win"""
    ok = ~np.isnan(row) & (row > -np.inf)
    if not ok.any():
        return 0, T.STATUS_NO_WINNER
    m = row[ok].max()
    return int(np.flatnonzero(ok & (row == m))[0]), 0


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("local_vocab", [16, 100, 384])
def test_greedy_pick_is_the_argmax_of_the_gathered_row(world, local_vocab):
    rng = np.random.default_rng(local_vocab * 10 + world)
    offsets = [r * local_vocab for r in range(world)]
    for trial in range(40):
        row = rng.standard_normal(world * local_vocab).astype(F32)
        kind = trial % 8
        if kind == 1:  # ties across ranks and inside one
            row[rng.integers(0, row.size, 6)] = 7.0
        elif kind == 2:
            row[:local_vocab] = -np.inf
        elif kind == 3:
            row[local_vocab:2 * local_vocab] = np.nan
        elif kind == 4:
            row[:] = np.nan
        elif kind == 5:
            row[:] = -np.inf
        elif kind == 6:
            row[rng.integers(0, row.size, row.size // 2)] = np.nan
            row[rng.integers(0, row.size, 5)] = np.inf
        elif kind == 7:
            row[:] = np.where(rng.random(row.size) < 0.5, np.nan, -np.inf)
        shards = [T.pairs_of(row[o:o + local_vocab]) for o in offsets]
        got = T.greedy_pick([s[0] for s in shards], [s[1] for s in shards], offsets)
        assert got == _brute(row), (trial, kind)
        # the order in which a rank lists its pairs does not matter
        perm = rng.permutation(shards[0][0].size)
        got = T.greedy_pick([s[0][perm] for s in shards], [s[1][perm] for s in shards], offsets)
        assert got == _brute(row), (trial, kind)


def test_greedy_pick_edges():
    s = T.SENTINEL
    ninf, nan = -np.inf, np.nan
    one = lambda v, i: (np.array([v], F32), np.array([i], np.int32))  # noqa: E731
    pick = lambda a, b: T.greedy_pick([a[0], b[0]], [a[1], b[1]], [0, 100])  # noqa: E731
    assert pick(one(1.0, 5), one(1.0, 2)) == (5, 0)  # equal maxima: the lowest GLOBAL index (102 loses)
    assert pick(one(ninf, s), one(0.5, 2)) == (102, 0)
    assert pick(one(nan, 3), one(-3.0, 2)) == (102, 0)
    assert pick(one(nan, 3), one(nan, 2)) == (0, 4) and pick(one(ninf, s), one(ninf, s)) == (0, 4)
    assert pick(one(ninf, s), one(ninf, 7)) == (107, 0)  # -inf under a real index is a candidate
    assert T.pairs_of(np.full(20, ninf, F32))[1].tolist() == [s, s]
    pm, pi = T.pairs_of(np.array([nan] * 15 + [2.0] + [3.0, 3.0, nan], F32), offset=0)
    assert pm.tolist() == [2.0, 3.0] and pi.tolist() == [15, 16]
