"""orip.stages.subsample_indices keeps the fixed-seed subsample of stage 02 (02:39-44) per (n, limit): the same values as a fresh draw, one shared
read-only array per key, at most four keys."""
import numpy as np
import pytest

from orip import stages as S


@pytest.fixture(autouse=True)
def empty_memo():
    S._SUBSAMPLE_MEMO.clear()
    yield
    S._SUBSAMPLE_MEMO.clear()


@pytest.mark.parametrize("n,limit", [(5_000, 1_000), (200_001, 200_000), (1 << 20, 200_000)])
def test_equals_a_fresh_draw_and_is_shared(n, limit):
    want = np.random.default_rng(42).choice(n, limit, replace=False)
    got = S.subsample_indices(n, limit)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert S.subsample_indices(n, limit) is got                 # the second call: the same object
    assert not got.flags.writeable
    with pytest.raises(ValueError):
        got[0] = 0
    assert np.array_equal(got, want)


def test_default_limit_is_the_reference_one():
    assert S.subsample_indices(200_001) is S.subsample_indices(200_001, 200_000)
    assert S.SUBSAMPLE_LIMIT == 200_000


@pytest.mark.parametrize("n,limit", [(1_000, 1_000), (999, 1_000), (1, 200_000), (200_000, 200_000)])
def test_no_subsample_at_or_below_the_limit(n, limit):
    assert S.subsample_indices(n, limit) is None
    assert not S._SUBSAMPLE_MEMO


def test_fifth_key_evicts_the_oldest():
    keys = [(2_000 + i, 100) for i in range(5)]
    first = [S.subsample_indices(*k) for k in keys[:4]]
    assert list(S._SUBSAMPLE_MEMO) == keys[:4]
    assert all(S.subsample_indices(*k) is a for k, a in zip(keys[:4], first))      # hits move nothing: still oldest first
    S.subsample_indices(*keys[4])
    assert list(S._SUBSAMPLE_MEMO) == keys[1:]
    again = S.subsample_indices(*keys[0])                                           # drawn anew: equal, another object; evicts the next oldest
    assert again is not first[0] and np.array_equal(again, first[0])
    assert list(S._SUBSAMPLE_MEMO) == keys[2:] + [keys[0]]
    assert S.subsample_indices(*keys[2]) is first[2]
