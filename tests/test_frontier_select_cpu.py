"""frontier.select_reference - the numpy statement of ngw_frontier_select (include/ngw.h) - against a brute-force statement written here with
Python's sorted() on (value, position) tuples, and the argument checks of the reference and of Frontier.select that run without a device.  No
GPU needed."""
import numpy as np
import pytest

from gym_novel_gridworlds_amd import frontier as F
from gym_novel_gridworlds_amd.key_table import VALUE_NONE
from gym_novel_gridworlds_amd.spec import IDX_NONE

PATTERNS = ('equal', 'two', 'range4', 'full', 'none')


def pattern(name, n, rs):
    if name == 'equal':
        return np.full(n, 7, np.int32)
    if name == 'two':
        return rs.choice(np.array([-3, 12], np.int32), n)
    if name == 'range4':
        return rs.randint(100, 104, n).astype(np.int32)
    if name == 'full':
        v = rs.randint(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)                 # (the upper end is exclusive: VALUE_NONE is not drawn here)
        if n:
            v[rs.randint(0, n, 3)] = np.array([-2 ** 31, 2 ** 31 - 2, VALUE_NONE], np.int32)
        return v
    return np.full(n, VALUE_NONE, np.int32)


def brute(values, keep, div, amap, flags, groups, largest, capacity):
    m = len(values) // groups
    first, second = [IDX_NONE] * capacity, [IDX_NONE] * capacity
    taken, bound, candidates = [], [], 0
    for g in range(groups):
        cand = [(int(values[p]), p) for p in range(g * m, (g + 1) * m) if values[p] != VALUE_NONE and (flags is None or flags[p] != 0)]
        candidates += len(cand)
        ordered = sorted(cand, key=lambda vp: (-vp[0] if largest else vp[0], vp[1]))[:keep]
        taken.append(len(ordered))
        bound.append(ordered[-1][0] if ordered else VALUE_NONE)
        for i, p in enumerate(sorted(p for _, p in ordered)):
            first[g * keep + i] = int(amap[p // div]) if amap is not None else p // div
            second[g * keep + i] = p % div
    return first, second, taken, bound, [taken[0] if groups == 1 else groups * keep, candidates]


def test_reference_against_brute_force():
    rs = np.random.RandomState(2024)
    seen = set()
    for case in range(600):
        name = PATTERNS[case % len(PATTERNS)]
        m, groups = int(rs.randint(0, 41)), int(rs.randint(1, 5))
        keep, div, largest = int(rs.randint(0, m + 3)), int(rs.choice([1, 3, 17])), bool(rs.randint(0, 2))
        n = m * groups
        values = pattern(name, n, rs)
        flags = None if rs.randint(0, 2) else rs.choice(np.array([0, 0, 1, 2, 0x80, 0xFF], np.uint8), n)
        amap = None if rs.randint(0, 2) else (rs.permutation(-(-n // div) + 2) + 5).astype(np.int32)
        capacity = groups * keep + int(rs.choice([0, 9]))
        got = F.select_reference(values.reshape(groups, m), keep, div, amap, flags, groups, largest, capacity)
        want = brute(values, keep, div, amap, flags, groups, largest, capacity)
        where = 'case %d %s m %d groups %d keep %d div %d largest %s' % (case, name, m, groups, keep, div, largest)
        for a, b in zip(got, want):
            assert a.dtype == np.int32 and a.tolist() == b, where
        seen.add((name, largest, flags is None, amap is None))
    assert len(seen) == len(PATTERNS) * 8
    # capacity None: groups * keep entries
    assert F.select_reference(np.arange(6, dtype=np.int32), 2, groups=3)[0].tolist() == [0, 1, 2, 3, 4, 5]


def test_ties_at_the_cut_go_to_the_smaller_position():
    v = np.array([5, 3, 3, 7, VALUE_NONE, 3, 1, 9], np.int32)
    first, second, taken, bound, count = F.select_reference(v, 3)
    assert first.tolist() == [1, 2, 6] and second.tolist() == [0, 0, 0] and taken.tolist() == [3] and bound.tolist() == [3] and count.tolist() == [3, 7]
    first, _, taken, bound, _ = F.select_reference(v, 3, largest=True)
    assert first.tolist() == [0, 3, 7] and bound.tolist() == [5]
    first, _, taken, bound, count = F.select_reference(v, 0)
    assert first.size == 0 and taken.tolist() == [0] and bound.tolist() == [VALUE_NONE] and count.tolist() == [0, 7]


def test_reference_argument_checks():
    v = np.arange(12, dtype=np.int32)
    with pytest.raises(ValueError, match='keep'):
        F.select_reference(v, 5, groups=3, capacity=14)              # groups * keep > capacity
    with pytest.raises(ValueError, match='groups'):
        F.select_reference(v, 1, groups=5)                           # n not divisible
    with pytest.raises(ValueError, match='groups'):
        F.select_reference(v, 1, groups=0)
    with pytest.raises(ValueError, match='values'):
        F.select_reference(v.astype(np.int64), 1)
    with pytest.raises(ValueError, match='keep'):
        F.select_reference(v, -1)
    with pytest.raises(ValueError, match='div'):
        F.select_reference(v, 1, div=0)
    with pytest.raises(ValueError, match='flags'):
        F.select_reference(v, 1, flags=np.ones(11, np.uint8))
    with pytest.raises(ValueError, match='map'):
        F.select_reference(v, 1, div=3, map=np.zeros(3, np.int32))


def test_the_checks_select_shares_with_the_reference():
    """Frontier.select validates through check_select before anything reaches the device."""
    assert F.check_select(12, 3, 4, 12) == (3, 4, 4)
    with pytest.raises(ValueError, match='keep'):
        F.check_select(12, 3, 5, 14)
    with pytest.raises(ValueError, match='groups'):
        F.check_select(12, 5, 1, 100)
    with pytest.raises(ValueError, match='values'):
        F.check_select((1 << 24) + 1, 1, 1, 100)
    with pytest.raises(ValueError, match='keep'):
        F.check_select(12, 1, True, 100)
    assert F.SELECT_WAVE_MAX == 1024 and F.Selected._fields == ('first', 'second', 'taken', 'bound')


def test_the_library_exports_the_symbol():
    from gym_novel_gridworlds_amd import _cabi
    assert 'ngw_frontier_select' in _cabi.SYMBOLS and hasattr(_cabi.lib(), 'ngw_frontier_select')
