"""frontier.compact_reference / alloc_reference held to tests/frontier_oracle.py - the contract of include/ngw.h in plain Python loops, which the
search fuzz's model uses in their place - over the edge list of tests/test_frontier.py: its lengths, flag contents, div, map and capacities, and
every cursor / limit pair of its allocation test.  No GPU."""
import numpy as np
import pytest

import frontier_oracle as FO
from gym_novel_gridworlds_amd import frontier as F
from gym_novel_gridworlds_amd.spec import F_FRONTIER_FULL, IDX_NONE

TILE = 4096


def flag_cases(n, rs):
    """tests/test_frontier.py's flag contents: none, all, sparse, stray non-zero bytes."""
    yield 'none', np.zeros(n, np.uint8)
    yield 'all', np.ones(n, np.uint8)
    f = (rs.randint(0, 17, n) == 0).astype(np.uint8)
    yield 'sparse', f
    g = f.copy()
    if n:
        g[rs.randint(0, n, 6)] = np.array([2, 0x80, 0xFF, 2, 0x80, 0xFF], np.uint8)
    yield 'stray', g


def test_the_constants():
    assert FO.IDX_NONE == IDX_NONE and FO.F_FRONTIER_FULL == F_FRONTIER_FULL


@pytest.mark.parametrize('n', [0, 1, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 64 * 17])
def test_compact_reference_against_the_oracle(n):
    rs = np.random.RandomState(100 + n)
    for name, flags in flag_cases(n, rs):
        total = int(np.count_nonzero(flags))
        for div in (1, 17):
            amap = (rs.permutation(-(-n // div) + 3) + 7).astype(np.int32)
            for m in (None, amap):
                for cap in sorted({max(total - 1, 0), total, total + 70}) + [None]:
                    where = 'n %d %s div %d map %s capacity %s' % (n, name, div, m is not None, cap)
                    first, second, count, full = F.compact_reference(flags, div, m, cap)
                    e_first, e_second, e_count, e_full = FO.compact(flags, div, m, cap)
                    assert first.dtype == e_first.dtype and first.shape == e_first.shape and second.shape == e_second.shape, where
                    assert (first == e_first).all() and (second == e_second).all(), where
                    assert count.tolist() == e_count and bool(full) == e_full, where
    flags = rs.randint(0, 5, n) == 0                                         # bool flags of two dimensions read flattened
    a, b = F.compact_reference(flags.reshape(1, -1), 17, None, n + 3), FO.compact(flags.reshape(1, -1), 17, None, n + 3)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tolist() == b[2] and bool(a[3]) == b[3]


@pytest.mark.parametrize('cursor, limit', [(0, 512), (37, 512), (0, 9), (3, 12), (3, 11), (3, 4), (12, 12), (20, 12)])
def test_alloc_reference_against_the_oracle(cursor, limit):
    for count, capacity in ((9, 16), (0, 16), (16, 16), (9, 9), (0, 0)):
        slots, after, full = F.alloc_reference(count, cursor, limit, capacity)
        e_slots, e_after, e_full = FO.alloc(count, cursor, limit, capacity)
        assert slots.dtype == e_slots.dtype and slots.shape == e_slots.shape and (slots == e_slots).all(), (count, capacity)
        assert after == e_after and bool(full) == e_full, (count, capacity)
