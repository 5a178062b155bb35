"""The state-key contract on the host (include/ngw.h ngw_state_keys; state_keys.py keys_of_rows / unique_of_keys / check_fields): the known
answers, the numpy twin against the plain-integer oracle (tests/state_key_oracle.py), what a key must and must not depend on.  No GPU."""
import os
import re

import numpy as np
import pytest

import state_key_oracle as KO
import gym_novel_gridworlds_amd as G
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.state_keys import check_fields, keys_of_rows, unique_of_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 17
FIELDS = (1, 2, 4, 8, 16, 32, 15, 63, 6)


def empty_rows(n, S):
    """n never-saved slots: zeros, the agent at (1, 1)."""
    return {'map': np.zeros((n, S * S), np.int8), 'loc': np.ones((n, 2), np.int32), 'facing': np.zeros(n, np.int32),
            'inv': np.zeros((n, K), np.int32), 'selected': np.zeros(n, np.int32), 'step_count': np.zeros(n, np.int32),
            'episode': np.zeros(n, np.uint32)}


def random_rows(n, S, rs):
    inv = rs.randint(0, 4, (n, K)).astype(np.int32)              # about a quarter of the entries 0 ...
    big = rs.rand(n, K) < 0.2
    inv[big] = rs.randint(256, 1 << 20, int(big.sum()))          # ... and values above 255
    step, ep = rs.randint(0, 1 << 31, n, dtype=np.int64), rs.randint(0, (1 << 31) + 1, n, dtype=np.int64)
    step[0], ep[0] = (1 << 31) - 1, 1 << 31                       # (the ends of the ranges)
    return {'map': rs.randint(0, K, (n, S * S)).astype(np.int8), 'loc': rs.randint(1, S - 1, (n, 2)).astype(np.int32),
            'facing': rs.randint(0, 4, n).astype(np.int32), 'inv': inv, 'selected': rs.randint(0, K, n).astype(np.int32),
            'step_count': step.astype(np.int32), 'episode': ep.astype(np.uint32)}


def test_the_known_answers():
    rows = empty_rows(1, 10)
    for impl in (lambda f: int(keys_of_rows(rows, f)[0]), lambda f: KO.key_of_row(rows, 0, f)):
        assert impl(G.KEY_STATE) == 0x43fc77d84676ced7
        assert impl(G.KEY_ALL) == 0x832aebfd8bded47c
    assert KO.term(1, 20, 5) == 0xa63311a5fe432d5f
    nine = empty_rows(1, 9)
    nine['map'][0, 80] = 5                                      # a 9 x 9 map whose only non-air cell is the last one: group 20 holds one cell
    assert int(keys_of_rows(nine, G.KEY_MAP)[0]) == 0xa63311a5fe432d5f == KO.key_of_row(nine, 0, KO.MAP)


def test_the_constants():
    assert (G.KEY_MAP, G.KEY_POSE, G.KEY_INV, G.KEY_SELECTED, G.KEY_STEP_COUNT, G.KEY_EPISODE) == KO.SINGLE == (1, 2, 4, 8, 16, 32)
    assert G.KEY_STATE == 15 and G.KEY_ALL == 63
    text = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    for name, value in (('MAP', 1), ('POSE', 2), ('INV', 4), ('SELECTED', 8), ('STEP_COUNT', 16), ('EPISODE', 32), ('STATE', 15), ('ALL', 63)):
        assert re.search(r'#define\s+NGW_KEY_%s\s+%du\b' % (name, value), text), name
    assert re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', text)


@pytest.mark.parametrize('S', [9, 10, 12])
@pytest.mark.parametrize('fields', FIELDS)
def test_the_numpy_twin_equals_the_oracle(S, fields):
    rows = random_rows(40, S, np.random.RandomState(100 * S + fields))
    got = keys_of_rows(rows, fields)
    assert got.dtype == np.uint64 and got.shape == (40,)
    KO.assert_keys(got, rows, np.arange(40), fields, 'S=%d' % S)
    square = dict(rows, map=rows['map'].reshape(40, S, S))       # (the [n, S, S] shape of an observation)
    assert (keys_of_rows(square, fields) == got).all()


@pytest.mark.parametrize('fields', FIELDS)
def test_a_key_changes_exactly_with_the_selected_fields(fields):
    """One field of one row changed at a time (a map cell, each pose component, an inventory entry from and to 0, ...): the key differs
    exactly when that field's bit is in `fields`."""
    rs = np.random.RandomState(fields)
    S = 9
    rows = random_rows(1, S, rs)
    base = int(keys_of_rows(rows, fields)[0])
    edits = [('map', (0, 80), 3 if rows['map'][0, 80] != 3 else 4), ('map', (0, 0), 0 if rows['map'][0, 0] else 1),
             ('loc', (0, 0), int(rows['loc'][0, 0]) % (S - 2) + 1), ('loc', (0, 1), int(rows['loc'][0, 1]) % (S - 2) + 1),
             ('facing', (0,), (int(rows['facing'][0]) + 1) % 4), ('inv', (0, 3), int(rows['inv'][0, 3]) + 1),
             ('inv', (0, K - 1), 0 if rows['inv'][0, K - 1] else 7), ('selected', (0,), (int(rows['selected'][0]) + 1) % K),
             ('step_count', (0,), 5), ('episode', (0,), 6)]
    for name, at, value in edits:
        changed = {k: x.copy() for k, x in rows.items()}
        assert changed[name][at] != value
        changed[name][at] = value
        differs = int(keys_of_rows(changed, fields)[0]) != base
        assert differs == bool(fields & KO.FIELD_OF[name]), (name, at)
        assert KO.key_of_row(changed, 0, fields) == int(keys_of_rows(changed, fields)[0])


@pytest.mark.parametrize('S', [9, 10])
def test_the_incremental_identity(S):
    """Two rows that differ in one cell: the XOR of their keys is the XOR of that one group's two terms."""
    rs = np.random.RandomState(S)
    rows = random_rows(1, S, rs)
    for cell in (0, 5, S * S - 1):
        other = {k: x.copy() for k, x in rows.items()}
        other['map'][0, cell] = (int(rows['map'][0, cell]) + 1) % K
        g = cell // 4
        w0, w1 = (KO.map_group_word(r['map'][0], g) for r in (rows, other))
        expect = (KO.term(1, g, w0) if w0 else 0) ^ (KO.term(1, g, w1) if w1 else 0)
        for f in (G.KEY_MAP, G.KEY_STATE, G.KEY_ALL):
            assert int(keys_of_rows(rows, f)[0]) ^ int(keys_of_rows(other, f)[0]) == expect, (cell, f)


@pytest.mark.parametrize('bad', [0, 64, 128, 1 << 32, -1, 1.0, None, True])
def test_bad_fields_raise(bad):
    with pytest.raises(ValueError, match='fields'):
        check_fields(bad)
    with pytest.raises(ValueError, match='fields'):
        keys_of_rows(empty_rows(2, 9), bad)


def test_unique_returns_the_smallest_positions():
    keys = np.array([7, 1 << 63, 7, 3, 1 << 63, 7, 0, 3], np.uint64)
    first, inverse = unique_of_keys(keys)
    assert first.dtype == np.int64 and inverse.dtype == np.int64 and inverse.shape == (8,)
    assert sorted(first.tolist()) == [0, 1, 3, 6]
    for j in range(8):
        assert keys[first[inverse[j]]] == keys[j] and first[inverse[j]] <= j
        assert first[inverse[j]] == min(i for i in range(8) if keys[i] == keys[j])
    first, inverse = unique_of_keys(np.zeros(0, np.uint64))
    assert first.shape == (0,) and inverse.shape == (0,)


def test_the_header_declares_the_symbol_and_the_ctypes_table_lists_it():
    text = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+ngw_state_keys\s*\(', text)
    L = _cabi.lib()
    assert 'ngw_state_keys' in _cabi.SYMBOLS and hasattr(L, 'ngw_state_keys')
    assert len(L.ngw_state_keys.argtypes) == 6
