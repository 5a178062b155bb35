"""The device-side key table and Snapshot.copy, host side (no GPU): the C-ABI and Python surfaces, the host checks of a key list and of
a slot-to-slot copy's lists on stand-ins that look open (tests/key_table_oracle.py), the buckets arithmetic, and the model itself against
np.unique on one batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import key_table_oracle as KT
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.key_table import KeyInsert, KeyTable, buckets_for, check_keys
from gym_novel_gridworlds_amd.snapshot import check_copy, tensor_len
from gym_novel_gridworlds_amd.state_keys import unique_of_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_API = {'ngw_key_table_create': 3, 'ngw_key_table_destroy': 2, 'ngw_key_table_clear': 2, 'ngw_key_table_insert': 6,
             'ngw_key_table_lookup': 5, 'ngw_key_table_count': 3, 'ngw_snapshot_copy': 6}


def test_header_declares_and_library_exports_the_api():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    L = _cabi.lib()
    for name, n_args in TABLE_API.items():
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert name in _cabi.SYMBOLS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    assert re.search(r'#define\s+NGW_F_TABLE_FULL\s+8u', text) and re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', text)
    from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, F_TABLE_FULL
    assert (F_BAD_INDEX, F_TABLE_FULL) == (4, 8)
    assert L.ngw_abi_version() == 3


def test_null_arguments_are_refused_without_a_device():
    L = _cabi.lib()
    out, n = C.c_void_p(), C.c_int64()
    assert L.ngw_key_table_create(None, 4, C.byref(out)) == -1
    assert L.ngw_key_table_destroy(None, None) == -1 and L.ngw_key_table_clear(None, None) == -1
    assert L.ngw_key_table_insert(None, None, None, 1, None, None) == -1
    assert L.ngw_key_table_lookup(None, None, None, 1, None) == -1
    assert L.ngw_key_table_count(None, None, C.byref(n)) == -1
    assert L.ngw_snapshot_copy(None, None, None, None, None, 1) == -1


def test_python_surface():
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.snapshot import Snapshot
    for cls, names in ((VecNovelGridworld, ('key_table', 'insert_state_keys')), (ShardedVecNovelGridworld, ('key_table', 'insert_state_keys')),
                       (Snapshot, ('copy', 'insert_keys')), (KeyTable, ('insert', 'lookup', 'clear', 'close', '__len__'))):
        for name in names:
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    assert KeyInsert._fields == ('where', 'fresh')
    assert 'race' in KeyTable.insert.__doc__ and 'not part of the contract' in KeyTable.insert.__doc__


@pytest.mark.parametrize('capacity, buckets', [(1, 2), (2, 4), (3, 8), (4, 8), (5, 16), (1024, 2048), (1025, 4096), (700, 2048), (1 << 29, 1 << 30)])
def test_buckets_arithmetic(capacity, buckets):
    """The smallest power of two >= 2 * capacity."""
    assert buckets_for(capacity) == buckets
    assert buckets >= 2 * capacity and buckets & (buckets - 1) == 0 and buckets // 2 < 2 * capacity
    assert KT.stand_in_table(capacity).buckets == buckets


@pytest.mark.parametrize('bad', [0, -1, (1 << 29) + 1])
def test_bad_capacity_raises(bad):
    with pytest.raises(ValueError, match='capacity'):
        buckets_for(bad)


def test_key_list_checks():
    k, n = check_keys(np.array([1, (1 << 64) - 1, 1 << 63], np.uint64))
    assert n == 3 and k.dtype == np.int64 and k.flags['C_CONTIGUOUS'] and k.tolist() == [1, -1, -(1 << 63)]       # the same 64 bits
    k, n = check_keys(np.array([5, -1], np.int64))
    assert k.dtype == np.int64 and k.tolist() == [5, -1]
    k, n = check_keys([3, 4, 3])
    assert n == 3 and k.dtype == np.int64 and k.tolist() == [3, 4, 3]
    k, n = check_keys(np.arange(10, dtype=np.uint64)[::2])                  # (a strided view is made contiguous)
    assert k.flags['C_CONTIGUOUS'] and k.tolist() == [0, 2, 4, 6, 8]
    assert check_keys(np.array([7, 8], np.int32))[0].dtype == np.int64     # narrower integers widen
    k, n = check_keys([])
    assert n == 0 and k.dtype == np.int64 and k.shape == (0,)
    for bad in ([0.5, 1.0], np.zeros(3, np.float32), ['a'], [True, False]):
        with pytest.raises(ValueError, match='integer'):
            check_keys(bad)
    for bad in (np.zeros((2, 2), np.uint64), 3, np.uint64(3)):
        with pytest.raises(ValueError, match='one-dimensional'):
            check_keys(bad)
    with pytest.raises(ValueError, match='keys'):
        check_keys(None)


def test_a_stand_in_table_checks_before_anything_launches():
    """dtype, dimensions, a tensor on the wrong device or of the wrong kind, and use of a closed table - through insert() and lookup()."""
    import torch
    t = KT.stand_in_table(8)
    for call in (t.insert, t.lookup):
        with pytest.raises(ValueError, match='integer'):
            call(np.zeros(3, np.float64))
        with pytest.raises(ValueError, match='one-dimensional'):
            call(np.zeros((2, 3), np.uint64))
        with pytest.raises(ValueError, match='int64 tensor on cuda:0'):
            call(torch.zeros(4, dtype=torch.int64))                        # on the host: the wrong device
        with pytest.raises(ValueError, match='int64 tensor on cuda:0'):
            call(torch.zeros(4, dtype=torch.int32))
    dev = torch.device('cuda:0')
    for bad in (torch.zeros((2, 2), dtype=torch.int64), torch.zeros(8, dtype=torch.int64)[::2], torch.zeros(4, dtype=torch.float32)):
        with pytest.raises(ValueError, match='contiguous one-dimensional int64'):
            tensor_len(dev, 'keys', bad, 'int64')
    assert tensor_len(dev, 'keys', [1, 2], 'int64') is None                 # (no tensor: the host checks take it)
    with pytest.raises(ValueError, match='contiguous one-dimensional int32'):
        tensor_len(dev, 'slots', torch.zeros(4, dtype=torch.int64))         # (index lists stay int32)
    assert not t.closed
    t._invalidate()
    assert t.closed
    for call in (lambda: t.insert([1]), lambda: t.lookup([1]), lambda: len(t), t.clear):
        with pytest.raises(ValueError, match='closed'):
            call()
    t.close()                                                               # (closing twice is fine)
    gone = KT.stand_in_table(8)
    gone.env._h = None                                                      # the env was closed under it
    with pytest.raises(ValueError, match='closed'):
        gone.insert([1])
    other = KT.stand_in_table(8)
    with pytest.raises(ValueError, match='another env'):
        KT.stand_in_snapshot(4).insert_keys(other)
    with pytest.raises(ValueError, match='closed'):
        KT.stand_in_snapshot(4).insert_keys(t)


def test_copy_list_checks():
    s, d, count = check_copy([3, 3, 1], [0, 2, 4], 8, 8, True)
    assert count == 3 and s.dtype == d.dtype == np.int32 and s.tolist() == [3, 3, 1] and d.tolist() == [0, 2, 4]     # sources may repeat
    assert check_copy(None, None, 5, 8, False)[2] == 5                      # without lists: every slot of the source
    assert check_copy(None, [7, 6], 8, 8, True)[2] == 2                     # slots 0, 1 -> 7, 6
    assert check_copy([], [], 8, 8, True)[2] == 0
    with pytest.raises(ValueError, match='twice'):
        check_copy([0, 1], [5, 5], 8, 8, False)                             # a repeat in dst
    with pytest.raises(ValueError, match='also a source'):
        check_copy([0, 1, 2], [5, 1, 6], 8, 8, True)                        # dst and src meet in one buffer ...
    assert check_copy([0, 1, 2], [5, 1, 6], 8, 8, False)[2] == 3            # ... which two buffers allow
    with pytest.raises(ValueError, match='also a source'):
        check_copy(None, None, 4, 4, True)                                  # slots 0 .. 3 onto themselves
    with pytest.raises(ValueError, match='also a source'):
        check_copy(None, [3, 1], 8, 8, True)                                # sources 0, 1
    with pytest.raises(ValueError, match='outside'):
        check_copy([8], [0], 8, 16, False)
    with pytest.raises(ValueError, match='outside'):
        check_copy([0], [-1], 8, 8, False)
    with pytest.raises(ValueError, match='outside'):
        check_copy([0], [4], 8, 4, False)                                   # (the destination's own capacity)
    with pytest.raises(ValueError, match='different lengths'):
        check_copy([0, 1], [2], 8, 8, False)
    with pytest.raises(ValueError, match='pairs for a snapshot of 4 slots'):
        check_copy(None, None, 8, 4, False)
    with pytest.raises(ValueError, match='no list given'):
        check_copy(None, [0, 1, 2], 2, 8, False)
    with pytest.raises(ValueError, match='integer'):
        check_copy([0.5], [1], 8, 8, False)
    # a device tensor's values are not checked here: its length counts
    s, d, count = check_copy('dev', [1, 2], 8, 8, True, lambda x: 2 if isinstance(x, str) else None)
    assert s == 'dev' and d.tolist() == [1, 2] and count == 2
    with pytest.raises(ValueError, match='different lengths'):
        check_copy('dev', [1, 2, 3], 8, 8, True, lambda x: 2 if isinstance(x, str) else None)


def test_a_stand_in_snapshot_checks_a_copy_before_anything_launches():
    import torch
    env = KT.StandInEnv()
    pool, other = KT.stand_in_snapshot(8, env), KT.stand_in_snapshot(4, env)
    with pytest.raises(ValueError, match='twice'):
        pool.copy([0, 1], [2, 2])
    with pytest.raises(ValueError, match='also a source'):
        pool.copy([0, 1], [1, 2])
    with pytest.raises(ValueError, match='outside'):
        pool.copy([4], [0], source=other)                                   # the source has four slots
    with pytest.raises(ValueError, match='outside'):
        other.copy([0], [4], source=pool)
    with pytest.raises(ValueError, match='int32 tensor on cuda:0'):
        pool.copy(torch.zeros(2, dtype=torch.int32), [1, 2])
    with pytest.raises(ValueError, match='another env'):
        pool.copy([0], [1], source=KT.stand_in_snapshot(8))
    with pytest.raises(ValueError, match='Snapshot expected'):
        pool.copy([0], [1], source=3)
    other._invalidate()
    with pytest.raises(ValueError, match='closed'):
        pool.copy([0], [1], source=other)
    with pytest.raises(ValueError, match='closed'):
        other.copy([0], [1])


def test_the_model_against_np_unique_on_one_batch():
    """One call into an empty table: fresh marks exactly np.unique's first occurrences (key 0 left out), which is unique_of_keys' `first`."""
    rs = np.random.RandomState(5)
    keys = rs.randint(0, 40, 300).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)        # about 40 distinct values, 0 among them
    keys[7] = np.uint64((1 << 64) - 1)
    m = KT.KeyTableModel()
    fresh, stored = m.insert(keys)
    _, first = np.unique(keys, return_index=True)
    expect = np.zeros(300, bool)
    expect[first] = True
    expect &= keys != 0
    assert (fresh == expect).all() and (stored == (keys != 0)).all()
    assert len(m) == len(set(keys.tolist()) - {0})
    firsts, _ = unique_of_keys(keys)
    assert sorted(np.nonzero(fresh)[0].tolist()) == sorted(j for j in firsts.tolist() if keys[j] != 0)
    again, _ = m.insert(keys)                                               # the second call: nothing is new
    assert not again.any() and len(m) == int(fresh.sum())
    more = np.concatenate([keys[keys != 0][:5], np.array([12345, 12345, 0], np.uint64)])
    fresh2, stored2 = m.insert(more)
    assert fresh2.tolist() == [False] * 5 + [True, False, False] and stored2.tolist() == [True] * 5 + [True, True, False]
    assert m.contains([12345, 54321, 0]).tolist() == [True, False, False]
    book = KT.WhereBook(8)
    book.check(np.array([5, 6, 5, 0], np.uint64), np.array([3, 1, 3, -1], np.int32), [True, True, True, False], 'book')
    with pytest.raises(AssertionError, match='moved'):
        book.check(np.array([5], np.uint64), np.array([2], np.int32), [True], 'book')
    with pytest.raises(AssertionError, match='holds'):
        book.check(np.array([9], np.uint64), np.array([1], np.int32), [True], 'book')
    with pytest.raises(AssertionError, match='outside'):
        book.check(np.array([10], np.uint64), np.array([8], np.int32), [True], 'book')
    with pytest.raises(AssertionError, match='not stored'):
        book.check(np.array([0], np.uint64), np.array([0], np.int32), [False], 'book')
