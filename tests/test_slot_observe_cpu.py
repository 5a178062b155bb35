"""The host side of the slot observations (snapshot.py check_slots; the three C-ABI symbols): no GPU."""
import os
import re

import numpy as np
import pytest

from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.snapshot import check_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ngw_snapshot_lidar', 'ngw_snapshot_agent_view', 'ngw_snapshot_action_mask')


def test_none_means_every_slot():
    assert check_slots(None, 37) == (None, 37)


def test_lists_and_arrays_may_repeat_and_exceed_the_capacity():
    s, count = check_slots([3, 3, 0, 4, 3, 1, 1], 5)
    assert count == 7 and s.dtype == np.int32 and s.flags['C_CONTIGUOUS'] and s.tolist() == [3, 3, 0, 4, 3, 1, 1]
    s, count = check_slots(np.array([2, 0], np.int64), 3)
    assert count == 2 and s.dtype == np.int32 and s.tolist() == [2, 0]


def test_an_empty_list_is_count_zero():
    s, count = check_slots([], 5)
    assert count == 0 and s.dtype == np.int32 and s.shape == (0,)


@pytest.mark.parametrize('bad', [np.array([0.0, 1.0]), [[0, 1], [1, 0]], [0, -1, 2], [0, 5]],
                         ids=['float dtype', 'two dimensions', 'negative', 'capacity as an index'])
def test_bad_lists_raise(bad):
    with pytest.raises(ValueError, match='slots'):
        check_slots(bad, 5)


def test_a_device_length_passes_through_unchecked():
    token = object()                                            # (stands for a device tensor: its values are never looked at)
    assert check_slots(token, 5, device_len=lambda x: 1000 if x is token else None) == (token, 1000)
    s, count = check_slots([1, 2], 5, device_len=lambda x: None)
    assert count == 2 and s.tolist() == [1, 2]
    with pytest.raises(ValueError):
        check_slots([7], 5, device_len=lambda x: None)


def test_the_header_declares_the_three_symbols_and_the_ctypes_table_lists_them():
    text = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    L = _cabi.lib()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), name
        assert name in _cabi.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes, name
