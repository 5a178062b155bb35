"""The dispatch of rollouts and playouts to their C entry points (playout.pairs_symbol) and the keywords a forwarding playouts() passes on
(playout.forward_keywords): both pure functions, checked exhaustively.  No GPU."""
import itertools

import pytest

from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.playout import forward_keywords, pairs_symbol

SEVEN = {'ngw_snapshot_rollout', 'ngw_snapshot_rollout_path', 'ngw_snapshot_rollout_traj', 'ngw_snapshot_playout', 'ngw_snapshot_playout_weighted',
         'ngw_snapshot_playout_path', 'ngw_snapshot_playout_traj'}


def test_dispatch_table_is_exactly_the_seven_symbols():
    table = {(k, w, p, t): pairs_symbol(k, w, p, t) for k in ('rollout', 'playout') for w, p, t in itertools.product((False, True), repeat=3)}
    assert len(table) == 16 and set(table.values()) == SEVEN and SEVEN <= set(_cabi.SYMBOLS)
    for (kind, weighted, path, traj), name in table.items():
        if traj:                                # any traj is the trajectory form, whatever else is set
            assert name == 'ngw_snapshot_%s_traj' % kind
        elif path:                              # any path without traj is the path form
            assert name == 'ngw_snapshot_%s_path' % kind
        elif kind == 'playout':
            assert name == ('ngw_snapshot_playout_weighted' if weighted else 'ngw_snapshot_playout')
        else:                                   # a rollout draws nothing: `weighted` is ignored
            assert name == 'ngw_snapshot_rollout'
        assert name == pairs_symbol(kind, weighted=weighted, path=path, traj=traj)     # (by keyword too)
    for w, p, t in itertools.product((False, True), repeat=3):
        assert pairs_symbol('rollout', w, p, t) == pairs_symbol('rollout', False, p, t)
    assert pairs_symbol('playout') == 'ngw_snapshot_playout' and pairs_symbol('rollout') == 'ngw_snapshot_rollout'
    with pytest.raises(ValueError):
        pairs_symbol('expand')


def test_forwarded_keywords_are_only_those_that_are_set():
    assert forward_keywords() == {} and forward_keywords(False, 15, False, False, None) == {}      # (fields alone is not forwarded)
    assert forward_keywords(path_keys=True, fields=5) == {'path_keys': True, 'fields': 5}
    assert forward_keywords(path_keys=True) == {'path_keys': True, 'fields': None}
    assert forward_keywords(rewards=True) == {'rewards': True}
    assert forward_keywords(masks=True) == {'masks': True}
    assert forward_keywords(observe='lidar') == {'observe': 'lidar'}
    assert forward_keywords(True, 15, True, True, 'lidar') == {'path_keys': True, 'fields': 15, 'rewards': True, 'masks': True, 'observe': 'lidar'}
