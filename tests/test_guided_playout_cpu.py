"""Guided playouts, host side (no GPU): the exported call, the refusals before a handle is touched, tree_steps, PlayoutGuided's shaped() / row(),
LimitActions' column scatter, the forwarding by every layer down to a 2-rank sharded env, and the forward simulation's event counts for the exact
seeds tests/test_guided_playout.py uses - its coverage conditions."""
import inspect
import os
import re

import numpy as np
import pytest

import guided_playout_oracle as GO
import key_table_oracle as KT
import trajectory_view_oracle as VO
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.playout import OUTSIDE, PlayoutGuided, check_guide, forward_keywords, pairs_symbol, tree_steps
from gym_novel_gridworlds_amd.state_keys import KEY_STATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'ngw_snapshot_playout_guided'
SEED = 11


def test_header_declares_and_library_exports_the_call():
    raw = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    L = _cabi.lib()
    assert re.search(r'\bint\s+%s\s*\(' % NAME, text) and hasattr(L, NAME) and NAME in _cabi.SYMBOLS
    assert NAME in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', raw) and L.ngw_abi_version() == 3
    for word, value in OUTSIDE.items():
        assert int(re.search(r'#define\s+NGW_OUTSIDE_%s\s+(\d+)' % word.upper(), raw).group(1)) == value
    args = [None, None, None, 0, 1, 0, 0, None, None, None, None, None, None, None, None, None, None, 0, 15, None, 0, None, 0, None, 0, None, 0, None,
            None, None, None, 0, None, 0]
    assert len(args) == len(L.ngw_snapshot_playout_guided.argtypes)
    assert L.ngw_snapshot_playout_guided(*args) == _cabi.E_INVALID_ARG and 'NULL' in _cabi.last_error()
    # the dispatch: a table makes the guided call whatever else is set; nothing else moved
    for w, p, t, v in [(False, False, False, False), (True, True, True, True), (True, True, True, False)]:
        assert pairs_symbol('playout', w, p, t, v, True) == NAME and pairs_symbol('playout', w, p, t, v, guided=False) != NAME
    with pytest.raises(ValueError, match='rollout takes plans'):
        pairs_symbol('rollout', guided=True)


def test_refusals_come_before_a_handle_is_touched():
    env, other = KT.StandInEnv(), KT.StandInEnv()
    table, foreign, closed = KT.stand_in_table(8, env), KT.stand_in_table(8, other), KT.stand_in_table(8, env)
    closed._t = None
    snap = KT.stand_in_snapshot(8, env)
    snap.env.lidar = None
    snap._s = None                                                  # (no handle: _open() would raise "snapshot is closed" - every refusal below comes first)
    A = env.n_actions
    good = np.ones((table.buckets, A), np.float32)
    call = lambda **kw: snap.playout([0], 3, SEED, **kw)            # noqa: E731
    with pytest.raises(ValueError, match='another env'):
        call(table=foreign, table_weights=good)
    with pytest.raises(ValueError, match='key table is closed'):
        call(table=closed, table_weights=good)
    with pytest.raises(ValueError, match='table_weights without table'):
        call(table_weights=good)
    with pytest.raises(ValueError, match='table without table_weights'):
        call(table=table)
    with pytest.raises(ValueError, match="outside: 'default' or 'stop'"):
        call(table=table, table_weights=good, outside='leaf')
    with pytest.raises(ValueError, match="outside: 'default' or 'stop'"):
        call(outside=1)
    with pytest.raises(ValueError, match="outside='stop' without table"):
        call(outside='stop')
    with pytest.raises(ValueError, match='fields == 0'):
        call(table=table, table_weights=good, fields=0)
    with pytest.raises(ValueError, match='KeyTable expected'):
        call(table=object(), table_weights=good)
    # accepted keywords get as far as the handle (which this snapshot does not have)
    with pytest.raises(ValueError, match='snapshot is closed'):
        call(table=table, table_weights=good, outside='stop')
    assert check_guide(env, None, None, 'default', KEY_STATE) is None
    assert check_guide(env, table, good, 'stop', None) == (1, KEY_STATE) and check_guide(env, table, good, 'default', 5) == (0, 5)


def test_the_weight_rows_are_checked_for_shape_dtype_and_device():
    import torch
    from gym_novel_gridworlds_amd.playout import check_table_weights
    cpu = torch.device('cpu')
    ok = torch.ones((16, 5), dtype=torch.float32)
    assert check_table_weights(ok, 16, 5, cpu) == (ok, False)                                    # a tensor is used in place
    up, mine = check_table_weights(np.ones((16, 5)), 16, 5, cpu)                                 # a host array is uploaded, as float32
    assert mine and up.dtype == torch.float32 and tuple(up.shape) == (16, 5)
    for bad in (torch.ones((16, 4)), torch.ones((8, 5)), torch.ones((16, 5), dtype=torch.float64), torch.ones((5, 16)).t(), torch.ones(80)):
        with pytest.raises(ValueError, match='contiguous float32 tensor'):
            check_table_weights(bad, 16, 5, cpu)
    with pytest.raises(ValueError, match='on cuda:0 expected'):
        check_table_weights(ok, 16, 5, torch.device('cuda:0'))
    for bad in (np.ones((16, 4)), np.ones(80), np.ones((16, 5), dtype='U1')):
        with pytest.raises(ValueError, match='float32 array'):
            check_table_weights(bad, 16, 5, cpu)


def _result(T=3, count=4):
    where = np.array([[2, -1, 5, -1], [2, 7, -1, -1], [-1, 7, 5, -1]], np.int32)
    actions = np.array([[1, 0, 3, -1], [0, 2, 1, -1], [4, 1, 0, -1]], np.int32)
    length = np.array([3, 3, 3, 0], np.int32)
    depth = np.array([2, 0, 1, 0], np.int32)
    return PlayoutGuided(length, length, length > 0, length.astype(np.uint32), actions[0], actions, None, None, None, None, where, depth)


def test_tree_steps_and_the_result_type():
    import torch
    r = _result()
    b, a, t, j = tree_steps(r)
    assert b.tolist() == [2, 5, 2, 7, 7, 5] and a.tolist() == [1, 3, 0, 2, 1, 0] and t.tolist() == [0, 0, 1, 1, 2, 2] and j.tolist() == [0, 2, 0, 1, 1, 2]
    dev = PlayoutGuided(*[None if x is None else torch.from_numpy(np.asarray(x)) for x in r])
    tb, ta, tt, tj = tree_steps(dev)
    assert isinstance(tb, torch.Tensor) and tb.dtype == torch.int64 and (tb.tolist(), ta.tolist(), tt.tolist(), tj.tolist()) == (b.tolist(), a.tolist(), t.tolist(), j.tolist())
    N = torch.zeros((8, 5))
    N.view(-1).index_add_(0, tb * 5 + ta, torch.ones(len(tb)))                                  # the backup it is for
    assert N.sum() == 6 and N[7, 2] == 1 and N[2, 1] == 1
    with pytest.raises(ValueError, match='record=True'):
        tree_steps(r._replace(actions=None))
    s = r.shaped(2, 2)
    assert s.where.shape == (3, 2, 2) and s.depth.shape == (2, 2) and s['where'] is s.where and isinstance(s, PlayoutGuided)
    assert [x.tolist() for x in tree_steps(s)] == [b.tolist(), a.tolist(), t.tolist(), j.tolist()]   # (j indexes the flattened pair axes)
    row = s.row(1)
    assert (row.where == r.where[:, 2:]).all() and (row.depth == r.depth[2:]).all() and (row.actions == r.actions[:, 2:]).all()
    from gym_novel_gridworlds_amd.snapshot import transitions
    tt, tj = transitions(r)                                                                      # keeps working: T off the recorded actions
    assert tt.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and tj.tolist() == [0, 1, 2] * 3


def test_python_surface_and_forwarding():
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.envs import PogostickV1Env
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    from gym_novel_gridworlds_amd.snapshot import Snapshot
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    for fn in (Snapshot.playout, VecNovelGridworld.playouts, ShardedVecNovelGridworld.playouts, PogostickV1Env.playouts, NoveltyWrapper.playouts, LimitActions.playouts):
        par = inspect.signature(fn).parameters
        assert par['table'].default is None and par['table_weights'].default is None and par['outside'].default == 'default', fn
    assert 'table' not in inspect.signature(Snapshot.rollout).parameters                         # (a rollout takes plans)
    assert forward_keywords() == {} and forward_keywords(path_keys=True, fields=5) == {'path_keys': True, 'fields': 5}
    t, w = object(), object()
    assert forward_keywords(table=t, table_weights=w, fields=7) == {'table': t, 'fields': 7, 'table_weights': w, 'outside': 'default'}
    assert forward_keywords(table=t, table_weights=w, outside='stop', path_keys=True)['outside'] == 'stop'
    assert forward_keywords(outside='stop') == {'outside': 'stop'} and forward_keywords(table_weights=w) == {'table_weights': w}   # (travel on: the env refuses them)


def test_every_layer_passes_the_keywords_through(monkeypatch):
    """The adapter, a wrapper chain and a 2-rank sharded env hand table / table_weights / outside to the batched env's playouts unchanged."""
    import ngw_testlib as T
    import torch.distributed as dist
    seen = []

    def spy(self, n_playouts, steps, seed, device=False, weights=None, **kw):
        seen.append(kw)
        return _result().shaped(1, 4)
    monkeypatch.setattr(VO.OracleVecViews, 'playouts', spy)
    monkeypatch.setattr(T, 'OracleVec', VO.OracleVecViews)
    env = T.make_adapter_env('axe10', backend='oracle')
    env.reset()
    t, w = object(), object()
    assert env is not env.unwrapped
    for who in (env, env.unwrapped):
        got = who.playouts(4, 3, SEED, table=t, table_weights=w, outside='stop')
        assert isinstance(got, PlayoutGuided) and got.where.shape == (3, 4) and got.depth.shape == (4,)
        assert seen[-1]['table'] is t and seen[-1]['table_weights'] is w and seen[-1]['outside'] == 'stop' and seen[-1]['fields'] == KEY_STATE
        who.playouts(4, 3, SEED)
        assert seen[-1] == {}                                       # without the keywords the call is the call it always was
    spec = T.build_spec('pogo10')
    for rank in (0, 1):
        monkeypatch.setattr(dist, 'is_initialized', lambda: True)
        monkeypatch.setattr(dist, 'get_rank', lambda group=None, r=rank: r)
        monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
        sh = VO.sharded_on_oracle(spec=spec, global_num_envs=6, seed=3)
        sh.playouts(2, 3, SEED, table=t, table_weights=w)
        assert seen[-1]['table'] is t and seen[-1]['table_weights'] is w and seen[-1]['outside'] == 'default'


def test_limit_actions_scatters_the_columns_once(monkeypatch):
    """LimitActions.playouts: table_weights' columns are in the wrapper's id space; the limited env gets them in its own (sorted-name) order."""
    import ngw_testlib as T
    from gym_novel_gridworlds_amd import wrappers
    from gym_novel_gridworlds_amd.wrappers import LimitActions, limit_weight_columns
    seen = []

    def spy(self, n_playouts, steps, seed, device=False, weights=None, **kw):
        seen.append(kw)
        return _result()._replace(first_action=np.array([1, 0, 2, 0], np.int32)).shaped(1, 4)      # (the kernel's ids: below the three limited actions)

    def stand_in(vec, names):
        new = VO.OracleVecViews(wrappers.limited_spec(vec.spec, names), vec.num_envs, seed=vec.o.seed)
        new.reset()
        return new
    monkeypatch.setattr(wrappers, 'limit_actions_vec', stand_in)
    monkeypatch.setattr(T, 'OracleVec', VO.OracleVecViews)
    env = T.make_adapter_env('axe10', backend='oracle')
    env.reset()
    lim = LimitActions(env, {'Break', 'Forward', 'Left'})
    lim.set_limited_actions_id({'Break': 2, 'Forward': 0, 'Left': 1})          # sorted names: Break, Forward, Left -> the kernel's column i is the wrapper's ids[i]
    monkeypatch.setattr(VO.OracleVecViews, 'playouts', spy)
    tw = np.arange(8 * 3, dtype=np.float32).reshape(8, 3)
    t = object()
    play = lim.playouts(4, 3, SEED, table=t, table_weights=tw)
    sent = seen[-1]['table_weights']
    assert sent.shape == (8, 3) and (sent == tw[:, [2, 0, 1]]).all() and seen[-1]['table'] is t
    assert play.first_action.tolist() == [0, 2, 1, 2] and (play.where == _result().where).all()   # (ids of the wrapper's own; buckets know no id space)
    import torch
    dev_rows = limit_weight_columns(torch.from_numpy(tw), [2, 0, 1])
    assert dev_rows.is_contiguous() and (dev_rows.numpy() == tw[:, [2, 0, 1]]).all()
    with pytest.raises(ValueError, match='one column per limited action'):
        limit_weight_columns(np.ones((8, 4)), [2, 0, 1])
    lim.set_limited_actions_id({'Break': 0, 'Forward': 1, 'Left': 2})          # the kernel's own order: the rows travel as they are
    lim.playouts(4, 3, SEED, table=t, table_weights=tw)
    assert seen[-1]['table_weights'] is tw


@pytest.mark.parametrize('name', list(GO.CONFIGS))
def test_the_gpu_tests_seeds_meet_the_coverage_conditions(name):
    e = GO.expected(name)
    ev = GO.coverage(e)
    assert ev['executed'] == int(e['reports']['length'].sum()) and ev['hits'] + ev['misses'] == ev['executed']
    spec = GO.twin(name)[0]
    _, _, members = GO.inputs(name)
    A, craft = len(spec.actions_id), GO.craft_ids(spec)
    kinds = {(int(k) >> 3) % 5 for k in members.tolist()}
    assert kinds == {0, 1, 2, 3, 4} and len(set(members.tolist())) == len(members) and 0 not in members.tolist()
    rows = np.stack([GO.row_of(k, A, craft) for k in members.tolist()])
    assert (rows.sum(1) == 0).any() and ((rows > 0).sum(1) == 1).any()                          # all-zero rows and peaked rows
    # a load near one half: probe chains occur whatever buckets the device picks (more keys than a quarter of the buckets share home buckets)
    from gym_novel_gridworlds_amd.key_table import buckets_for
    buckets = buckets_for(len(members))
    home = GO.home_buckets(members, buckets)
    assert len(members) > buckets // 4 and len(np.unique(home)) < len(members), "two members share a home bucket: one of them sits outside it"
    s = GO.expected(name, stop=True)
    length = s['reports']['length']
    assert ((~s['reports']['ended']) & (length < GO.STEPS)).any() and (s['depth'] == length).all() and s['events']['misses'] == 0
    if name == 'axe11':
        assert spec.map_size ** 2 % 4 and e['events']['pickups'] > 0 and A == 18
    if name == 'fire12h':
        assert e['events']['deaths'] > 0 and e['events']['cuts'] > 0
