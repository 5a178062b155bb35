"""Trajectories that observe AgentMap views, host side (no GPU): the two exported calls, check_observe's old and new answers, refusals before a handle
is touched, dict-valued `obs` in transitions() / shaped() / row(), and the forwarding of observe='agent_view', view_size= by the adapter, the
wrappers, LimitActions and a 2-rank sharded env on oracle-backed stand-ins (tests/trajectory_view_oracle.py)."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import ngw_testlib as T
import path_key_oracle as KO
import trajectory_oracle as TO
import trajectory_view_oracle as VO
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.playout import Playout, PlayoutTraj, forward_keywords, pairs_symbol
from gym_novel_gridworlds_amd.snapshot import VIEW_SIZE_MAX, Snapshot, check_observe, transitions
from gym_novel_gridworlds_amd.vec_env import RolloutTraj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (7 << 32) | 5
NAMES = ('ngw_snapshot_rollout_traj_views', 'ngw_snapshot_playout_traj_views')


def test_header_declares_and_library_exports_the_calls():
    raw = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    L = _cabi.lib()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), name
        assert hasattr(L, name) and name in _cabi.SYMBOLS and name in doc, name
    assert re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', raw) and L.ngw_abi_version() == 3
    assert int(re.search(r'#define\s+NGW_TRAJ_VIEW_MAX\s+(\d+)', raw).group(1)) == VIEW_SIZE_MAX >= 8
    assert re.search(r'typedef\s+struct\s+ngw_traj_views\s*\{\s*int32_t\s+view_size;\s*int8_t\s*\*\s*view_dev;\s*int32_t\s*\*\s*facing_dev;\s*int32_t\s*\*\s*inv_dev;'
                     r'\s*int64_t\s+stride;\s*\}', text)
    vw = _cabi.TrajViews(5, None, None, None, 64)
    for views in (None, vw):                                        # a NULL handle, with and without the struct
        assert L.ngw_snapshot_rollout_traj_views(None, None, None, None, 0, 1, None, None, None, 0, None, None, None, None, 15, None, 0, None, 0, None, 0,
                                                 views) == _cabi.E_INVALID_ARG
        assert 'NULL' in _cabi.last_error()
        assert L.ngw_snapshot_playout_traj_views(None, None, None, 0, 1, 0, 0, None, None, None, None, None, None, None, None, None, None, 0, 15, None, 0, None, 0,
                                                 None, 0, None, 0, views) == _cabi.E_INVALID_ARG
        assert 'NULL' in _cabi.last_error()
    # the dispatch: views are the trajectory form's own entry points, everything else goes where it went
    assert pairs_symbol('rollout', False, True, True, True) == NAMES[0] and pairs_symbol('playout', True, True, True, views=True) == NAMES[1]
    assert pairs_symbol('playout', True, True, True) == 'ngw_snapshot_playout_traj' and pairs_symbol('rollout', False, True, True, False) == 'ngw_snapshot_rollout_traj'


def test_check_observe_keeps_its_answers_and_takes_agent_view():
    no_lidar, with_lidar = types.SimpleNamespace(lidar=None), types.SimpleNamespace(lidar=object())
    assert check_observe(no_lidar, None) is False and check_observe(with_lidar, None) is False and check_observe(with_lidar, 'lidar') is True
    assert check_observe(with_lidar, None, 5) is False and check_observe(with_lidar, 'lidar', 5) is True
    with pytest.raises(ValueError, match='lidar_configure'):
        check_observe(no_lidar, 'lidar')
    for bad in ('agent_map', 'rgb', True, 'Lidar', 1, 'AGENT_VIEW', ('lidar', 'agent_view')):
        for env in (no_lidar, with_lidar):
            with pytest.raises(ValueError, match="None or 'lidar'"):
                check_observe(env, bad)
    for env in (no_lidar, with_lidar):                              # no lidar needed
        for V in (1, 5, 8, VIEW_SIZE_MAX, np.int64(3)):
            assert check_observe(env, 'agent_view', V)
        assert check_observe(env, 'agent_view')
        for V in (0, -1, VIEW_SIZE_MAX + 1, 2.0, '5', None, True):
            with pytest.raises(ValueError, match=r'view_size.*1\.\.%d' % VIEW_SIZE_MAX):
                check_observe(env, 'agent_view', V)
        # view_size belongs to 'agent_view': at its default it is ignored, anything else is refused
        for V in (3, 0, 6.0, None):
            with pytest.raises(ValueError, match='view_size'):
                check_observe(env, None, V)
    with pytest.raises(ValueError, match='view_size'):
        check_observe(with_lidar, 'lidar', 3)


def test_refusals_come_before_a_handle_is_touched():
    no_lidar = types.SimpleNamespace(lidar=None)
    snap = Snapshot.__new__(Snapshot)                               # (no handle: every refusal below comes before the first use of one)
    snap.env = no_lidar
    for V in (0, VIEW_SIZE_MAX + 1, 2.5, True):
        with pytest.raises(ValueError, match='view_size'):
            snap.rollout([0], [[0]], observe='agent_view', view_size=V)
        with pytest.raises(ValueError, match='view_size'):
            snap.playout([0], 3, SEED, observe='agent_view', view_size=V)
    with pytest.raises(ValueError, match='view_size'):
        snap.playout([0], 3, SEED, view_size=3)
    with pytest.raises(ValueError, match='view_size'):
        snap.rollout([0], [[0]], rewards=True, view_size=7)
    with pytest.raises(ValueError, match="None or 'lidar'"):
        snap.playout([0], 3, SEED, observe='agent_map', view_size=3)
    with pytest.raises(ValueError, match='masks=True'):
        snap.rollout([0], [[0]], masks=True, observe='agent_view')
    # accepted keywords get as far as the handle (which this snapshot does not have)
    with pytest.raises(AttributeError):
        snap.playout([0], 3, SEED, observe='agent_view', view_size=VIEW_SIZE_MAX)
    with pytest.raises(AttributeError):
        snap.rollout([0], [[0]], observe='agent_view')


def test_python_surface():
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.envs import PogostickV1Env
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    for fn in (Snapshot.rollout, Snapshot.playout, VecNovelGridworld.playouts, ShardedVecNovelGridworld.playouts, PogostickV1Env.playouts, NoveltyWrapper.playouts,
               LimitActions.playouts):
        par = inspect.signature(fn).parameters
        assert par['view_size'].default == 5 and par['observe'].default is None, fn
    assert forward_keywords() == {} and forward_keywords(observe='lidar') == {'observe': 'lidar'} and forward_keywords(observe='lidar', view_size=5) == {'observe': 'lidar'}
    assert forward_keywords(observe='agent_view') == {'observe': 'agent_view', 'view_size': 5}
    assert forward_keywords(rewards=True, observe='agent_view', view_size=2) == {'rewards': True, 'observe': 'agent_view', 'view_size': 2}
    assert forward_keywords(view_size=3) == {'view_size': 3}        # (travels on, so that the env refuses it)


def _dict_obs(steps, count, V=1, K=3):
    W = 2 * V + 1
    return {'agent_map': np.arange((steps + 1) * count * W * W, dtype=np.int64).astype(np.int8).reshape(steps + 1, count, W, W),
            'agent_facing_id': np.arange((steps + 1) * count, dtype=np.int32).reshape(steps + 1, count),
            'inventory_items_quantity': np.arange((steps + 1) * count * K, dtype=np.int32).reshape(steps + 1, count, K)}


def test_transitions_and_shaped_take_a_dict():
    import torch
    length = np.array([2, 0, 3, 1], np.int32)
    obs = _dict_obs(3, 4)
    only = RolloutTraj(length, length, length > 0, length.astype(np.uint32), None, None, obs)
    t, j = transitions(only)
    assert t.tolist() == [0, 0, 0, 1, 1, 2] and j.tolist() == [0, 2, 3, 0, 2, 2]
    dev = PlayoutTraj(*[torch.from_numpy(np.asarray(x)) for x in only[:4]], torch.from_numpy(length), None, None, None, None,
                      {k: torch.from_numpy(x) for k, x in obs.items()})
    tt, tj = transitions(dev)
    assert isinstance(tt, torch.Tensor) and tt.tolist() == t.tolist() and tj.tolist() == j.tolist()
    p = PlayoutTraj(length, length, length > 0, length.astype(np.uint32), length, None, None, np.zeros((3, 4), np.int32), None, obs)
    s = p.shaped(2, 2)
    assert isinstance(s.obs, dict) and sorted(s.obs) == sorted(obs)
    assert s.obs['agent_map'].shape == (4, 2, 2, 3, 3) and s.obs['agent_facing_id'].shape == (4, 2, 2) and s.obs['inventory_items_quantity'].shape == (4, 2, 2, 3)
    for k in obs:
        assert (s.obs[k].reshape(obs[k].shape) == obs[k]).all()
    r = s.row(1)
    assert r.obs['agent_map'].shape == (4, 2, 3, 3) and (r.obs['agent_map'] == obs['agent_map'][:, 2:]).all() and (r.obs['agent_facing_id'] == obs['agent_facing_id'][:, 2:]).all()
    assert (r.obs['inventory_items_quantity'] == obs['inventory_items_quantity'][:, 2:]).all() and r.rewards.shape == (3, 2)
    sd = dev.shaped(4, 1)
    assert sd.obs['agent_map'].shape == (4, 4, 1, 3, 3) and isinstance(sd.obs['agent_facing_id'], torch.Tensor)


def _adapter(monkeypatch, cfg='axe10'):
    monkeypatch.setattr(T, 'OracleVec', VO.OracleVecViews)          # (make_adapter_env's oracle backend, with trajectories and views)
    env = T.make_adapter_env(cfg, backend='oracle')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    return env


def test_adapter_and_wrappers_forward_the_keywords(monkeypatch):
    env = _adapter(monkeypatch)
    vec = env.unwrapped._backend()
    assert vec.lidar is None                                        # no lidar anywhere in this test
    P, steps = 6, 4
    _, rep, acts, _ = KO.SO.PO.oracle_playout(vec.spec, vec.o.st, np.zeros(P, np.int64), steps, SEED)
    e = TO.oracle_traj(vec.spec, vec.o.st, np.zeros(P, np.int64), acts)
    K = len(vec.spec.items_id)
    assert env is not env.unwrapped                                 # (a wrapper chain sits on the adapter)
    for V in (5, 2):
        exp = VO.expect_views(vec.spec, vec.o.st, np.zeros(P, np.int64), e, V)
        W = 2 * V + 1
        for who in (env, env.unwrapped):
            play = who.playouts(P, steps, SEED, rewards=True, masks=True, observe='agent_view', view_size=V)
            assert isinstance(play, PlayoutTraj) and play.keys is None and play.actions is None
            assert play.obs['agent_map'].shape == (steps + 1, P, W, W) and play.obs['agent_facing_id'].shape == (steps + 1, P)
            assert play.obs['inventory_items_quantity'].shape == (steps + 1, P, K)
            VO.assert_views(play.obs, exp, '%s V=%d' % (type(who).__name__, V))
            TO.assert_traj(play, e, type(who).__name__, ('rewards', 'masks'))
            behind = np.arange(steps)[:, None] >= play.length[None, :]
            assert all((play.obs[k][1:][behind] == 0).all() for k in play.obs) and (play.ret == rep['ret']).all()
    assert VO.windows_move(exp, rep['length']) > 0
    # the default window; the keyword alone allocates nothing else; without it the call is the call it always was
    default = env.playouts(P, steps, SEED, observe='agent_view')
    VO.assert_views(default.obs, VO.expect_views(vec.spec, vec.o.st, np.zeros(P, np.int64), e, 5), 'default view_size')
    assert default.rewards is None and default.masks is None and default.keys is None
    keyed = env.playouts(P, steps, SEED, observe='agent_view', path_keys=True)
    KO.assert_keys(keyed.keys, e['keys'], 'views with path keys')
    assert type(env.playouts(P, steps, SEED)) is Playout
    # refusals travel through the forwarding
    with pytest.raises(ValueError, match='view_size'):
        env.playouts(P, steps, SEED, observe='agent_view', view_size=0)
    with pytest.raises(ValueError, match='view_size'):
        env.playouts(P, steps, SEED, view_size=3)
    with pytest.raises(ValueError, match="None or 'lidar'"):
        env.playouts(P, steps, SEED, observe='agent_map', view_size=3)


def test_limit_actions_changes_nothing_in_the_views(monkeypatch):
    """LimitActions.playouts on the stand-in: the limited env is the oracle on the limited spec (what limit_actions_vec builds on the device); the
    views are those of the limited playouts' states, with ids of the wrapper's own and with or without a lidar on the backend."""
    from gym_novel_gridworlds_amd import wrappers
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    made = []

    def stand_in(vec, names):
        new = VO.OracleVecViews(wrappers.limited_spec(vec.spec, names), vec.num_envs, seed=vec.o.seed)
        new.reset()
        made.append(new)
        return new
    monkeypatch.setattr(wrappers, 'limit_actions_vec', stand_in)
    env = _adapter(monkeypatch)
    vec = env.unwrapped._backend()
    lim = LimitActions(env, {'Break', 'Forward', 'Left'})
    lim.set_limited_actions_id({'Break': 5, 'Forward': 0, 'Left': 3})
    P, steps, V = 6, 4, 3
    play = lim.playouts(P, steps, SEED, rewards=True, observe='agent_view', view_size=V)
    limited = made[0]
    _, rep, acts, _ = KO.SO.PO.oracle_playout(limited.spec, vec.o.st, np.zeros(P, np.int64), steps, SEED)
    e = TO.oracle_traj(limited.spec, vec.o.st, np.zeros(P, np.int64), acts)
    VO.assert_views(play.obs, VO.expect_views(limited.spec, vec.o.st, np.zeros(P, np.int64), e, V), 'LimitActions')
    assert (play.rewards == e['rewards']).all() and limited.configured == 0 and limited.lidar is None
    vec.lidar_configure(num_beams=8, dtype=np.int32)                # a lidar on the backend is none of the views' business
    again = lim.playouts(P, steps, SEED, rewards=True, observe='agent_view', view_size=V)
    assert limited.configured == 0 and all((again.obs[k] == play.obs[k]).all() for k in play.obs)
    lim.close()


def test_two_sharded_ranks_return_what_one_env_returns(monkeypatch):
    import torch.distributed as dist
    spec = T.build_spec('pogo10')
    G, P, steps, V = 6, 2, 3, 2
    seed = KO.SO.XO.good_seed(spec, G)
    whole = VO.OracleVecViews(spec, G, seed=seed)
    whole.reset()
    exp = whole.playouts(P, steps, SEED, rewards=True, masks=True, observe='agent_view', view_size=V)
    assert exp.obs['agent_map'].shape == (steps + 1, G, P, 2 * V + 1, 2 * V + 1) and (exp.obs['agent_map'] != 0).any()
    parts = []
    for rank in (0, 1):
        monkeypatch.setattr(dist, 'is_initialized', lambda: True)
        monkeypatch.setattr(dist, 'get_rank', lambda group=None, r=rank: r)
        monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
        sh = VO.sharded_on_oracle(spec=spec, global_num_envs=G, seed=seed)
        assert sh.world == 2 and sh.rank == rank and sh.num_envs == G // 2 and sh.local.env_index_base == sh.first
        sh.reset()
        parts.append(sh.playouts(P, steps, SEED, rewards=True, masks=True, observe='agent_view', view_size=V))
        with pytest.raises(ValueError, match='view_size'):
            sh.playouts(P, steps, SEED, view_size=V)
    monkeypatch.undo()
    for name in ('rewards', 'masks'):
        assert (np.concatenate([p[name] for p in parts], 1) == exp[name]).all(), name
    for name in ('ret', 'length', 'first_action'):
        assert (np.concatenate([p[name] for p in parts], 0) == exp[name]).all(), name
    for k in VO.FIELDS:                                             # the env axis is axis 1 of every value, as it is of the lidar rows
        assert (np.concatenate([p.obs[k] for p in parts], 1) == exp.obs[k]).all(), k
