"""Path keys and per-pair step limits, host side (no GPU): the limits check, fresh_steps, the result types, the declared symbols, and the
forwarding of path_keys / fields by the adapter, the wrappers, LimitActions' signature and the sharded env on oracle-backed stand-ins
(tests/path_key_oracle.py)."""
import inspect
import os
import re

import numpy as np
import pytest

import ngw_testlib as T
import path_key_oracle as KO
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.playout import Playout, PlayoutPath
from gym_novel_gridworlds_amd.snapshot import Snapshot, check_limits, fresh_pairs, fresh_steps
from gym_novel_gridworlds_amd.state_keys import KEY_ALL, KEY_INV, KEY_POSE, KEY_STATE
from gym_novel_gridworlds_amd.vec_env import PlanEval, RolloutPath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (7 << 32) | 5
NAMES = ('ngw_snapshot_rollout_path', 'ngw_snapshot_playout_path')


def test_header_declares_and_library_exports_the_calls():
    raw = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', text)
    L = _cabi.lib()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), name
        assert hasattr(L, name) and name in _cabi.SYMBOLS and name in doc, name
    assert L.ngw_snapshot_rollout_path(None, None, None, None, 0, 1, None, None, None, 0, None, None, None, None, 15, None, 0) == _cabi.E_INVALID_ARG
    assert 'NULL' in _cabi.last_error()
    assert L.ngw_snapshot_playout_path(None, None, None, 0, 1, 0, 0, None, None, None, None, None, None, None, None, None, None, 0, 15, None, 0) == _cabi.E_INVALID_ARG


def test_limits_are_checked_on_the_host():
    assert check_limits(None, 5, 9) is None
    got = check_limits([0, 9, 3], 3, 9)
    assert got.dtype == np.int32 and got.tolist() == [0, 9, 3] and got.flags.c_contiguous
    assert check_limits(np.array([2, 1], np.int64), 2, 2).tolist() == [2, 1]
    assert check_limits([], 0, 4).size == 0
    for bad, what in (([0, 10], 'outside'), ([-1, 3], 'outside'), ([1.0, 2.0], 'integers'), ([True, False], 'integers'), ([[1, 2]], 'one-dimensional'),
                      ([1, 2, 3], '3 limits for 2 pairs')):
        with pytest.raises(ValueError, match=what):
            check_limits(bad, 2, 9)
    # a device tensor is taken as it is: its values are the kernel's to clamp
    marker = object()
    assert check_limits(marker, 4, 9, lambda x: 4) is marker
    with pytest.raises(ValueError, match='5 limits for 4 pairs'):
        check_limits(marker, 4, 9, lambda x: 5)


def test_fresh_steps_maps_positions_back_to_step_and_pair():
    import torch
    fresh = np.zeros((4, 5), bool)
    fresh[0, 3] = fresh[2, 0] = fresh[3, 4] = True
    t, j = fresh_steps(fresh)
    assert t.tolist() == [0, 2, 3] and j.tolist() == [3, 0, 4]
    tt, tj = fresh_steps(torch.from_numpy(fresh))
    assert isinstance(tt, torch.Tensor) and tt.tolist() == [0, 2, 3] and tj.tolist() == [3, 0, 4]
    t0, j0 = fresh_steps(np.zeros((3, 2), bool))
    assert len(t0) == 0 and len(j0) == 0
    # row-major positions: the flattened keys' order, as fresh_pairs is for [count, A]
    assert [x.tolist() for x in fresh_pairs(fresh)] == [t.tolist(), j.tolist()]


def test_result_types():
    one = np.array([1, 2], np.int32)
    ended, info = np.array([True, True]), np.array([2 | 1, 14 << 8], np.uint32)
    keys = np.arange(6, dtype=np.uint64).reshape(3, 2)
    r = RolloutPath(one, one, ended, info, keys)
    assert r['keys'] is r.keys is r[4] and r._fields == PlanEval._fields + ('keys',)
    assert r.goal.tolist() == [True, False] and r.died.tolist() == [False, True]
    ret, length, e, i, k = r
    p = PlayoutPath(one, one, ended, info, one, None, keys)
    assert p['keys'] is p.keys is p[6] and p._fields == Playout._fields + ('keys',)
    assert p.goal.tolist() == [True, False] and p.died.tolist() == [False, True]
    s = p.shaped(1, 2)
    assert isinstance(s, PlayoutPath) and s.ret.shape == (1, 2) and s.keys.shape == (3, 1, 2) and s.actions is None
    row = s.row(0)
    assert isinstance(row, PlayoutPath) and row.keys.shape == (3, 2) and (row.keys == keys).all() and row.ret.shape == (2,)
    withacts = PlayoutPath(one, one, ended, info, one, np.zeros((3, 2), np.int32), keys).shaped(2, 1)
    assert withacts.actions.shape == (3, 2, 1) and withacts.row(1).actions.shape == (3, 1)


def test_python_surface():
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.envs import PogostickV1Env
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    for fn in (Snapshot.rollout, Snapshot.playout):
        par = inspect.signature(fn).parameters
        assert par['limits'].default is None and par['path_keys'].default is False and par['fields'].default == KEY_STATE, fn
    for owner in (VecNovelGridworld, ShardedVecNovelGridworld, PogostickV1Env, NoveltyWrapper, LimitActions):
        par = inspect.signature(owner.playouts).parameters
        assert par['path_keys'].default is False and 'fields' in par, owner


def _adapter(monkeypatch, cfg='axe10'):
    monkeypatch.setattr(T, 'OracleVec', KO.OracleVecPath)            # (make_adapter_env's oracle backend, with path keys)
    env = T.make_adapter_env(cfg, backend='oracle')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    return env


def test_adapter_and_wrappers_forward_path_keys(monkeypatch):
    env = _adapter(monkeypatch)
    vec = env.unwrapped._backend()
    P, steps = 6, 4
    _, rep, acts, _ = KO.SO.PO.oracle_playout(vec.spec, vec.o.st, np.zeros(P, np.int64), steps, SEED)
    for fields in (KEY_STATE, KEY_POSE | KEY_INV, KEY_ALL):
        exp, _, _, _, _ = KO.oracle_path(vec.spec, vec.o.st, np.zeros(P, np.int64), acts, fields=fields)
        for who in (env, env.unwrapped):
            play = who.playouts(P, steps, SEED, path_keys=True, fields=fields)
            assert isinstance(play, PlayoutPath) and play.keys.shape == (steps, P)
            KO.assert_keys(play.keys, exp, 'adapter fields=%d' % fields)
            assert (play.first_action == rep['first_action']).all() and (play.length == rep['length']).all()
    assert (exp != 0).sum() == rep['length'].sum()                   # a key for every executed step, 0 elsewhere
    plain = env.playouts(P, steps, SEED)
    assert isinstance(plain, Playout) and not isinstance(plain, PlayoutPath) and (plain.ret == rep['ret']).all()
    # weights and path keys together
    x = np.ones(vec.n_actions, np.float32)
    x[0] = 5
    _, _, wacts, _ = KO.SO.oracle_weighted_playout(vec.spec, vec.o.st, np.zeros(P, np.int64), steps, SEED, x)
    wexp, _, _, _, _ = KO.oracle_path(vec.spec, vec.o.st, np.zeros(P, np.int64), wacts)
    KO.assert_keys(env.playouts(P, steps, SEED, weights=x, path_keys=True).keys, wexp, 'adapter, weighted')


def test_sharded_env_returns_what_one_env_returns():
    spec = T.build_spec('pogo10')
    seed = KO.SO.XO.good_seed(spec, 6)
    sh = KO.sharded_on_oracle(spec=spec, global_num_envs=6, seed=seed)
    sh.reset()
    whole = KO.OracleVecPath(spec, 6, seed=seed)
    whole.reset()
    got, exp = sh.playouts(2, 3, SEED, path_keys=True, fields=KEY_ALL), whole.playouts(2, 3, SEED, path_keys=True, fields=KEY_ALL)
    assert got.keys.shape == (3, 6, 2) and (got.keys != 0).any()
    KO.assert_keys(got.keys, exp.keys, 'sharded')
    assert isinstance(sh.playouts(2, 3, SEED), Playout) and not isinstance(sh.playouts(2, 3, SEED), PlayoutPath)
