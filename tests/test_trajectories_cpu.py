"""Trajectories, host side (no GPU): keyword validation and refusals, the result types, transitions(), the declared symbols, and the
forwarding of rewards / masks / observe by the adapter, the wrappers, LimitActions' id space and the sharded env on oracle-backed stand-ins
(tests/trajectory_oracle.py)."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import ngw_testlib as T
import path_key_oracle as KO
import trajectory_oracle as TO
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.playout import Playout, PlayoutPath, PlayoutTraj, choose_actions
from gym_novel_gridworlds_amd.sample import choose_weighted
from gym_novel_gridworlds_amd.playout import playout_words
from gym_novel_gridworlds_amd.snapshot import Snapshot, check_observe, transitions
from gym_novel_gridworlds_amd.vec_env import RolloutPath, RolloutTraj
from gym_novel_gridworlds_amd.wrappers import limit_mask_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (7 << 32) | 5
NAMES = ('ngw_snapshot_rollout_traj', 'ngw_snapshot_playout_traj')


def test_header_declares_and_library_exports_the_calls():
    raw = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    L = _cabi.lib()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), name
        assert hasattr(L, name) and name in _cabi.SYMBOLS and name in doc, name
    assert L.ngw_snapshot_rollout_traj(None, None, None, None, 0, 1, None, None, None, 0, None, None, None, None, 15, None, 0, None, 0, None, 0) == _cabi.E_INVALID_ARG
    assert 'NULL' in _cabi.last_error()
    assert L.ngw_snapshot_playout_traj(None, None, None, 0, 1, 0, 0, None, None, None, None, None, None, None, None, None, None, 0, 15, None, 0, None, 0, None, 0,
                                       None, 0) == _cabi.E_INVALID_ARG


def test_keywords_are_validated_before_anything_runs():
    no_lidar, with_lidar = types.SimpleNamespace(lidar=None), types.SimpleNamespace(lidar=object())
    assert check_observe(no_lidar, None) is False and check_observe(with_lidar, 'lidar') is True
    with pytest.raises(ValueError, match='lidar_configure'):
        check_observe(no_lidar, 'lidar')
    for bad in ('agent_map', True, 'Lidar', 1):
        with pytest.raises(ValueError, match="None or 'lidar'"):
            check_observe(with_lidar, bad)
    snap = Snapshot.__new__(Snapshot)                               # (no handle: every refusal below comes before the first use of one)
    snap.env = no_lidar
    with pytest.raises(ValueError, match='masks=True'):
        snap.rollout([0], [[0]], masks=True)
    with pytest.raises(ValueError, match='lidar_configure'):
        snap.rollout([0], [[0]], observe='lidar')
    with pytest.raises(ValueError, match='lidar_configure'):
        snap.playout([0], 3, SEED, observe='lidar')
    snap.env = with_lidar
    with pytest.raises(ValueError, match="None or 'lidar'"):
        snap.playout([0], 3, SEED, observe='agent_map')
    with pytest.raises(ValueError, match="None or 'lidar'"):
        snap.rollout([0], [[0]], observe='agent_map')


def test_python_surface():
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.envs import PogostickV1Env
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    for fn in (Snapshot.rollout, Snapshot.playout, VecNovelGridworld.playouts, ShardedVecNovelGridworld.playouts, PogostickV1Env.playouts, NoveltyWrapper.playouts,
               LimitActions.playouts):
        par = inspect.signature(fn).parameters
        assert par['rewards'].default is False and par['masks'].default is False and par['observe'].default is None, fn


def test_result_types():
    one = np.array([1, 2], np.int32)
    ended, info = np.array([True, True]), np.array([2 | 1, 14 << 8], np.uint32)
    keys = np.arange(6, dtype=np.uint64).reshape(3, 2)
    rew, obs = np.arange(6, dtype=np.int32).reshape(3, 2), np.arange(4 * 2 * 5, dtype=np.int16).reshape(4, 2, 5)
    r = RolloutTraj(one, one, ended, info, None, rew, obs)
    assert r['rewards'] is r.rewards is r[5] and r.keys is None and r._fields == RolloutPath._fields + ('rewards', 'obs')
    assert r.goal.tolist() == [True, False] and r.died.tolist() == [False, True]
    p = PlayoutTraj(one, one, ended, info, one, None, keys, rew, None, obs)
    assert p['obs'] is p.obs is p[9] and p.masks is None and p._fields == PlayoutPath._fields + ('rewards', 'masks', 'obs')
    assert p.goal.tolist() == [True, False] and p.died.tolist() == [False, True]
    s = p.shaped(1, 2)
    assert isinstance(s, PlayoutTraj) and s.ret.shape == (1, 2) and s.keys.shape == (3, 1, 2) and s.rewards.shape == (3, 1, 2) and s.obs.shape == (4, 1, 2, 5)
    assert s.actions is None and s.masks is None
    row = s.row(0)
    assert isinstance(row, PlayoutTraj) and row.rewards.shape == (3, 2) and (row.rewards == rew).all() and row.obs.shape == (4, 2, 5) and (row.obs == obs).all()
    # the packed format's pair travels through both
    pair = (np.zeros((4, 2, 3), np.uint8), np.ones((4, 2, 2), np.int16))
    q = PlayoutTraj(one, one, ended, info, one, None, None, None, None, pair).shaped(2, 1)
    assert isinstance(q.obs, tuple) and q.obs[0].shape == (4, 2, 1, 3) and q.obs[1].shape == (4, 2, 1, 2) and q.row(1).obs[1].shape == (4, 1, 2)


def test_transitions_lists_the_executed_steps_row_major():
    import torch
    length = np.array([2, 0, 3, 1], np.int32)
    res = RolloutTraj(length, length, length > 0, length.astype(np.uint32), None, np.zeros((3, 4), np.int32), None)
    t, j = transitions(res)
    assert t.tolist() == [0, 0, 0, 1, 1, 2] and j.tolist() == [0, 2, 3, 0, 2, 2]
    dev = RolloutTraj(*[torch.from_numpy(np.asarray(x)) for x in res[:4]], None, torch.zeros((3, 4), dtype=torch.int32), None)
    tt, tj = transitions(dev)
    assert isinstance(tt, torch.Tensor) and tt.tolist() == t.tolist() and tj.tolist() == j.tolist()
    # T from the rows alone ([T + 1, count, row]); from the packed pair; no per-step field at all
    only_obs = RolloutTraj(length, length, length > 0, length.astype(np.uint32), None, None, np.zeros((4, 4, 2), np.int16))
    assert [x.tolist() for x in transitions(only_obs)] == [t.tolist(), j.tolist()]
    packed = PlayoutTraj(length, length, length > 0, length.astype(np.uint32), length, None, None, None, None, (np.zeros((4, 4, 2), np.uint8), np.zeros((4, 4, 1), np.int16)))
    assert [x.tolist() for x in transitions(packed)] == [t.tolist(), j.tolist()]
    with pytest.raises(ValueError, match='no per-step field'):
        transitions(Playout(length, length, length > 0, length.astype(np.uint32), length, None))
    t0, j0 = transitions(RolloutTraj(length * 0, length * 0, length > 9, length.astype(np.uint32), None, np.zeros((3, 4), np.int32), None))
    assert len(t0) == 0 and len(j0) == 0


def test_limit_mask_words_moves_bits_into_the_wrappers_id_space():
    import torch
    ids = [4, 0, 9]
    w = np.array([0b000, 0b001, 0b010, 0b100, 0b111, 0b101], np.uint64)
    exp = [0, 1 << 4, 1 << 0, 1 << 9, (1 << 4) | 1 | (1 << 9), (1 << 4) | (1 << 9)]
    got = limit_mask_words(w, ids)
    assert got.dtype == np.uint64 and got.tolist() == exp
    assert limit_mask_words(torch.from_numpy(w.view(np.int64)), ids).tolist() == exp


def _adapter(monkeypatch, cfg='axe10'):
    monkeypatch.setattr(T, 'OracleVec', TO.OracleVecTraj)            # (make_adapter_env's oracle backend, with trajectories)
    env = T.make_adapter_env(cfg, backend='oracle')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    return env


def test_adapter_and_wrappers_forward_the_keywords(monkeypatch):
    env = _adapter(monkeypatch)
    vec = env.unwrapped._backend()
    vec.lidar_configure()
    P, steps, A = 6, 4, vec.n_actions
    pairs = np.arange(P, dtype=np.uint64)
    _, rep, acts, _ = KO.SO.PO.oracle_playout(vec.spec, vec.o.st, np.zeros(P, np.int64), steps, SEED)
    exp = TO.oracle_traj(vec.spec, vec.o.st, np.zeros(P, np.int64), acts, lc=vec.lidar)
    for who in (env, env.unwrapped):
        play = who.playouts(P, steps, SEED, rewards=True, masks=True, observe='lidar')
        assert isinstance(play, PlayoutTraj) and play.keys is None and play.actions is None
        assert play.rewards.shape == (steps, P) and play.masks.shape == (steps, P) and play.obs.shape == (steps + 1, P, exp['obs'].shape[-1])
        TO.assert_traj(play, exp, type(who).__name__)
        assert (play.rewards.sum(0) == play.ret).all() and (play.ret == rep['ret']).all()
        assert (play.obs[0] == play.obs[0][0]).all() and (play.obs[1:][np.arange(steps)[:, None] >= play.length[None, :]] == 0).all()
    # the recorded words reproduce the recorded actions
    for t in range(steps):
        ran = play.length > t
        assert (choose_actions(play.masks[t][ran], SEED, pairs[ran], t, A) == acts[t][ran]).all() and (play.masks[t][~ran] == 0).all()
    # one keyword alone allocates nothing else; none is the call it always was
    only = env.playouts(P, steps, SEED, rewards=True)
    assert isinstance(only, PlayoutTraj) and only.masks is None and only.obs is None and (only.rewards == exp['rewards']).all()
    both = env.playouts(P, steps, SEED, masks=True, path_keys=True)
    KO.assert_keys(both.keys, exp['keys'], 'masks with path keys')
    assert both.rewards is None and (both.masks == exp['masks']).all()
    plain = env.playouts(P, steps, SEED)
    assert type(plain) is Playout and (plain.ret == rep['ret']).all()
    assert type(env.playouts(P, steps, SEED, path_keys=True)) is PlayoutPath
    # weights and the mask words together: the weighted rule on the recorded word is the recorded action
    x = np.ones(A, np.float32)
    x[0] = 5
    _, _, wacts, _ = KO.SO.oracle_weighted_playout(vec.spec, vec.o.st, np.zeros(P, np.int64), steps, SEED, x)
    wexp = TO.oracle_traj(vec.spec, vec.o.st, np.zeros(P, np.int64), wacts)
    wplay = env.playouts(P, steps, SEED, weights=x, rewards=True, masks=True)
    TO.assert_traj(wplay, wexp, 'adapter, weighted', ('rewards', 'masks'))
    for t in range(steps):
        ran = wplay.length > t
        got = choose_weighted(wplay.masks[t][ran], np.broadcast_to(x, (int(ran.sum()), A)), SEED, pairs[ran], t, A, words=playout_words(SEED, pairs[ran], t))
        assert (np.asarray(got[0]) == wacts[t][ran]).all()
    # refusals travel through the forwarding
    with pytest.raises(ValueError, match="None or 'lidar'"):
        env.playouts(P, steps, SEED, observe='rgb')
    vec.lidar = None
    with pytest.raises(ValueError, match='lidar_configure'):
        env.playouts(P, steps, SEED, observe='lidar')


def test_limit_actions_reports_masks_in_its_own_ids_and_follows_the_backends_lidar(monkeypatch):
    """LimitActions.playouts on the stand-in: the limited env is the oracle on the limited spec (what limit_actions_vec builds on the device)."""
    from gym_novel_gridworlds_amd import wrappers
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    made = []

    def stand_in(vec, names):
        new = TO.OracleVecTraj(wrappers.limited_spec(vec.spec, names), vec.num_envs, seed=vec.o.seed)
        new.reset()
        if vec.lidar is not None:
            new.lidar_configure(vec.lidar, dtype=vec.lidar_dtype)
        made.append(new)
        return new
    monkeypatch.setattr(wrappers, 'limit_actions_vec', stand_in)
    env = _adapter(monkeypatch)
    vec = env.unwrapped._backend()
    lim = LimitActions(env, {'Break', 'Forward', 'Left'})
    # ids of its own that are no permutation of 0 .. 2: bit i of the kernel's word must move to bit ids[i]
    lim.set_limited_actions_id({'Break': 5, 'Forward': 0, 'Left': 3})
    names = sorted(lim.limited_actions)
    ids = [lim.limited_actions_id[name] for name in names]
    P, steps = 6, 4
    play = lim.playouts(P, steps, SEED, rewards=True, masks=True)
    limited = made[0]
    _, rep, acts, _ = KO.SO.PO.oracle_playout(limited.spec, vec.o.st, np.zeros(P, np.int64), steps, SEED)
    e = TO.oracle_traj(limited.spec, vec.o.st, np.zeros(P, np.int64), acts)
    assert isinstance(play, PlayoutTraj) and play.obs is None and (play.rewards == e['rewards']).all()
    assert (play.first_action == np.asarray(ids, np.int32)[rep['first_action']]).all()
    assert (play.masks == limit_mask_words(e['masks'], ids)).all() and (play.masks != 0).sum() == rep['length'].sum()
    assert ((play.masks[0] >> play.first_action.astype(np.uint64)) & np.uint64(1)).all()       # the action it reports is a bit of the word it reports
    assert (play.masks & ~np.uint64(sum(1 << i for i in ids))).sum() == 0
    # observe: refused while the backend has no lidar; then the limited env takes the backend's configuration - and takes it AGAIN when that changes
    with pytest.raises(ValueError, match='lidar_configure'):
        lim.playouts(P, steps, SEED, observe='lidar')
    vec.lidar_configure(num_beams=8, dtype=np.int32)
    first = lim.playouts(P, steps, SEED, observe='lidar')
    assert limited.lidar is vec.lidar and limited.configured == 1 and first.obs.shape[:2] == (steps + 1, P)
    lim.playouts(P, steps, SEED, observe='lidar')
    assert limited.configured == 1                                  # (unchanged: not configured again)
    vec.lidar_configure(num_beams=10, dtype=np.int16)
    second = lim.playouts(P, steps, SEED, observe='lidar', masks=True)
    assert limited.lidar is vec.lidar and limited.lidar_dtype == np.int16 and limited.configured == 2
    assert second.obs.shape[-1] == vec.lidar.obs_len(vec.spec) != first.obs.shape[-1]
    e10 = TO.oracle_traj(limited.spec, vec.o.st, np.zeros(P, np.int64), acts, lc=vec.lidar)
    assert (second.obs == e10['obs']).all() and (second.masks == play.masks).all()
    lim.close()


def test_sharded_env_returns_what_one_env_returns():
    spec = T.build_spec('pogo10')
    seed = KO.SO.XO.good_seed(spec, 6)
    sh = TO.sharded_on_oracle(spec=spec, global_num_envs=6, seed=seed)
    sh.reset()
    sh.local.lidar_configure()
    whole = TO.OracleVecTraj(spec, 6, seed=seed)
    whole.reset()
    whole.lidar_configure()
    got = sh.playouts(2, 3, SEED, rewards=True, masks=True, observe='lidar')
    exp = whole.playouts(2, 3, SEED, rewards=True, masks=True, observe='lidar')
    assert got.rewards.shape == (3, 6, 2) and got.masks.shape == (3, 6, 2) and got.obs.shape[:3] == (4, 6, 2) and (got.masks != 0).any() and (got.obs != 0).any()
    for name in ('rewards', 'masks', 'obs', 'ret', 'length'):
        assert (got[name] == exp[name]).all(), name
    assert (got.rewards.sum(0) == got.ret).all()
    assert type(sh.playouts(2, 3, SEED)) is Playout
