"""One-step lookahead tables, host side (no GPU): the C-ABI and Python surfaces, the LimitActions column mapping, wrapper delegation and
the single-env adapter on the oracle backend, the decode of a table's info words, and the oracle helper the GPU tests compare against,
tied to the reference's recorded single-step outcomes (G4).

test_oracle_helper_agrees_with_reference_single_steps and test_oracle_helper_reports_the_horizon_under_autoreset pin the test helper
(tests/lookahead_oracle.py), not the product: they run the CPU oracle alone, so they do not depend on the library having the feature.
Every other test here, and every test of tests/test_lookahead.py, exercises the product's lookahead."""
import os
import re

import numpy as np
import pytest

import lookahead_oracle as LO
import mask_oracle as M
import ngw_testlib as T
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.spec import STEP_COSTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOK_API = ['ngw_lookahead', 'ngw_get_lookahead', 'ngw_lookahead_device_ptrs']
CFG_G4 = sorted(T.spec_json()['cfgs'])


def test_header_declares_and_library_exports_the_lookahead_api():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    L = _cabi.lib()
    for name in LOOK_API:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert hasattr(L, name), name
        assert name in _cabi.SYMBOLS
    assert L.ngw_abi_version() == 3


def test_null_handle_is_refused_without_a_gpu():
    L = _cabi.lib()
    for call in (lambda: L.ngw_lookahead(None), lambda: L.ngw_get_lookahead(None, None, None, None),
                 lambda: L.ngw_lookahead_device_ptrs(None, None, None, None, None, None)):
        assert call() == _cabi.E_INVALID_ARG
        assert 'NULL' in _cabi.last_error()


def test_python_surface_has_the_lookahead_method():
    from gym_novel_gridworlds_amd import LidarInFront, LimitActions, VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.envs import _NovelGridworldEnv
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    from gym_novel_gridworlds_amd.observation_wrappers import AgentMap
    for cls in (VecNovelGridworld, ShardedVecNovelGridworld, _NovelGridworldEnv, NoveltyWrapper, LimitActions, LidarInFront, AgentMap):
        assert callable(getattr(cls, 'lookahead', None)), cls.__name__
    assert LimitActions.lookahead is not NoveltyWrapper.lookahead      # (it maps columns into its own id space)


@pytest.mark.parametrize('cfg', CFG_G4)
def test_oracle_helper_agrees_with_reference_single_steps(cfg):
    """For each recorded (injected state, action, outcome) of G4, the helper's entry for that action is the recorded outcome: reward,
    done, result, step cost and message; and its `result` columns are unpack_action_masks of the oracle's mask words."""
    g = T.golden(cfg)
    spec = T.build_spec(cfg)
    st = M.state_from(spec, g['ss_pre_map'], g['ss_pre_loc'], g['ss_pre_facing'], g['ss_pre_inv'], g['ss_pre_sel'])
    t = LO.oracle_lookahead(spec, st)
    n, A = st.n, spec.compile().n_actions
    assert all(t[k].shape == (n, A) for k in t)
    rows, act = np.arange(n), g['ss_action'].astype(np.int64)
    w = t['info'][rows, act]
    out = dict(reward=t['reward'][rows, act], done=t['done'][rows, act], result=t['result'][rows, act], cost_code=(w >> 2) & 63,
               msg_code=(w >> 8) & 255, msg_arg=w >> 16)
    for c in range(n):
        T.check_outs(spec, out, c, act[c], g['ss_reward'][c], g['ss_done'][c], g['ss_result'][c], g['ss_cost'][c], g['ss_cost_is_int'][c],
                     g['ss_msg'][c], '%s single-step case %d' % (cfg, c))
    assert ((t['info'] & 1).astype(bool) == t['result']).all()
    assert (t['result'] == M.oracle_masks(spec, st)).all()
    # autoreset off: done is the goal test alone, and info bit 1 says the same
    assert (((t['info'] >> 1) & 1).astype(bool) == t['done']).all()


def test_oracle_helper_reports_the_horizon_under_autoreset():
    """One step below the horizon every action ends the episode: done = 1 everywhere, info bit 1 only where the goal was reached; the
    other fields are those of the table without autoreset.  The stepped copy resets; the state handed in does not change."""
    g = T.golden('pogo10')
    spec = T.build_spec('pogo10')
    n = len(g['ss_action'])
    sc = np.where(np.arange(n) % 2 == 0, 6, 2).astype(np.int32)
    st = M.state_from(spec, g['ss_pre_map'], g['ss_pre_loc'], g['ss_pre_facing'], g['ss_pre_inv'], g['ss_pre_sel'], step_count=sc)
    before = [x.copy() for x in st.arrays()]
    plain = LO.oracle_lookahead(spec, st)
    auto = LO.oracle_lookahead(spec, st, autoreset=True, horizon=7)
    assert all((a == b).all() for a, b in zip(before, st.arrays()))
    assert (auto['reward'] == plain['reward']).all() and (auto['info'] == plain['info']).all()
    assert auto['done'][0::2].all()
    assert (auto['done'][1::2] == plain['done'][1::2]).all()


def test_limit_actions_column_mapping_of_a_table():
    from gym_novel_gridworlds_amd.wrappers import limit_column_ids, limit_mask_columns
    actions_id = {'Forward': 0, 'Left': 1, 'Right': 2, 'Break': 3, 'Craft_plank': 7}
    limited = dict(zip(sorted(['Break', 'Forward', 'Craft_plank', 'Nope']), range(4)))   # Break 0, Craft_plank 1, Forward 2, Nope 3
    reward = np.arange(16, dtype=np.int32).reshape(2, 8) - 5
    got = limit_mask_columns(reward, limited, actions_id, 4, np.int32)
    assert got.dtype == np.int32 and got.tolist() == [[-2, 2, -5, 0], [6, 10, 3, 0]]
    info = (np.arange(16, dtype=np.uint32).reshape(2, 8) << np.uint32(20)) | np.uint32(1)
    got = limit_mask_columns(info, limited, actions_id, 4, np.uint32)
    assert got.dtype == np.uint32 and (got[:, :3] == info[:, [3, 7, 0]]).all() and (got[:, 3] == 0).all()
    assert limit_mask_columns(reward[0] > 0, limited, actions_id, 4).dtype == np.bool_      # (the mask form is unchanged)
    assert limit_column_ids(limited, actions_id, 4, 8) == [3, 7, 0, None] and limit_column_ids(limited, actions_id, 4, 7) == [3, None, 0, None]


def _oracle_env(cfg):
    import gym_novel_gridworlds_amd as G
    env_id, S, nov = T.CFGS[cfg]
    env = G.make(env_id)
    env._make_backend = lambda spec, seed_: LO.OracleVecLook(spec, 1, seed=seed_)
    env.seed(5)
    env.map_size = S
    for one in T.novelty_list(nov):
        env = G.inject_novelty(env, *one)
    return env


def _base(env):
    while hasattr(env, 'env') and not hasattr(env, '_backend'):
        env = env.env
    return env


@pytest.mark.parametrize('cfg', ['pogo10', 'axe10', 'fire10h'])
def test_adapter_and_wrappers_on_the_oracle_backend(cfg):
    """The single-env adapter returns arrays of length A that predict its own next step(), through every NoveltyWrapper on top (plain
    delegation); attribute edits made since the last step are pushed first; LimitActions answers in its own id space."""
    import gym_novel_gridworlds_amd as G
    env = _oracle_env(cfg)
    env.reset()
    base = _base(env)
    A = len(base.actions_id)
    rs = np.random.RandomState(3)
    for i in range(60):
        t = env.lookahead()
        assert [t[k].shape for k in ('reward', 'done', 'result', 'info')] == [(A,)] * 4
        assert t.reward.dtype == np.int32 and t.done.dtype == np.bool_ and t.result.dtype == np.bool_ and t.info.dtype == np.uint32
        reward, done, result, info = t                              # (unpacks in that order)
        a = int(rs.randint(0, A))
        _, r, d, inf = env.step(a)
        assert (r, d, inf['result']) == (int(reward[a]), bool(done[a]), bool(result[a])), (cfg, i, a)
        assert inf['step_cost'] == STEP_COSTS[int((info[a] >> 2) & 63)]
        assert inf['message'] == base._spec.format_message(a, int((info[a] >> 8) & 255), int(info[a] >> 16))
        if d or i % 20 == 19:
            env.reset()
    # an attribute edit is seen by the next lookahead (the reference's users inject state that way)
    env.reset()
    goal = base._spec.item_names[base._spec.compile().goal_item]
    base.inventory_items_quantity[goal] = 1
    t = env.lookahead()
    assert t.done.all() and (t.reward == base._spec.compile().reward_done).all()
    env.close()
    # LimitActions: the table in the limited id space
    limited = {'Forward', 'Left', 'Right', 'Break', 'Craft_plank', 'Craft_stick'}
    w = G.LimitActions(_oracle_env(cfg), limited)
    w.reset()
    names = sorted(limited)
    for i in range(20):
        t, full = w.lookahead(), _base(w).lookahead()
        cols = [w.actions_id[nm] for nm in names]
        for k in ('reward', 'done', 'result', 'info'):
            assert t[k].shape == (len(limited),) and (t[k] == full[k][cols]).all(), (i, k)
        a = int(rs.randint(0, len(limited)))
        _, r, d, inf = w.step(a)
        assert (r, d, inf['result']) == (int(t.reward[a]), bool(t.done[a]), bool(t.result[a])), (cfg, i, a)
        if d:
            w.reset()
    w.close()


def test_info_words_of_a_table_decode_with_the_step_helpers():
    """decode_info_words(column) is a StepInfo: step_costs() and messages() of VecNovelGridworld take it as they take a step's info."""
    from gym_novel_gridworlds_amd.vec_env import StepInfo, VecNovelGridworld, decode_info_words
    g = T.golden('axe10')
    spec = T.build_spec('axe10')
    st = M.state_from(spec, g['ss_pre_map'], g['ss_pre_loc'], g['ss_pre_facing'], g['ss_pre_inv'], g['ss_pre_sel'])
    t = LO.oracle_lookahead(spec, st)
    v = VecNovelGridworld.__new__(VecNovelGridworld)                 # (the two helpers read nothing but the spec)
    v.spec = spec
    for a in range(t['info'].shape[1]):
        o = LO.Oracle(spec.compile(), st.n)
        o.st = st.copy()
        o.step(np.full(st.n, a, np.int32))
        info = decode_info_words(t['info'][:, a])
        assert isinstance(info, StepInfo)
        assert (info['result'] == t['result'][:, a]).all() and (info['step_cost_code'] == o.cost_code).all()
        assert v.step_costs(info) == [STEP_COSTS[int(c)] for c in o.cost_code]
        assert v.messages(info, np.full(st.n, a)) == [spec.format_message(a, int(c), int(x)) for c, x in zip(o.msg_code, o.msg_arg)]
    row = decode_info_words(t['info'][3])                            # one env's row: actions = range(A)
    assert len(v.messages(row, range(t['info'].shape[1]))) == t['info'].shape[1]
