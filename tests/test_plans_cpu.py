"""Plan evaluation, host side (no GPU): the C-ABI and Python surfaces, the single-env adapter's [P, T] form, the LimitActions id mapping,
wrapper delegation and the sharded split on the oracle backend (tests/plan_oracle.py OracleVecPlans), host validation, and the oracle helper
the GPU tests compare against, pinned to the reference's recorded solved episodes.

test_oracle_helper_* pin the test helper, not the product: they run the CPU oracle alone.  Every other test here, and every test of
tests/test_plans.py, exercises the product's evaluate_plans / ngw_plan_eval."""
import os
import re

import numpy as np
import pytest

import mask_oracle as M
import ngw_testlib as T
import plan_oracle as PO
from gym_novel_gridworlds_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_API = ['ngw_plan_eval', 'ngw_get_plan_eval', 'ngw_plan_eval_device_ptrs']
CFG_SOLVED = sorted(c for c, v in T.spec_json()['cfgs'].items() if v['n_solved'] > 0)


def test_header_declares_and_library_exports_the_plan_api():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    L = _cabi.lib()
    for name in PLAN_API:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert hasattr(L, name), name
        assert name in _cabi.SYMBOLS
    assert L.ngw_abi_version() == 3


def test_null_arguments_are_refused_without_a_gpu():
    L = _cabi.lib()
    for call in (lambda: L.ngw_plan_eval(None, None, 0, 1, 1), lambda: L.ngw_get_plan_eval(None, None, None, None, None),
                 lambda: L.ngw_plan_eval_device_ptrs(None, None, None, None, None, None, None)):
        assert call() == _cabi.E_INVALID_ARG
        assert 'NULL' in _cabi.last_error()


def test_python_surface_has_the_method():
    from gym_novel_gridworlds_amd import LidarInFront, LimitActions, VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.envs import _NovelGridworldEnv
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    from gym_novel_gridworlds_amd.observation_wrappers import AgentMap
    from gym_novel_gridworlds_amd.wrappers import SaveTrajectories
    for cls in (VecNovelGridworld, ShardedVecNovelGridworld, _NovelGridworldEnv, NoveltyWrapper, LimitActions, LidarInFront, AgentMap, SaveTrajectories):
        assert callable(getattr(cls, 'evaluate_plans', None)), cls.__name__
    assert LimitActions.evaluate_plans is not NoveltyWrapper.evaluate_plans      # (it maps the ids out of its own id space)
    assert callable(VecNovelGridworld.evaluate_plans_ptr)


def test_plan_eval_tuple_and_its_goal_and_died_properties():
    from gym_novel_gridworlds_amd.vec_env import PlanEval
    info = np.array([[3, 1, (14 << 8), (14 << 8) | 1]], np.uint32)
    e = PlanEval(np.zeros((1, 4), np.int32), np.ones((1, 4), np.int32), np.array([[True, True, True, False]]), info)
    ret, length, ended, words = e                                   # (unpacks in that order)
    assert e['ret'] is ret and e['info'] is words and e.row(0).ended.shape == (4,)
    assert e.goal.tolist() == [[True, False, False, False]] and e.died.tolist() == [[False, False, True, False]]


@pytest.mark.parametrize('cfg', CFG_SOLVED)
def test_oracle_helper_agrees_with_reference_solved_episodes(cfg):
    """A recorded solved episode used as a plan returns the recorded rewards' sum and length up to the recorded goal step and ends with
    the goal bit; and the state handed in does not change."""
    spec, st, plans, ret, length = PO.solved_plans(cfg)
    before = [x.copy() for x in st.arrays()]
    t = PO.oracle_plans(spec, st, plans)
    assert all((a == b).all() for a, b in zip(before, st.arrays()))
    assert t['ret'][:, 0].tolist() == ret and t['length'][:, 0].tolist() == length
    assert t['ended'].all() and ((t['info'] >> 1) & 1).all()


def test_oracle_helper_stops_at_the_horizon_and_at_the_sticky_done():
    g = T.golden('pogo10')
    spec = T.build_spec('pogo10')
    cs = spec.compile()
    n, H = 12, 9
    sl = slice(0, n)
    sc = (H - 1 - np.arange(n) % 3).astype(np.int32)                # 1, 2 or 3 steps below the horizon
    st = M.state_from(spec, g['ss_pre_map'][sl], g['ss_pre_loc'][sl], g['ss_pre_facing'][sl], g['ss_pre_inv'][sl] * 0, g['ss_pre_sel'][sl] * 0,
                      step_count=sc)
    plans = np.ones((n, 2, 6), np.int32)                             # turning on the spot: no goal within six steps
    t = PO.oracle_plans(spec, st, plans, autoreset=True, horizon=H)
    assert (t['length'] == (H - sc)[:, None]).all() and t['ended'].all() and not ((t['info'] >> 1) & 1).any()
    assert (t['ret'] == (H - sc)[:, None] * cs.reward_step).all()
    off = PO.oracle_plans(spec, st, plans)                           # autoreset off: no horizon, the whole plan runs
    assert (off['length'] == 6).all() and not off['ended'].any()
    st.inv[:, cs.goal_item] = 1                                      # sticky done: the first step ends it, with the forced reward
    t = PO.oracle_plans(spec, st, plans)
    assert (t['length'] == 1).all() and t['ended'].all() and (t['ret'] == cs.reward_done).all() and ((t['info'] >> 1) & 1).all()


def _oracle_env(cfg):
    import gym_novel_gridworlds_amd as G
    env_id, S, nov = T.CFGS[cfg]
    env = G.make(env_id)
    env._make_backend = lambda spec, seed_: PO.OracleVecPlans(spec, 1, seed=seed_)
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
def test_adapter_takes_p_by_t_and_predicts_its_own_steps(cfg):
    """The single-env adapter takes [P, T] and returns [P] arrays, through every NoveltyWrapper on top (plain delegation); the returns it
    predicts are what stepping the plan then collects; attribute edits made since the last step are pushed first."""
    env = _oracle_env(cfg)
    env.reset()
    base = _base(env)
    A = len(base.actions_id)
    rs = np.random.RandomState(3)
    for i in range(12):
        plans = rs.randint(0, A, (5, 7))
        e = env.evaluate_plans(plans)
        assert [e[k].shape for k in ('ret', 'length', 'ended', 'info')] == [(5,)] * 4
        assert e.ret.dtype == np.int32 and e.length.dtype == np.int32 and e.ended.dtype == np.bool_ and e.info.dtype == np.uint32
        p = int(rs.randint(0, 5))
        total, steps, d = 0, 0, False
        for a in plans[p]:
            _, r, d, inf = env.step(int(a))
            total, steps = total + r, steps + 1
            if d:
                break
        assert (total, steps, bool(d)) == (int(e.ret[p]), int(e.length[p]), bool(e.ended[p])), (cfg, i, p)
        assert bool(inf['result']) == bool(e.info[p] & 1)
        if d or i % 4 == 3:
            env.reset()
    env.reset()
    goal = base._spec.item_names[base._spec.compile().goal_item]
    base.inventory_items_quantity[goal] = 1                          # an attribute edit is seen by the next evaluation
    e = env.evaluate_plans(np.ones((3, 4), np.int64))
    assert e.ended.all() and (e.length == 1).all() and e.goal.all() and not e.died.any()
    with pytest.raises(AssertionError):
        env.evaluate_plans(np.ones(4, np.int32))                     # not [P, T]
    env.close()


def test_limit_actions_maps_plans_out_of_its_id_space():
    """LimitActions takes plans in its own id space: each id through the two look-ups of step(); an id beyond the limited table and an id
    whose name the env no longer has (an action a wrapper removed) raise step()'s AssertionErrors before anything runs."""
    import gym_novel_gridworlds_amd as G
    from gym_novel_gridworlds_amd.wrappers import limit_plan_ids
    limited = {'Forward', 'Left', 'Right', 'Break', 'Craft_plank', 'Craft_stick'}
    names = sorted(limited)
    w = G.LimitActions(_oracle_env('pogo10'), limited)
    w.reset()
    base = _base(w)
    vec = base._backend()
    rs = np.random.RandomState(7)
    for i in range(8):
        plans = rs.randint(0, len(limited), (4, 6))
        e = w.evaluate_plans(plans)
        full = base.evaluate_plans(np.array([[w.actions_id[names[a]] for a in row] for row in plans]))
        for k in ('ret', 'length', 'ended', 'info'):
            assert e[k].shape == (4,) and (e[k] == full[k]).all(), (i, k)
        _, r, d, _ = w.step(int(plans[0, 0]))
        if d:
            w.reset()
    before = vec.launches
    with pytest.raises(AssertionError, match='is not valid, maxaction ID is 5'):
        w.evaluate_plans(np.array([[0, 6, 1]]))
    # the mapping function alone: a limited name the env's table does not hold (removed below the wrapper)
    actions_id = {'Forward': 0, 'Left': 1, 'Right': 2, 'Break': 3, 'Craft_plank': 7}
    lim = dict(zip(sorted(['Break', 'Forward', 'Craft_plank', 'Nope']), range(4)))       # Break 0, Craft_plank 1, Forward 2, Nope 3
    assert limit_plan_ids([[0, 1], [2, 2]], lim, actions_id, 4).tolist() == [[3, 7], [0, 0]]
    assert limit_plan_ids(np.zeros((2, 0), np.int64), lim, actions_id, 4).shape == (2, 0)
    with pytest.raises(AssertionError, match='Nope is not a valid action'):
        limit_plan_ids([[0, 3]], lim, actions_id, 4, 'env')
    with pytest.raises(AssertionError, match='Action ID -1 is not valid'):
        limit_plan_ids([[-1]], lim, actions_id, 4)
    assert vec.launches == before, "a refused plan reached the backend"
    w.close()


def test_host_validation_raises_before_anything_runs():
    """An id outside the action list raises the ValueError step() raises - on the product's VecNovelGridworld.evaluate_plans the check
    comes before the library is touched (a handle-less object shows it), on the adapter before the backend is called."""
    from gym_novel_gridworlds_amd import VecNovelGridworld
    spec = T.build_spec('pogo10')
    v = VecNovelGridworld.__new__(VecNovelGridworld)                 # no handle: anything that reached the library would fail differently
    v.num_envs, v.device, v.actions_id = 3, 0, dict(spec.actions_id)
    A = len(spec.actions_id)
    for bad in (A, -1, 1000):
        plans = np.zeros((3, 2, 4), np.int64)
        plans[2, 1, 3] = bad
        with pytest.raises(ValueError, match='%d is not in list' % bad):
            v.evaluate_plans(plans)
    with pytest.raises(AssertionError):
        v.evaluate_plans(np.zeros((2, 2, 4), np.int32))              # not N envs
    with pytest.raises(AssertionError):
        v.evaluate_plans(np.zeros((3, 2, 4), np.float32))            # not integers
    v._h = None                                                      # (nothing for __del__ to close)
    env = _oracle_env('pogo10')
    env.reset()
    vec = _base(env)._backend()
    before = vec.launches
    with pytest.raises(ValueError, match='is not in list'):
        env.evaluate_plans(np.array([[0, A]]))
    assert vec.launches == before
    env.close()


def test_sharded_split_at_world_two_equals_the_unsharded_result():
    """Each rank of a two-rank group evaluates its slice of the GLOBAL [N, P, T] array: the two halves are the unsharded result."""
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld, shard_range
    spec = T.build_spec('axe10')
    n, P, steps = 24, 3, 9
    A = len(spec.actions_id)

    class Rank(ShardedVecNovelGridworld):
        def __init__(self, rank, world):                              # (a rank without a process group: what __init__ derives from it)
            self.rank, self.world, self.global_num_envs = rank, world, n
            self.first, self.num_envs = shard_range(n, world, rank)
            self.local = PO.OracleVecPlans(spec, self.num_envs, seed=3, env_index_base=self.first, autoreset=True, horizon=14)
            self.spec = spec

    whole = PO.OracleVecPlans(spec, n, seed=3, autoreset=True, horizon=14)
    whole.reset()
    rs = np.random.RandomState(2)
    acts = rs.randint(0, A, (10, n)).astype(np.int32)
    plans = rs.randint(0, A, (n, P, steps))
    for t in range(10):
        whole.step(acts[t])
    exp = whole.evaluate_plans(plans)
    for rank in range(2):
        sh = Rank(rank, 2)
        sh.reset()
        for t in range(10):
            sh.step(acts[t, sh.first:sh.first + sh.num_envs])
        got = sh.evaluate_plans(plans)
        for k in ('ret', 'length', 'ended', 'info'):
            assert got[k].shape == (n // 2, P) and (got[k] == exp[k][sh.first:sh.first + sh.num_envs]).all(), (rank, k)
        with pytest.raises(AssertionError):
            sh.evaluate_plans(plans[:n // 2])                        # the local slice alone is not the global array
