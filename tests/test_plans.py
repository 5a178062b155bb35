"""Plan evaluation on the MI355X (csrc/ngw_plans.inc, include/ngw.h ngw_plan_eval ...), held to the CPU oracle: the expected result of a
plan is what the unmodified oracle collects when a copy of the state is stepped through it and stopped at the first episode end
(tests/plan_oracle.py) - never the device's own step."""
import ctypes as C

import numpy as np
import pytest

import mask_oracle as M
import ngw_testlib as T
import plan_oracle as PO
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.spec import F_INVALID_ACTION, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_ALL = sorted(T.CFGS)
CFG_SOLVED = sorted(c for c, v in T.spec_json()['cfgs'].items() if v['n_solved'] > 0)
STATE_KEYS = ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode')


def load_state(v, st):
    v.set_state(0, map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, selected=st.selected, step_count=st.step_count)


def oracle_state(spec, v):
    s = v.get_state()
    st = M.state_from(spec, s['map'], s['loc'], s['facing'], s['inv'], s['selected'], step_count=s['step_count'])
    st.episode[...] = s['episode']
    return st


def good_seed(spec, n, lo=4):
    return next(sd for sd in range(lo, lo + 40) if not Oracle(spec.compile(), n, seed=sd).reset() & 2)   # (tight maps can exhaust the placement)


def check(v, spec, st, plans, where, **kw):
    exp = PO.oracle_plans(spec, st, plans, autoreset=v.autoreset, horizon=v.horizon)
    got = v.evaluate_plans(plans, copy=True, **kw)
    PO.assert_plans(got, exp, where)
    assert ((got.length >= 1) & (got.length <= plans.shape[2])).all(), where
    return got


@pytest.mark.parametrize('cfg', CFG_ALL)
def test_every_configuration_after_reset_and_along_random_play(cfg):
    """130 envs (two full waves and a partial one), P = 3, T = 12, random plans: right after reset and after 60 random steps, with
    autoreset off and with autoreset on under a horizon of 25."""
    spec = T.build_spec(cfg)
    n, A, P, steps = 130, len(spec.actions_id), 3, 12
    seed = good_seed(spec, n)
    rs = np.random.RandomState(5)
    for auto in (False, True):
        kw = dict(autoreset=True, horizon=25) if auto else {}
        v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
        o = Oracle(spec.compile(), n, seed=seed, **kw)
        v.reset(); o.reset()
        check(v, spec, o.st, rs.randint(0, A, (n, P, steps)), '%s after reset auto=%d' % (cfg, auto))
        for t in range(60):
            a = rs.randint(0, A, n).astype(np.int32)
            if o.step(a) & 2:                                   # a tight map exhausted the placement of an autoreset: stop here
                break
            v.step(a)
        check(v, spec, o.st, rs.randint(0, A, (n, P, steps)), '%s after random play auto=%d' % (cfg, auto))
        assert v.error_flags() == 0
        v.close()


@pytest.mark.parametrize('S', [9, 10, 12, 32])
@pytest.mark.parametrize('n', [1, 63, 65])
def test_map_sizes_batch_sizes_and_plan_shapes(S, n):
    """One map size per staging form (BYTE 9, STRAIGHT 10, DWORD 12) and the size that needs the LDS opt-in above 64 KiB (32), batch sizes
    around the wavefront width, (P, T) in (1, 1), (5, 2), (64, 7), the host and the device result form."""
    spec = make_spec(T.POGO, S)
    A = len(spec.actions_id)
    seed = good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=30)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=30)
    v.reset(); o.reset()
    rs = np.random.RandomState(S + n)
    for t in range(25):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    for P, steps in ((1, 1), (5, 2), (64, 7)):
        plans = rs.randint(0, A, (n, P, steps))
        where = 'S=%d n=%d P=%d T=%d' % (S, n, P, steps)
        host = check(v, spec, o.st, plans, where)
        dev = v.evaluate_plans(plans, device=True)
        for k in ('ret', 'length', 'ended'):
            assert tuple(dev[k].shape) == (n, P) and (dev[k].cpu().numpy() == host[k]).all(), (where, k)
        assert (dev['info'].cpu().numpy().view(np.uint32) == host['info']).all(), where
        assert (dev.goal.cpu().numpy() == host.goal).all() and (dev.died.cpu().numpy() == host.died).all()
    v.close()


def test_horizon_inside_a_plan():
    """step_count injected to H - k for k in 1 .. 3 under a horizon H: length = k, ended, info bit 1 clear (a horizon cut is not the goal)."""
    spec = T.build_spec('pogo10')
    n, H, P, steps = 130, 11, 2, 6
    seed = good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.reset(); o.reset()
    st = o.st.copy()
    k = 1 + np.arange(n) % 3
    st.step_count[...] = H - k
    load_state(v, st)
    plans = np.ones((n, P, steps), np.int32)                     # Left: turning on the spot reaches no goal
    plans[:, 1, :] = 2
    got = check(v, spec, st, plans, 'horizon inside a plan')
    assert (got.length == k[:, None]).all() and got.ended.all() and not got.goal.any() and not ((got.info >> 1) & 1).any()
    v.close()


def test_sticky_done_with_autoreset_off():
    """Envs that hold the goal item, autoreset off: every plan has length 1 and the forced reward."""
    spec = T.build_spec('axe10')
    cs = spec.compile()
    n, A = 130, len(spec.actions_id)
    seed = good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    o = Oracle(cs, n, seed=seed)
    v.reset(); o.reset()
    st = o.st.copy()
    st.inv[0::2, cs.goal_item] = 1
    load_state(v, st)
    got = check(v, spec, st, np.random.RandomState(1).randint(0, A, (n, 4, 5)), 'sticky done')
    assert (got.length[0::2] == 1).all() and got.ended[0::2].all() and (got.ret[0::2] == cs.reward_done).all() and got.goal[0::2].all()
    v.close()


def _place_agents(spec, st, want):
    """Moves each env's agent onto an air cell with a 4-neighbour holding item `want`; returns the envs where one was found."""
    S = spec.map_size
    hit = []
    for i in range(st.n):
        m = st.map[i].reshape(S, S)
        cells = [(r, c) for r in range(1, S - 1) for c in range(1, S - 1)
                 if m[r, c] == 0 and want in (m[r - 1, c], m[r + 1, c], m[r, c - 1], m[r, c + 1])]
        if cells:
            st.loc[i] = cells[0]
            hit.append(i)
    return np.array(hit, np.int64)


def test_firewall_death_inside_a_plan():
    """fire10h with agents placed beside the fire: the plan dies at step 1 (or 2, where the wrapper nesting skips the first action's
    check), and the later steps add nothing - the same plans cut after the deadly step give the same results."""
    spec = T.build_spec('fire10h')
    cs = spec.compile()
    n, A = 130, len(spec.actions_id)
    seed = good_seed(spec, n)
    o = Oracle(cs, n, seed=seed)
    o.reset()
    st = o.st.copy()
    hit = _place_agents(spec, st, cs.fire_item)
    assert len(hit) > n // 4
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    v.reset()
    load_state(v, st)
    plans = np.random.RandomState(3).randint(0, A, (n, 3, 8))
    got = check(v, spec, st, plans, 'fire10h beside the fire')
    died = got.died[hit]
    assert died.any() and (got.length[hit][died] <= 2).all() and (((got.info[hit][died] >> 8) & 255) == 14).all()
    short = check(v, spec, st, plans[:, :, :2], 'fire10h, plans cut to two steps')
    sel = got.died & (got.length <= 2)
    for k in ('ret', 'length', 'ended', 'info'):
        assert (got[k][sel] == short[k][sel]).all(), k
    v.close()


@pytest.mark.parametrize('cfg', CFG_SOLVED)
def test_reference_recorded_solved_episodes_as_plans(cfg):
    """The reference's recorded solved episodes, loaded from their recorded start states and used as plans (padded with Left to the
    longest): ret is the sum of the recorded rewards and length the recorded step count up to the recorded goal step - the recordings
    run on past it under the sticky done, a plan stops there (plan_oracle.solved_plans) -, ended with the goal bit."""
    spec, st, plans, ret, length = PO.solved_plans(cfg)
    v = VecNovelGridworld(spec=spec, num_envs=st.n, seed=1)
    v.reset()
    load_state(v, st)
    got = v.evaluate_plans(plans, copy=True)
    assert got.ret[:, 0].tolist() == ret and got.length[:, 0].tolist() == length
    assert got.ended.all() and got.goal.all() and not got.died.any()
    v.close()


@pytest.mark.parametrize('cfg', ['pogo10', 'axe10', 'stk_fr_crate12'])
def test_one_step_plans_are_the_lookahead_columns(cfg):
    """T = 1: column p equals lookahead() column a for plans[..., 0] = a, over all A actions, on the injected G4 states."""
    g = T.golden(cfg)
    spec = T.build_spec(cfg)
    st = M.state_from(spec, g['ss_pre_map'], g['ss_pre_loc'], g['ss_pre_facing'], g['ss_pre_inv'], g['ss_pre_sel'])
    n, A = st.n, len(spec.actions_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    v.reset()
    load_state(v, st)
    plans = np.tile(np.arange(A)[None, :, None], (n, 1, 1))
    got = check(v, spec, st, plans, cfg + ' T=1')
    look = v.lookahead(copy=True)
    assert (got.ret == look.reward).all() and (got.ended == look.done).all() and (got.info == look.info).all() and (got.length == 1).all()
    v.close()


def _everything(v):
    st = v.get_state()
    reward, done, info = v.get_step_out(copy=True)
    out = {k: st[k].copy() for k in STATE_KEYS}
    out.update(reward=reward, done=done, words=v.action_mask_words(copy=True))
    out.update({'info_' + k: np.asarray(info[k]).copy() for k in ('result', 'step_cost_code', 'message_code', 'message_arg')})
    out.update({'look_' + k: np.asarray(x) for k, x in zip(('reward', 'done', 'result', 'info'), v.lookahead(copy=True))})
    return out


@pytest.mark.parametrize('cfg', ['pogo10', 'fire10h'])
def test_nothing_is_committed(cfg):
    """State, last step's outputs, mask words and lookahead table are byte-identical after an evaluation; a lookahead table overwritten
    through its zero-copy view reads back overwritten (still current); under autoreset the next 40 real steps equal the oracle's, so no
    prepared episode was consumed."""
    import torch
    spec = T.build_spec(cfg)
    n, A, H = 130, len(spec.actions_id), 12
    seed = good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.reset(); o.reset()
    rs = np.random.RandomState(9)
    for t in range(7):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    before = _everything(v)
    got = check(v, spec, o.st, rs.randint(0, A, (n, 6, 10)), cfg + ' before the real steps')
    assert got.ended.any()
    after = _everything(v)
    for k in before:
        assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), k
    d = v.lookahead(device=True)
    d['reward'].fill_(-77)
    torch.cuda.synchronize()
    v.evaluate_plans(rs.randint(0, A, (n, 2, 3)))
    assert (v.lookahead(copy=True)['reward'] == -77).all(), "an evaluation made the lookahead table stale"
    ends = 0
    for t in range(40):
        a = rs.randint(0, A, n).astype(np.int32)
        assert not o.step(a) & 2
        _, reward, done, _ = v.step(a, copy=True)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
        ends += int(done.sum())
        if t % 13 == 0:
            check(v, spec, o.st, rs.randint(0, A, (n, 2, 5)), '%s t=%d' % (cfg, t))
    s = v.get_state()
    for k, ref in zip(STATE_KEYS, (o.st.map, o.st.loc, o.st.facing, o.st.inv, o.st.selected, o.st.step_count, o.st.episode)):
        assert (s[k].reshape(ref.shape) == ref).all(), k
    assert ends >= 2 * n and v.error_flags() == 0
    v.close()


def test_adapter_steps_on_after_an_evaluation():
    """The single-env adapter: evaluate_plans ([P, T] in, [P] out) predicts what stepping the plan then collects, and the adapter keeps
    stepping correctly afterwards (its resident step loop is ended by the call and starts again)."""
    import gym_novel_gridworlds_amd as G
    np.random.seed(0)
    env = G.make('NovelGridworld-Pogostick-v1')
    env.reset()
    A = len(env.actions_id)
    rs = np.random.RandomState(4)
    for i in range(15):
        plans = rs.randint(0, A, (4, 6))
        e = env.evaluate_plans(plans)
        assert e.ret.shape == (4,) and e.ended.dtype == np.bool_
        spec = env._sync_spec()
        s = env._backend().get_state()
        st = M.state_from(spec, s['map'], s['loc'], s['facing'], s['inv'], s['selected'], step_count=s['step_count'])
        PO.assert_plans(PO.PlanRows(e), PO.oracle_plans(spec, st, plans[None]), 'adapter %d' % i)
        total, steps, d = 0, 0, False
        for a in plans[i % 4]:
            _, r, d, _ = env.step(int(a))
            total, steps = total + r, steps + 1
            if d:
                break
        assert (total, steps, bool(d)) == (int(e.ret[i % 4]), int(e.length[i % 4]), bool(e.ended[i % 4])), i
        if d:
            env.reset()
    env.close()


def test_invalid_ids_from_the_device():
    """Device plans are not validated: a plan with an out-of-range id at step k has the ret of the same plan with step k deleted and a
    length larger by one; the sticky NGW_F_INVALID_ACTION is raised; the state is untouched."""
    import torch
    spec = T.build_spec('axe10')
    n, A, P, steps, k = 130, len(spec.actions_id), 3, 6, 2
    seed = good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    o = Oracle(spec.compile(), n, seed=seed)
    v.reset(); o.reset()
    o.st.inv[0::5, spec.compile().goal_item] = 1                     # a fifth of the envs end at step 1 (sticky done): they never meet the id
    load_state(v, o.st)
    rs = np.random.RandomState(6)
    clean = rs.randint(0, A, (n, P, steps))
    bad = np.insert(clean, k, [A, -1, 1 << 20], axis=2)              # one invalid id per plan at step k
    exp = PO.oracle_plans(spec, o.st, clean)
    before = v.get_state()
    assert v.error_flags() == 0
    dev = torch.from_numpy(np.ascontiguousarray(bad.transpose(2, 1, 0), np.int32)).cuda()
    torch.cuda.synchronize()
    got = v.evaluate_plans(dev, copy=True)
    hit = exp['length'] > k                                          # the plan was still running when it met the invalid id
    assert hit.any() and not hit.all()
    assert (got.ret == exp['ret']).all() and (got.ended == exp['ended']).all() and (got.info == exp['info']).all()
    assert (got.length == exp['length'] + hit).all()
    assert v.error_flags() & F_INVALID_ACTION
    after = v.get_state()
    for key in STATE_KEYS:
        assert (before[key] == after[key]).all(), key
    one = torch.full((1, 1, n), A, dtype=torch.int32, device='cuda')  # T = 1, invalid: reward 0, length 1, info 0, not ended
    torch.cuda.synchronize()
    g1 = v.evaluate_plans(one, copy=True)
    assert (g1.ret == 0).all() and (g1.length == 1).all() and (g1.info == 0).all() and not g1.ended.any()
    v.close()


def test_cabi_errors():
    """Each NGW_E_INVALID_ARG case of include/ngw.h; S = 64 raises the error the fused rollout raises at that size."""
    import torch
    L = _cabi.lib()
    spec = T.build_spec('pogo10')
    n = 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset()
    plans = torch.zeros((2, 3, n), dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    p4 = [C.c_void_p() for _ in range(4)]
    E = _cabi.E_INVALID_ARG
    assert L.ngw_get_plan_eval(v._h, None, None, None, None) == E and 'before' in _cabi.last_error()
    assert L.ngw_plan_eval_device_ptrs(v._h, *[C.byref(x) for x in p4], None, None) == E and 'before' in _cabi.last_error()
    ptr = C.c_void_p(plans.data_ptr())
    assert L.ngw_plan_eval(None, ptr, n, 3, 2) == E and 'NULL' in _cabi.last_error()
    assert L.ngw_plan_eval(v._h, None, n, 3, 2) == E and 'NULL' in _cabi.last_error()
    assert L.ngw_plan_eval(v._h, ptr, n, 0, 2) == E and 'n_plans' in _cabi.last_error()
    assert L.ngw_plan_eval(v._h, ptr, n, 3, 0) == E and 'n_steps' in _cabi.last_error()
    assert L.ngw_plan_eval(v._h, ptr, n - 1, 3, 2) == E and 'env_stride' in _cabi.last_error()
    assert L.ngw_plan_eval(v._h, ptr, n, (1 << 31) - 1, 2) == E and '32 bits' in _cabi.last_error()
    assert L.ngw_get_plan_eval(None, None, None, None, None) == E and L.ngw_plan_eval_device_ptrs(None, None, None, None, None, None, None) == E
    assert L.ngw_get_plan_eval(v._h, None, None, None, None) == E, "a refused call counted as an evaluation"
    assert L.ngw_plan_eval(v._h, ptr, n, 3, 2) == 0
    assert L.ngw_get_plan_eval(v._h, None, None, None, None) == 0                      # any pointer may be NULL
    es, ps = C.c_int64(), C.c_int64()
    assert L.ngw_plan_eval_device_ptrs(v._h, None, None, None, C.byref(p4[3]), C.byref(es), C.byref(ps)) == 0
    assert p4[3].value and es.value == 1 and ps.value == 128
    with pytest.raises(ValueError):
        v.evaluate_plans_ptr(plans.data_ptr(), n, 0, 2)
    v.set_terminal_capture(True)                                                       # no reset runs: allowed under terminal capture
    assert L.ngw_plan_eval(v._h, ptr, n, 3, 2) == 0
    v.close()
    big = VecNovelGridworld(spec=make_spec(T.POGO, 64), num_envs=n, seed=4)
    big.reset()
    with pytest.raises(ValueError, match='64 maps in LDS') as roll:
        big.rollout_actions(plans.data_ptr(), n, 2)
    with pytest.raises(ValueError, match='64 maps in LDS') as ev:
        big.evaluate_plans(plans)
    assert 'ngw_plan_eval' in str(ev.value) and 'map_size 64' in str(ev.value) and 'map_size 64' in str(roll.value)
    big.close()


def test_growth_and_rebuild():
    """P = 2, then P = 9 (the result buffers are regrown), then inject_novelty (rebuild: a fresh handle with fresh buffers) and an
    evaluation against the new spec's oracle."""
    import copy
    from gym_novel_gridworlds_amd.novelty import apply_novelty
    spec = T.build_spec('axe10')
    n, A = 130, len(spec.actions_id)
    seed = good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    o = Oracle(spec.compile(), n, seed=seed)
    v.reset(); o.reset()
    rs = np.random.RandomState(2)
    check(v, spec, o.st, rs.randint(0, A, (n, 2, 8)), 'P=2')
    check(v, spec, o.st, rs.randint(0, A, (n, 9, 8)), 'P=9')
    check(v, spec, o.st, rs.randint(0, A, (n, 4, 8)), 'P=4 in the grown buffers')
    spec2 = copy.deepcopy(v.spec)
    apply_novelty(spec2, 'axetobreak', 'hard', 'wooden', '')
    v.rebuild(spec2)
    v.reset()
    st = oracle_state(spec2, v)
    got = check(v, spec2, st, rs.randint(0, len(spec2.actions_id), (n, 5, 8)), 'after rebuild')
    assert got.ret.shape == (n, 5) and v.error_flags() == 0
    v.close()
