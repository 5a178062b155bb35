"""Snapshot rollout on the MI355X (csrc/ngw_slot_rollout.inc, include/ngw.h ngw_snapshot_rollout, snapshot.py Snapshot.rollout), held to the
CPU oracle (tests/slot_rollout_oracle.py): the expected reports come from an oracle copy stepped under the handle's autoreset setting and
horizon, the expected end states from a copy stepped with autoreset off that only ever steps the pairs still alive - never from the
device's own step.  All results are integers and compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import plan_oracle as PO
import slot_rollout_oracle as RO
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, F_INVALID_ACTION, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_ALL = sorted(T.CFGS)
CFG_SOLVED = sorted(c for c, v in T.spec_json()['cfgs'].items() if v['n_solved'] > 0)
STATE_KEYS = RO.STATE_KEYS
REPORTS = ('ret', 'length', 'ended', 'info')


def load_state(v, st):
    v.set_state(0, map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, selected=st.selected, step_count=st.step_count)


def host(e):
    """A PlanEval of device tensors as numpy arrays ('info' as the uint32 words)."""
    return {k: (e[k].cpu().numpy().view(np.uint32) if k == 'info' else e[k].cpu().numpy()) for k in REPORTS}


def rollout_checked(v, spec, snap, rows, parents, plans, children, where, **kw):
    """One rollout held to the oracle: `rows` is a host copy of the source's rows, plans [count, T].  Returns (PlanEval as numpy, expected
    end states, expected reports)."""
    plans = np.asarray(plans)
    p = np.arange(len(plans)) if parents is None else np.asarray(parents)
    ends, rep, _ = RO.oracle_slot_rollout(spec, rows, p, plans, v.autoreset, v.horizon)
    e = snap.rollout(parents, plans, children, **kw)
    RO.assert_reports(e, rep, where)
    if children is not None:
        RO.assert_rows(snap.state(), ends, where, idx=np.asarray(children))
    return e, ends, rep


@pytest.mark.parametrize('cfg', CFG_ALL)
def test_every_configuration_two_generations(cfg):
    """130 envs (two full waves and a partial one), right after reset and after up to 60 random steps, autoreset off and on under a horizon
    of 25: T = 4 random plans from the envs kept into a pool, then a second generation slot to slot in the same buffer with repeated
    parents."""
    spec = T.build_spec(cfg)
    n, A, steps = 130, len(spec.actions_id), 4
    seed = XO.good_seed(spec, n)
    rs = np.random.RandomState(12)
    for auto in (False, True):
        kw = dict(autoreset=True, horizon=25) if auto else {}
        v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
        o = Oracle(spec.compile(), n, seed=seed, **kw)
        v.reset(); o.reset()
        pool = v.snapshot(2 * n)
        for stage in ('after reset', 'after random play'):
            if stage == 'after random play':
                for t in range(60):
                    a = rs.randint(0, A, n).astype(np.int32)
                    if o.step(a) & 2:                           # a tight map exhausted the placement of an autoreset: stop here
                        break
                    v.step(a)
            where = '%s %s auto=%d' % (cfg, stage, auto)
            rollout_checked(v, spec, pool, o.st, None, rs.randint(0, A, (n, steps)), np.arange(n), where + ' gen 1', from_envs=True)
            parents = rs.randint(0, n, n)                       # end states of generation 1, some of them several times
            rollout_checked(v, spec, pool, pool.state(), parents, rs.randint(0, A, (n, steps)), n + rs.permutation(n), where + ' gen 2')
        assert v.error_flags() == 0
        v.close()


@pytest.mark.parametrize('S', [9, 10, 12, 32])
@pytest.mark.parametrize('count', [1, 63, 65, 200])
def test_map_sizes_and_counts(S, count):
    """One map size per staging form (odd S*S: 9, dwords: 10, 16-byte pieces: 12) and the size that needs the LDS opt-in above 64 KiB
    (32); counts around the wavefront width and far above num_envs = 5, so parents repeat heavily; T = 1, 2 and 7; host lists from the
    envs, device tensors slot to slot with the results left on the device, and a pure evaluation that leaves every slot byte-identical."""
    import torch
    spec = make_spec(T.POGO, S)
    n, A, cap = 5, len(spec.actions_id), 256
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=30)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=30)
    v.reset(); o.reset()
    rs = np.random.RandomState(S + count)
    for t in range(25):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    pool, second = v.snapshot(cap), v.snapshot(cap)
    for steps in (1, 2, 7):
        where = 'S=%d count=%d T=%d' % (S, count, steps)
        children = rs.permutation(cap)[:count]
        rollout_checked(v, spec, pool, o.st, rs.randint(0, n, count), rs.randint(0, A, (count, steps)), children, where + ' host lists', from_envs=True)
        # device tensors, slot to slot: the parents are the slots just written, the children the free ones
        rows = pool.state()
        free = np.setdiff1d(np.arange(cap), children)
        if len(free) < count:                                   # (count = 200 of 256: the second generation goes to a second buffer)
            dst, free = second, np.arange(cap)
        else:
            dst = pool
        parents, plans, kids_at = children[rs.randint(0, count, count)], rs.randint(0, A, (count, steps)), free[rs.permutation(len(free))[:count]]
        ends, rep, _ = RO.oracle_slot_rollout(spec, rows, parents, plans, True, 30)
        dev = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in (parents, plans.T, kids_at)]
        torch.cuda.synchronize()
        e = dst.rollout(dev[0], dev[1], dev[2], source=pool, device=True)
        assert all(isinstance(x, torch.Tensor) and tuple(x.shape) == (count,) for x in e) and e.info.dtype == torch.int32
        assert e.ended.dtype == torch.bool and e.ret.dtype == torch.int32 and e.length.dtype == torch.int32
        RO.assert_reports(host(e), rep, where + ' device tensors')
        assert (e.goal.cpu().numpy() == (rep['ended'] & ((rep['info'] >> 1) & 1).astype(bool))).all()
        RO.assert_rows(dst.state(), ends, where + ' device tensors', idx=kids_at)
        # a pure evaluation: the same reports, every slot of both pools as it was
        before = pool.state(), second.state()
        e = pool.rollout(dev[0], dev[1], device=True)
        RO.assert_reports(host(e), rep, where + ' nothing kept')
        e = pool.rollout(parents, plans)
        RO.assert_reports(e, rep, where + ' nothing kept, host lists')
        after = pool.state(), second.state()
        for b, a_ in zip(before, after):
            for k in STATE_KEYS:
                assert b[k].dtype == a_[k].dtype and b[k].tobytes() == a_[k].tobytes(), (where, k)
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('cfg', ['pogo10', 'fire10h', 'fence10e'])
def test_identities_with_expand_and_plan_evaluation(cfg):
    """T = 1 with children: the children and reports are oracle_expand's and what snap.expand leaves.  From the envs, parents = all envs,
    nothing kept: the reports are oracle_plans' for the same plan, and evaluate_plans'."""
    spec = T.build_spec(cfg)
    n, A, H = 130, len(spec.actions_id), 9
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.reset(); o.reset()
    rs = np.random.RandomState(6)
    for t in range(5):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    pool, twin = v.snapshot(3 * n), v.snapshot(3 * n)
    pool.save(slots=np.arange(n)); twin.save(slots=np.arange(n))
    count = 2 * n
    parents, acts, children = rs.randint(0, n, count), rs.randint(0, A, count), n + rs.permutation(count)
    kids, rep = XO.oracle_expand(spec, pool.state(), parents, acts, True, H)
    r = pool.rollout(parents, acts[:, None], children)
    x = twin.expand(parents, acts, children)
    assert (r.ret == rep['reward']).all() and (r.ended == rep['done']).all() and (r.info == rep['info']).all() and (r.length == 1).all()
    assert (r.ret == x.reward).all() and (r.ended == x.done).all() and (r.info == x.info).all()
    got, other = pool.state(), twin.state()
    XO.assert_rows(got, kids, cfg + ' T = 1 against oracle_expand', idx=children)
    for k in STATE_KEYS:
        assert got[k].tobytes() == other[k].tobytes(), k
    steps = 6
    plans = rs.randint(0, A, (n, 1, steps))
    exp = PO.oracle_plans(spec, o.st, plans, True, H)
    r = pool.rollout(np.arange(n), plans[:, 0, :], from_envs=True)
    ev = v.evaluate_plans(plans, copy=True)
    for k in REPORTS:
        assert (r[k] == exp[k][:, 0]).all() and (r[k] == ev[k][:, 0]).all(), k
    assert exp['ended'].any() and (exp['length'] < steps).any()
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('cfg', CFG_SOLVED)
def test_reference_recorded_solved_episodes(cfg):
    """The reference's recorded solved episodes as one rollout from their start states, the plans padded with Left to the longest, beside
    as many pairs that only ever turn Left: ret and length are the recorded sums, the kept child is the oracle's terminal state - under
    autoreset too, where it is still the un-reset state -, and restored into an env it continues as the oracle does."""
    spec, st, plans, ret, length = PO.solved_plans(cfg)
    cs = spec.compile()
    nso, steps, A = st.n, plans.shape[2], len(spec.actions_id)
    all_plans = np.concatenate([plans[:, 0, :], np.ones((nso, steps), np.int32)])
    parents = np.concatenate([np.arange(nso), np.arange(nso)])
    for auto in (False, True):
        v = VecNovelGridworld(spec=spec, num_envs=nso, seed=1, autoreset=auto)
        v.reset()
        load_state(v, st)
        st.episode[...] = v.get_state()['episode']              # (an input: the counters the envs happen to hold pass through unchanged)
        pool = v.snapshot(2 * nso)
        e, ends, rep = rollout_checked(v, spec, pool, st, parents, all_plans, np.arange(2 * nso), '%s auto=%d' % (cfg, auto), from_envs=True)
        assert rep['ret'][:nso].tolist() == ret and rep['length'][:nso].tolist() == length and rep['ended'][:nso].all()
        assert (rep['length'] == steps).any() and e.goal[:nso].all() and (ends['inv'][:nso, cs.goal_item] >= 1).all()
        assert (ends['step_count'][:nso] == np.array(length)).all()
        if not auto:                                            # the terminal children back into the envs: the sticky done, step by step
            pool.restore(slots=np.arange(nso))
            o = Oracle(cs, nso)
            o.st = XO.rows_state(spec, ends, np.arange(nso))
            rs = np.random.RandomState(3)
            for t in range(4):
                a = rs.randint(0, A, nso).astype(np.int32)
                o.step(a)
                _, reward, done, _ = v.step(a, copy=True)
                assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
            s = v.get_state()
            for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count'):
                assert (s[k].reshape(getattr(o.st, k).shape) == getattr(o.st, k)).all(), k
        assert v.error_flags() == 0
        v.close()


def _episode_prefixes(cfg, k=0):
    """Recorded solved episode k of cfg: (spec, rows after 0 .. L-1 of its steps - one row each, from the oracle -, its actions up to and
    including the first done)."""
    spec, st, plans, ret, length = PO.solved_plans(cfg)
    L = length[k]
    o = Oracle(spec.compile(), 1)
    o.st = XO.rows_state(spec, {key: getattr(st, key) for key in STATE_KEYS}, [k])
    rows = {key: [] for key in STATE_KEYS}
    for t in range(L):
        for key in STATE_KEYS:
            rows[key].append(getattr(o.st, key)[0].copy())
        o.step(plans[k:k + 1, 0, t].astype(np.int32))
    assert o.done[0]
    return spec, {key: np.stack(x) for key, x in rows.items()}, plans[k, 0, :L]


def test_early_ends_inside_a_wave_and_a_wave_that_leaves_early():
    """A recorded solved episode entered 1 .. 7 steps before its end, the plans padded with Left to T = 7: in one wave pairs end at every
    step 1 .. 7, beside pairs that only turn Left and never end.  And count = 1: the single pair ends at step 2 of 7, so the whole wave
    leaves the loop early."""
    cfg = next(c for c in CFG_SOLVED if c.startswith('pogo') and min(PO.solved_plans(c)[4]) >= 8)
    spec, rows, acts = _episode_prefixes(cfg)
    L, steps = len(acts), 7
    v = VecNovelGridworld(spec=spec, num_envs=L, seed=2)         # env t holds the episode after t of its steps
    v.reset()
    st = XO.rows_state(spec, rows, np.arange(L))
    load_state(v, st)
    src, pool = v.snapshot(L), v.snapshot(200)
    src.save()
    rows['episode'] = v.get_state()['episode'].copy()           # (an input: the counters the envs happen to hold pass through unchanged)
    count = 100
    back = 1 + np.arange(count) % 7                              # steps before the end at which pair j enters the episode
    parents = (L - back).astype(np.int64)
    plans = np.ones((count, steps), np.int32)
    for j in range(count):
        if j % 5 != 4:                                          # (every fifth pair only turns Left)
            plans[j, :back[j]] = acts[L - back[j]:]
    ends, rep, alive = RO.oracle_slot_rollout(spec, rows, parents, plans)
    wave0 = slice(0, 64)
    assert (rep['ended'][wave0] & (rep['length'][wave0] < steps)).any() and (rep['length'][wave0] == steps).any() and (~rep['ended'][wave0]).any()
    assert sorted(set(rep['length'][rep['ended']].tolist())) == list(range(1, 8))
    e = pool.rollout(parents, plans, np.arange(count), source=src)
    RO.assert_reports(e, rep, cfg + ' entered mid-episode')
    RO.assert_rows(pool.state(), ends, cfg + ' entered mid-episode', idx=np.arange(count))
    # count = 1: ends at step 2 of 7
    ends1, rep1, alive1 = RO.oracle_slot_rollout(spec, rows, [L - 2], plans[1:2])
    assert rep1['length'].tolist() == [2] and rep1['ended'].all() and alive1.sum() == 2
    e = pool.rollout([L - 2], plans[1:2], [150], source=src)
    RO.assert_reports(e, rep1, 'count = 1')
    RO.assert_rows(pool.state(), ends1, 'count = 1', idx=[150])
    assert v.error_flags() == 0
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


@pytest.mark.parametrize('auto', [False, True])
def test_firewall_death_mid_plan(auto):
    """fire10h: half of the agents placed beside the fire (they die at their first valid step that FireWall checks), the others walk
    random plans into it: deaths at step 1 and later, message code 14, the child the un-reset state the agent died in."""
    spec = T.build_spec('fire10h')
    cs = spec.compile()
    n, A, steps = 130, len(spec.actions_id), 6
    seed = XO.good_seed(spec, n)
    o = Oracle(cs, n, seed=seed)
    o.reset()
    st = o.st.copy()
    half = st.copy()
    hit = _place_agents(spec, half, cs.fire_item)
    hit = hit[hit % 2 == 0]
    st.loc[hit] = half.loc[hit]
    assert len(hit) > n // 8
    kw = dict(autoreset=True, horizon=40) if auto else {}
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
    v.reset()
    load_state(v, st)
    pool = v.snapshot(3 * n)
    rs = np.random.RandomState(3)
    count = 3 * n
    parents, plans = rs.randint(0, n, count), rs.randint(0, A, (count, steps))
    e, ends, rep = rollout_checked(v, spec, pool, st, parents, plans, np.arange(count), 'fire10h auto=%d' % auto, from_envs=True)
    died = rep['ended'] & (((rep['info'] >> 8) & 255) == 14)
    assert (died & (rep['length'] == 1)).any() and (died & (rep['length'] > 1)).any() and (~rep['ended']).any()
    assert (e.died == died).all() and e.ended[died].all()
    assert (ends['step_count'][died] == rep['length'][died]).all() and (ends['episode'] == st.episode[parents]).all()
    assert v.error_flags() == 0
    v.close()


def test_horizon_cut_mid_plan():
    """Autoreset on, horizon H, the parents' step_count H - 2: a T = 5 plan of Left turns is cut at its second step - length 2, ended, info
    bit 1 clear, the child's step_count H, not reset."""
    spec = T.build_spec('fire10h')
    n, H, steps = 130, 11, 5
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.reset(); o.reset()
    st = o.st.copy()
    st.step_count[...] = H - 2
    load_state(v, st)
    pool = v.snapshot(n)
    e, ends, rep = rollout_checked(v, spec, pool, st, None, np.ones((n, steps), np.int32), np.arange(n), 'horizon', from_envs=True)
    cut = rep['ended'] & (((rep['info'] >> 1) & 1) == 0)
    assert cut.sum() > n // 2 and (rep['length'][cut] == 2).all() and (ends['step_count'][cut] == H).all()
    assert (e.length[cut] == 2).all() and e.ended[cut].all() and not e.goal[cut].any() and (((e.info[cut] >> 1) & 1) == 0).all()
    assert (pool.state()['step_count'][cut] == H).all() and (ends['episode'] == st.episode).all()
    assert v.error_flags() == 0
    v.close()


def _everything(v):
    st = v.get_state()
    reward, done, info = v.get_step_out(copy=True)
    out = {k: st[k].copy() for k in STATE_KEYS}
    out.update(reward=reward, done=done, words=v.action_mask_words(copy=True))
    out.update({'info_' + k: np.asarray(info[k]).copy() for k in ('result', 'step_cost_code', 'message_code', 'message_arg')})
    out.update({'look_' + k: np.asarray(x) for k, x in zip(('reward', 'done', 'result', 'info'), v.lookahead(copy=True))})
    return out


@pytest.mark.parametrize('auto', [False, True])
@pytest.mark.parametrize('cfg', ['pogo10', 'fire10h'])
def test_nothing_is_committed(cfg, auto):
    """Rollouts of every kind leave the state, the last step's outputs, the mask words and the lookahead table byte-identical and CURRENT
    (both device buffers, overwritten through their zero-copy views, read back overwritten: no recompute), the prepared-episode cadence
    as it was, every slot that is no destination identical - in the destination buffer and in a second snapshot -, and the prepared next
    episodes untouched: the next real steps equal the oracle's.  Allowed while terminal capture is on."""
    import torch
    spec = T.build_spec(cfg)
    n, A, H, cap, steps = 130, len(spec.actions_id), 12, 600, 5
    seed = XO.good_seed(spec, n)
    kw = dict(autoreset=True, horizon=H) if auto else {}
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
    o = Oracle(spec.compile(), n, seed=seed, **kw)
    v.reset(); o.reset()
    if auto:
        v.set_terminal_capture(True)                             # no reset runs: allowed under terminal capture
    rs = np.random.RandomState(9)
    for t in range(7):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    pool, other = v.snapshot(cap), v.snapshot(n)
    pool.save(slots=np.arange(n)); other.save()
    before, pool0, other0, cadence = _everything(v), pool.state(), other.state(), v.refill_cadence
    written = []

    def kinds():
        c1 = n + rs.permutation(n)
        rollout_checked(v, spec, pool, o.st, rs.randint(0, n, n), rs.randint(0, A, (n, steps)), c1, cfg + ' from the envs', from_envs=True)
        written.append(c1)
        c2 = 2 * n + np.arange(70)
        dev = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in (rs.randint(0, n, 70), rs.randint(0, A, (steps, 70)), c2)]
        torch.cuda.synchronize()
        pool.rollout(*dev, device=True)                          # slot to slot, device tensors
        written.append(c2)
        c3 = 2 * n + 70 + np.arange(n)
        rollout_checked(v, spec, pool, other.state(), None, rs.randint(0, A, (n, steps)), c3, cfg + ' from a second snapshot', source=other)
        written.append(c3)
        rollout_checked(v, spec, pool, o.st, None, rs.randint(0, A, (n, steps)), None, cfg + ' nothing kept', from_envs=True)
    kinds()
    after = _everything(v)
    for k in before:
        assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), k
    assert v.refill_cadence == cadence
    v.lookahead(device=True)['reward'].fill_(-77)                # both derived buffers poisoned through their zero-copy views
    v.action_mask_words(device=True).fill_(-1)
    torch.cuda.synchronize()
    kinds()
    assert (v.lookahead(copy=True)['reward'] == -77).all(), "a rollout made the lookahead table stale"
    assert (v.action_mask_words(copy=True) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "a rollout made the action masks stale"
    untouched = np.setdiff1d(np.arange(cap), np.concatenate(written))
    assert len(untouched) >= n
    pool1, other1 = pool.state(), other.state()
    for k in STATE_KEYS:
        assert (pool1[k][untouched] == pool0[k][untouched]).all() and (other1[k] == other0[k]).all(), k
    assert v.refill_cadence == cadence
    ends = 0
    for t in range(40):                                         # no prepared episode was consumed: the resets are the oracle's
        a = rs.randint(0, A, n).astype(np.int32)
        assert not o.step(a) & 2
        _, reward, done, _ = v.step(a, copy=True)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
        ends += int(done.sum())
    s = v.get_state()
    for k, ref in zip(STATE_KEYS, (o.st.map, o.st.loc, o.st.facing, o.st.inv, o.st.selected, o.st.step_count, o.st.episode)):
        assert (s[k].reshape(ref.shape) == ref).all(), k
    assert ends >= 2 * n or not auto
    assert v.error_flags() == 0
    v.close()


def _raw(v, src, parents, plans_t, dst, children, count, fill=(77, 55, 9, 0x5A5A5A5A)):
    """The C-ABI call on device tensors with report arrays of known contents.  plans_t: [T, count].  -> {ret, length, ended, info}."""
    import torch
    dev = [None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in (parents, plans_t, children)]
    out = [torch.full((count,), fill[0], dtype=torch.int32, device='cuda'), torch.full((count,), fill[1], dtype=torch.int32, device='cuda'),
           torch.full((count,), fill[2], dtype=torch.uint8, device='cuda'), torch.full((count,), fill[3], dtype=torch.int32, device='cuda')]
    torch.cuda.synchronize()
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    _cabi.check(_cabi.lib().ngw_snapshot_rollout(v._h, None if src is None else src._s, ptr(dev[0]), ptr(dev[1]), count, int(plans_t.shape[0]),
                                                 None if dst is None else dst._s, ptr(dev[2]), count, *[ptr(x) for x in out]))
    v.sync()
    return dict(ret=out[0].cpu().numpy(), length=out[1].cpu().numpy(), ended=out[2].cpu().numpy(), info=out[3].cpu().numpy().view(np.uint32))


def test_bad_indices_from_the_device_skip_their_pairs():
    """Device tensors are range-checked in the kernel before use: one parent and one child out of range among valid pairs raise
    F_BAD_INDEX, their destination slots stay untouched and their report entries at the fill, the neighbouring pairs are correct."""
    spec = T.build_spec('axe10')
    n, A, cap, steps = 70, len(spec.actions_id), 90, 3
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    v.reset()
    pool = v.snapshot(cap)
    pool.save(slots=np.arange(n))
    rows = pool.state()
    rs = np.random.RandomState(8)
    count = 66                                                   # a full wave and a partial one, a bad pair in each
    parents, plans, children = rs.randint(0, n, count), rs.randint(0, A, (count, steps)), rs.permutation(cap)[:count]
    dst = v.snapshot(cap)
    dst.save(slots=np.arange(n))                                 # known contents: a skipped pair must leave them
    dst0 = dst.state()
    bad_parent, bad_child = 5, 65
    parents[bad_parent] = cap                                    # one past the last slot
    children[bad_child] = -3
    assert v.error_flags() == 0
    got = _raw(v, pool, parents, plans.T, dst, children, count, fill=(0, 0, 0, 0))
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    good = np.ones(count, bool)
    good[[bad_parent, bad_child]] = False
    ends, rep, _ = RO.oracle_slot_rollout(spec, rows, parents[good], plans[good])
    for k in REPORTS:
        assert (got[k][good] == rep[k]).all(), k
        assert (got[k][~good] == 0).all(), k                    # the zero fill
    dst1 = dst.state()
    RO.assert_rows(dst1, ends, 'the neighbouring pairs', idx=children[good])
    rest = np.setdiff1d(np.arange(cap), children[good])          # the slot of the pair with the bad parent among them
    assert children[bad_parent] in rest
    for k in STATE_KEYS:
        assert (dst1[k][rest] == dst0[k][rest]).all(), k
    # nothing kept: only the parent index counts, and a skipped pair's reports stay what they were
    got = _raw(v, pool, parents, plans.T, None, None, count)
    assert v.error_flags() == F_BAD_INDEX
    good[bad_child] = True
    _, rep, _ = RO.oracle_slot_rollout(spec, rows, parents[good], plans[good])
    for k in REPORTS:
        assert (got[k][good] == rep[k]).all(), k
    assert (got['ret'][bad_parent], got['length'][bad_parent], got['ended'][bad_parent], got['info'][bad_parent]) == (77, 55, 9, 0x5A5A5A5A)
    v.close()


def test_invalid_action_ids_from_the_device():
    """An id outside the action list at step 0, at a later step, and after the pair has already ended: a no-op step of reward 0 and info 0
    that counts in length - and raises F_INVALID_ACTION only while the pair still runs."""
    cfg = next(c for c in CFG_SOLVED if c.startswith('pogo') and min(PO.solved_plans(c)[4]) >= 8)
    spec, rows, acts = _episode_prefixes(cfg)
    A, L, steps = len(spec.actions_id), len(acts), 5
    v = VecNovelGridworld(spec=spec, num_envs=1, seed=2)
    v.reset()
    v.set_state(0, **{k: rows[k][L - 2:L - 1] for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count')})
    src = v.snapshot(1)
    src.save()
    rows = src.state()
    pool = v.snapshot(70)
    # after the end only: the pair ends at step 2, the bad ids come at steps 3 .. 5
    plans = np.ones((66, steps), np.int32)
    plans[:, :2] = acts[L - 2:]
    plans[:, 2:] = [A, -1, 99]
    ends, rep, _ = RO.oracle_slot_rollout(spec, rows, np.zeros(66, np.int64), plans)
    assert (rep['length'] == 2).all() and rep['ended'].all()
    got = _raw(v, src, np.zeros(66, np.int32), plans.T, pool, np.arange(66), 66)
    for k in REPORTS:
        assert (got[k] == rep[k]).all(), k
    RO.assert_rows(pool.state(), ends, 'bad ids after the end', idx=np.arange(66))
    assert v.error_flags() == 0, "an id outside the list after the pair's end raised a flag"
    # at step 0 (pair 3), at step 1 (pair 64), as the last step (pair 65: info 0); the other pairs as before
    plans[3] = [A, acts[L - 2], acts[L - 1], 1, 1]
    plans[64] = [acts[L - 2], -1, acts[L - 1], 1, 1]
    plans[65] = [1, 1, 1, 1, A + 7]
    ends, rep, _ = RO.oracle_slot_rollout(spec, rows, np.zeros(66, np.int64), plans)
    assert rep['length'][[3, 64, 65]].tolist() == [3, 3, 5] and rep['ended'][[3, 64, 65]].tolist() == [True, True, False]
    assert rep['ret'][3] == rep['ret'][64] == rep['ret'][0] and rep['info'][65] == 0
    got = _raw(v, src, np.zeros(66, np.int32), plans.T, pool, np.arange(66), 66)
    for k in REPORTS:
        assert (got[k] == rep[k]).all(), k
    RO.assert_rows(pool.state(), ends, 'bad ids while running', idx=np.arange(66))
    assert v.error_flags() == F_INVALID_ACTION
    # the host path refuses them before anything launches
    with pytest.raises(ValueError, match='^%d is not in list$' % A):
        pool.rollout(np.zeros(66, np.int64), plans, source=src)
    assert v.error_flags() == 0
    v.close()


def test_one_env_handle_stops_its_resident_loop_first():
    """A one-env handle whose step loop is resident: the rollout ends the loop (it reads HBM, which holds the state only then), the count
    is not bound by the one env, and the env steps on correctly afterwards."""
    spec = T.build_spec('pogo10')
    A, steps, count = len(spec.actions_id), 4, 66
    seed = XO.good_seed(spec, 1)
    v = VecNovelGridworld(spec=spec, num_envs=1, seed=seed)
    o = Oracle(spec.compile(), 1, seed=seed)
    v.reset1(); o.reset()
    rs = np.random.RandomState(2)
    pool = v.snapshot(count)
    for rnd in range(3):
        for t in range(5):
            a = int(rs.randint(0, A))
            out = v.step1(a)
            o.step(np.array([a], np.int32))
            assert out[0] == int(o.reward[0]) and out[1] == bool(o.done[0]), (rnd, t)
        rollout_checked(v, spec, pool, o.st, np.zeros(count, np.int64), rs.randint(0, A, (count, steps)), np.arange(count),
                        'one env, round %d' % rnd, from_envs=True)
    assert v.error_flags() == 0
    v.close()


def test_cabi_errors():
    """Each NGW_E_INVALID_ARG case of include/ngw.h; count == 0 is a no-op; S = 64 is refused like the fused rollout."""
    import torch
    L = _cabi.lib()
    spec = T.build_spec('pogo10')
    n = 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    w = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset(); w.reset()
    s, big, foreign = v.snapshot(8), v.snapshot(100), w.snapshot(8)
    acts = torch.zeros(2 * 128, dtype=torch.int32, device='cuda')
    out = torch.zeros(128, dtype=torch.int32, device='cuda')
    idx = torch.zeros(128, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    a, r, i, E = C.c_void_p(acts.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(idx.data_ptr()), _cabi.E_INVALID_ARG
    X = L.ngw_snapshot_rollout
    err = _cabi.last_error
    assert X(None, None, None, a, 1, 1, s._s, None, 1, r, None, None, None) == E and 'NULL' in err()
    assert X(v._h, None, None, None, 1, 1, s._s, None, 1, r, None, None, None) == E and 'NULL' in err()
    assert X(v._h, None, None, a, 1, 0, s._s, None, 1, r, None, None, None) == E and '0 steps' in err()
    assert X(v._h, None, None, a, 1, -2, s._s, None, 1, r, None, None, None) == E and 'steps' in err()
    assert X(v._h, None, None, a, 3, 2, s._s, None, 4, r, None, None, None) == E and 'pair stride of 3' in err()
    assert X(v._h, None, None, a, 8, 1, s._s, None, -1, r, None, None, None) == E
    assert X(v._h, None, None, a, 8, 1, None, None, 8, None, None, None, None) == E and 'nothing to do' in err()
    assert X(v._h, None, None, a, 8, 1, None, i, 8, r, None, None, None) == E and 'without a destination snapshot' in err()
    assert X(v._h, None, None, a, 8, 1, foreign._s, None, 1, None, None, None, None) == E and 'not an open snapshot' in err()
    assert X(v._h, foreign._s, None, a, 8, 1, s._s, None, 1, None, None, None, None) == E and 'not an open snapshot' in err()
    assert X(v._h, foreign._s, None, a, 8, 1, None, None, 1, r, None, None, None) == E and 'not an open snapshot' in err()
    assert X(v._h, None, None, a, 9, 1, s._s, None, 9, None, None, None, None) == E and '8 slots' in err()        # above dst's capacity
    assert X(v._h, None, None, a, 71, 1, big._s, None, 71, None, None, None, None) == E and '70 envs' in err()    # no list: above n_envs
    assert X(v._h, None, None, a, 71, 1, None, None, 71, r, None, None, None) == E and '70 envs' in err()
    assert X(v._h, s._s, None, a, 9, 1, big._s, None, 9, None, None, None, None) == E and '8 slots' in err()      # ... above src's capacity
    before = s.state()
    assert X(v._h, None, None, a, 0, 1, s._s, None, 0, None, None, None, None) == 0                               # count == 0: a no-op
    assert X(v._h, None, None, a, 8, 2, s._s, None, 8, None, None, None, None) == 0                               # reports may all be NULL with a dst
    assert X(v._h, None, i, a, 128, 2, None, None, 128, r, None, None, None) == 0                                 # a list: count above n_envs, nothing kept
    v.sync()
    after = s.state()
    assert (before['step_count'] == 0).all() and (after['step_count'] == 2).all()
    closed = v.snapshot(4)
    handle = closed._s
    closed.close()
    assert X(v._h, None, None, a, 1, 1, handle, None, 1, None, None, None, None) == E
    assert X(v._h, handle, None, a, 1, 1, None, None, 1, r, None, None, None) == E
    assert v.error_flags() == 0
    v.close(); w.close()
    huge = VecNovelGridworld(spec=make_spec(T.POGO, 64), num_envs=n, seed=4)
    huge.reset()
    hs = huge.snapshot(n)
    with pytest.raises(ValueError, match='64 maps in LDS') as ex:
        hs.rollout(None, np.zeros((n, 3), np.int64), from_envs=True)
    assert 'ngw_snapshot_rollout' in str(ex.value) and 'map_size 64' in str(ex.value)
    hs.save()                                                   # saving and restoring need no LDS
    huge.close()
