"""Snapshot expand on the MI355X (csrc/ngw_expand.inc, include/ngw.h ngw_snapshot_expand, snapshot.py Snapshot.expand), held to the CPU
oracle: the expected child is the parent row stepped by the unmodified oracle with autoreset off, the expected reports are the oracle's
outputs under the handle's autoreset setting (tests/expand_oracle.py) - never the device's own step."""
import ctypes as C

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import plan_oracle as PO
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, F_INVALID_ACTION, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_ALL = sorted(T.CFGS)
CFG_SOLVED = sorted(c for c, v in T.spec_json()['cfgs'].items() if v['n_solved'] > 0)
STATE_KEYS = XO.STATE_KEYS


def load_state(v, st):
    v.set_state(0, map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, selected=st.selected, step_count=st.step_count)


def expand_checked(v, spec, snap, rows, parents, actions, children, where, **kw):
    """One expand held to the oracle: `rows` is a host copy of the source's rows.  Returns (Expansion as numpy, expected children)."""
    count = len(actions)
    p = np.arange(count) if parents is None else np.asarray(parents)
    c = np.arange(count) if children is None else np.asarray(children)
    kids, rep = XO.oracle_expand(spec, rows, p, actions, v.autoreset, v.horizon)
    e = snap.expand(parents, actions, children, **kw)
    XO.assert_reports(e, rep, where)
    XO.assert_rows(snap.state(), kids, where, idx=c)
    return e, kids


@pytest.mark.parametrize('cfg', CFG_ALL)
def test_every_configuration_two_generations(cfg):
    """130 envs (two full waves and a partial one), right after reset and after 60 random steps, autoreset off and on under a horizon of
    25: one random action per env from the envs, then a second generation grown from the children, slot to slot in the same buffer.  The
    first generation's reports are the matching entries of the lookahead table."""
    spec = T.build_spec(cfg)
    n, A = 130, len(spec.actions_id)
    seed = XO.good_seed(spec, n)
    rs = np.random.RandomState(11)
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
            acts = rs.randint(0, A, n)
            e, _ = expand_checked(v, spec, pool, o.st, None, acts, None, where + ' gen 1', from_envs=True)
            look = v.lookahead(copy=True)
            col = (np.arange(n), acts)
            assert (e.reward == look.reward[col]).all() and (e.done == look.done[col]).all() and (e.info == look.info[col]).all(), where
            assert (e.result == look.result[col]).all(), where
            parents = rs.randint(0, n, n)                       # children of generation 1, some of them several times
            expand_checked(v, spec, pool, pool.state(), parents, rs.randint(0, A, n), n + rs.permutation(n), where + ' gen 2')
        assert v.error_flags() == 0
        v.close()


@pytest.mark.parametrize('S', [9, 10, 12, 32])
@pytest.mark.parametrize('count', [1, 63, 65, 200])
def test_map_sizes_and_counts(S, count):
    """One map size per staging form (odd S*S: 9, dwords: 10, 16-byte pieces: 12) and the size that needs the LDS opt-in above 64 KiB
    (32); counts around the wavefront width and far above num_envs = 5, so parents repeat heavily; host lists from the envs, device
    tensors slot to slot with the results left on the device."""
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
    pool = v.snapshot(cap)
    where = 'S=%d count=%d' % (S, count)
    children = rs.permutation(cap)[:count]
    expand_checked(v, spec, pool, o.st, rs.randint(0, n, count), rs.randint(0, A, count), children, where + ' host lists', from_envs=True)
    # device tensors, slot to slot: the parents are the slots just written, the children the free ones
    rows = pool.state()
    free = np.setdiff1d(np.arange(cap), children)
    if len(free) < count:                                       # (count = 200 of 256: the second generation goes to a second buffer)
        dst, free = v.snapshot(cap), np.arange(cap)
    else:
        dst = pool
    parents, acts, kids_at = children[rs.randint(0, count, count)], rs.randint(0, A, count), free[rs.permutation(len(free))[:count]]
    kids, rep = XO.oracle_expand(spec, rows, parents, acts, True, 30)
    dev = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in (parents, acts, kids_at)]
    torch.cuda.synchronize()
    e = dst.expand(dev[0], dev[1], dev[2], source=pool, device=True)
    assert all(isinstance(x, torch.Tensor) and tuple(x.shape) == (count,) for x in e) and e.info.dtype == torch.int32
    assert e.done.dtype == torch.bool and e.reward.dtype == torch.int32
    host = {k: e[k].cpu().numpy() for k in ('reward', 'done', 'result', 'info')}
    XO.assert_reports(host, rep, where + ' device tensors')
    assert (e.goal.cpu().numpy() == (rep['done'] & ((rep['info'] >> 1) & 1).astype(bool))).all()
    XO.assert_rows(dst.state(), kids, where + ' device tensors', idx=kids_at)
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


@pytest.mark.parametrize('cfg', ['pogo10', 'fire10h'])
def test_nothing_is_committed(cfg):
    """Expands of every kind leave the state, the last step's outputs, the mask words and the lookahead table byte-identical and CURRENT
    (both device buffers, overwritten through their zero-copy views, read back overwritten: no recompute), every slot that is no
    destination identical - in the destination buffer and in a second snapshot -, and the prepared next episodes untouched: the next 40
    real steps under autoreset equal the oracle's.  Allowed while terminal capture is on."""
    import torch
    spec = T.build_spec(cfg)
    n, A, H, cap = 130, len(spec.actions_id), 12, 600
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.reset(); o.reset()
    rs = np.random.RandomState(9)
    for t in range(7):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    pool, other = v.snapshot(cap), v.snapshot(n)
    pool.save(slots=np.arange(n)); other.save()
    before, pool0, other0 = _everything(v), pool.state(), other.state()
    written = []

    def kinds():
        c1 = n + rs.permutation(n)
        e, _ = expand_checked(v, spec, pool, o.st, rs.randint(0, n, n), rs.randint(0, A, n), c1, cfg + ' from the envs', from_envs=True)
        written.append(c1)
        c2 = 2 * n + np.arange(70)
        dev = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in (rs.randint(0, n, 70), rs.randint(0, A, 70), c2)]
        torch.cuda.synchronize()
        pool.expand(*dev, device=True)                           # slot to slot, device tensors
        written.append(c2)
        c3 = 2 * n + 70 + np.arange(n)
        expand_checked(v, spec, pool, other.state(), None, rs.randint(0, A, n), c3, cfg + ' from a second snapshot', source=other)
        written.append(c3)
        t = pool.expand_all([3, 77], 3 * n + 70)
        written.append(3 * n + 70 + np.arange(2 * A))
        return e, t
    e, t = kinds()
    assert t.reward.shape == (2, A)
    after = _everything(v)
    for k in before:
        assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), k
    v.lookahead(device=True)['reward'].fill_(-77)                # both derived buffers poisoned through their zero-copy views
    v.action_mask_words(device=True).fill_(-1)
    torch.cuda.synchronize()
    kinds()
    assert (v.lookahead(copy=True)['reward'] == -77).all(), "an expand made the lookahead table stale"
    assert (v.action_mask_words(copy=True) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "an expand made the action masks stale"
    untouched = np.setdiff1d(np.arange(cap), np.concatenate(written))
    assert len(untouched) >= n
    pool1, other1 = pool.state(), other.state()
    for k in STATE_KEYS:
        assert (pool1[k][untouched] == pool0[k][untouched]).all() and (other1[k] == other0[k]).all(), k
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
    assert ends >= 2 * n
    v.set_terminal_capture(True)                                 # no reset runs: allowed under terminal capture
    expand_checked(v, spec, pool, o.st, None, rs.randint(0, A, n), None, cfg + ' under terminal capture', from_envs=True)
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('cfg', CFG_SOLVED)
def test_reference_recorded_solved_episodes_as_chains_of_expands(cfg):
    """The reference's recorded solved episodes walked as a chain of expands, one node per step, ping-pong between the two halves of one
    pool: `done` first appears at the recorded step with reward_done, the terminal child holds the goal item - under autoreset too, where
    it is still the un-reset state -, and the chain's return and length up to its first done are evaluate_plans' for the same plan."""
    spec, st, plans, ret, length = PO.solved_plans(cfg)
    cs = spec.compile()
    nso, steps = st.n, plans.shape[2]
    for auto in (False, True):
        v = VecNovelGridworld(spec=spec, num_envs=nso, seed=1, autoreset=auto)
        v.reset()
        load_state(v, st)
        ev = v.evaluate_plans(plans, copy=True)
        pool = v.snapshot(2 * nso)
        total, first = np.zeros(nso, np.int64), np.full(nso, -1)
        for t in range(steps):
            src, dst = ((t + 1) % 2) * nso + np.arange(nso), (t % 2) * nso + np.arange(nso)
            e = pool.expand(None if t == 0 else src, plans[:, 0, t], dst, from_envs=(t == 0))
            running = first < 0
            total[running] += e.reward[running]
            ended_now = running & e.done
            if ended_now.any():
                kids = pool.state(int(dst[0]), nso)
                assert (e.reward[ended_now] == cs.reward_done).all() and e.goal[ended_now].all(), (cfg, auto, t)
                assert (kids['inv'][ended_now, cs.goal_item] >= 1).all(), "the terminal child does not hold the goal item"
                assert (kids['step_count'][ended_now] == t + 1).all() and (kids['episode'][ended_now] == v.get_state()['episode'][ended_now]).all()
                first[ended_now] = t
            if (first >= 0).all():
                break
        assert (first + 1).tolist() == length and total.tolist() == ret, (cfg, auto)
        assert ev.ret[:, 0].tolist() == total.tolist() and ev.length[:, 0].tolist() == (first + 1).tolist()
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
def test_firewall_death_leaves_the_state_it_died_in(auto):
    """fire10h with agents placed beside the fire: the step dies with message code 14, and the child is the un-reset state."""
    spec = T.build_spec('fire10h')
    cs = spec.compile()
    n, A = 130, len(spec.actions_id)
    seed = XO.good_seed(spec, n)
    o = Oracle(cs, n, seed=seed)
    o.reset()
    st = o.st.copy()
    hit = _place_agents(spec, st, cs.fire_item)
    assert len(hit) > n // 4
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=auto)
    v.reset()
    load_state(v, st)
    pool = v.snapshot(2 * n)
    rs = np.random.RandomState(3)
    e, kids = expand_checked(v, spec, pool, st, None, rs.randint(0, A, n), None, 'fire10h beside the fire', from_envs=True)
    died = e.died
    assert died[hit].any() and (((e.info[died] >> 8) & 255) == 14).all() and e.done[died].all()
    assert (e.reward[died] == cs.fire_reward).all()
    assert (kids['step_count'][died] == 1).all() and (kids['episode'] == st.episode).all()
    expand_checked(v, spec, pool, pool.state(), np.arange(n), rs.randint(0, A, n), n + np.arange(n), 'fire10h, the next generation')
    v.close()


def test_horizon_cut_sets_done_and_leaves_the_goal_bit_clear():
    spec = T.build_spec('pogo10')
    n, H = 130, 11
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.reset(); o.reset()
    st = o.st.copy()
    k = 1 + np.arange(n) % 3
    st.step_count[...] = H - k
    load_state(v, st)
    pool = v.snapshot(n)
    e, kids = expand_checked(v, spec, pool, st, None, np.ones(n, np.int32), None, 'horizon', from_envs=True)   # Left: reaches no goal
    assert (e.done == (k == 1)).all() and not ((e.info >> 1) & 1).any() and not e.goal.any()
    assert (kids['step_count'] == H - k + 1).all() and (kids['episode'] == st.episode).all()      # (the cut child is not reset)
    v.close()


def test_a_child_restored_into_an_env_continues_as_the_oracle_does():
    spec = T.build_spec('axe10')
    n, A, H = 130, len(spec.actions_id), 15
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.reset(); o.reset()
    rs = np.random.RandomState(5)
    for t in range(9):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    pool = v.snapshot(n)
    parents = rs.randint(0, n, n)
    e, kids = expand_checked(v, spec, pool, o.st, parents, rs.randint(0, A, n), None, 'round trip', from_envs=True)
    keep = ~e.done                                              # (an ended node is not stepped on: restoring it is the caller's business)
    envs = np.nonzero(keep)[0]
    pool.restore(slots=envs, envs=envs)
    for k_ in STATE_KEYS:
        getattr(o.st, k_)[envs] = kids[k_][envs]
    for t in range(30):
        a = rs.randint(0, A, n).astype(np.int32)
        assert not o.step(a) & 2
        _, reward, done, _ = v.step(a, copy=True)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
    s = v.get_state()
    for k_, ref in zip(STATE_KEYS, (o.st.map, o.st.loc, o.st.facing, o.st.inv, o.st.selected, o.st.step_count, o.st.episode)):
        assert (s[k_].reshape(ref.shape) == ref).all(), k_
    assert v.error_flags() == 0
    v.close()


def test_bad_indices_from_the_device_skip_their_pairs():
    """Device tensors are range-checked in the kernel before use: one parent and one child out of range among valid pairs raise
    F_BAD_INDEX, their destination slots and report entries stay untouched, the neighbouring pairs are correct."""
    import torch
    spec = T.build_spec('axe10')
    n, A, cap = 70, len(spec.actions_id), 90
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    o = Oracle(spec.compile(), n, seed=seed)
    v.reset(); o.reset()
    pool = v.snapshot(cap)
    pool.save(slots=np.arange(n))
    rows = pool.state()
    rs = np.random.RandomState(8)
    count = 66                                                   # a full wave and a partial one, a bad pair in each
    parents, acts, children = rs.randint(0, n, count), rs.randint(0, A, count), rs.permutation(cap)[:count]
    dst = v.snapshot(cap)
    dst.save(slots=np.arange(n))                                 # known contents: a skipped pair must leave them
    dst0 = dst.state()
    bad_parent, bad_child = 5, 65
    parents[bad_parent] = cap                                    # one past the last slot
    children[bad_child] = -3
    dev = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in (parents, acts, children)]
    reward = torch.full((count,), 77, dtype=torch.int32, device='cuda')
    done = torch.full((count,), 9, dtype=torch.uint8, device='cuda')
    info = torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    assert v.error_flags() == 0
    _cabi.check(_cabi.lib().ngw_snapshot_expand(v._h, pool._s, dev[0].data_ptr(), dev[1].data_ptr(), dst._s, dev[2].data_ptr(), count,
                                                reward.data_ptr(), done.data_ptr(), info.data_ptr()))
    v.sync()
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    good = np.ones(count, bool)
    good[[bad_parent, bad_child]] = False
    kids, rep = XO.oracle_expand(spec, rows, parents[good], acts[good], False, 0)
    got = dict(reward=reward.cpu().numpy(), done=done.cpu().numpy(), info=info.cpu().numpy().view(np.uint32))
    for k in ('reward', 'done', 'info'):
        assert (got[k][good] == rep[k]).all(), k
    assert got['reward'][~good].tolist() == [77, 77] and got['done'][~good].tolist() == [9, 9] and (got['info'][~good] == 0x5A5A5A5A).all()
    dst1 = dst.state()
    XO.assert_rows(dst1, kids, 'the neighbouring pairs', idx=children[good])
    rest = np.setdiff1d(np.arange(cap), children[good])          # the slot of the pair with the bad parent among them
    assert children[bad_parent] in rest
    for k in STATE_KEYS:
        assert (dst1[k][rest] == dst0[k][rest]).all(), k
    v.close()


def test_an_invalid_action_id_from_the_device_copies_the_parent():
    import torch
    spec = T.build_spec('axe10')
    n, A = 70, len(spec.actions_id)
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    o = Oracle(spec.compile(), n, seed=seed)
    v.reset(); o.reset()
    pool = v.snapshot(2 * n)
    rs = np.random.RandomState(4)
    acts = rs.randint(0, A, n)
    acts[[3, 64]] = A, -1
    kids, rep = XO.oracle_expand(spec, o.st, np.arange(n), acts, False, 0)
    dev = torch.from_numpy(np.ascontiguousarray(acts, np.int32)).cuda()
    torch.cuda.synchronize()
    e = pool.expand(None, dev, None, from_envs=True)
    XO.assert_reports(e, rep, 'invalid ids')
    got = pool.state()
    XO.assert_rows(got, kids, 'invalid ids', idx=np.arange(n))
    for i in (3, 64):
        assert e.reward[i] == 0 and e.info[i] == 0 and not e.done[i]
        assert (got['map'][i] == o.st.map[i]).all() and got['step_count'][i] == o.st.step_count[i] and (got['inv'][i] == o.st.inv[i]).all()
    assert v.error_flags() == F_INVALID_ACTION
    v.close()


def test_one_env_handle_stops_its_resident_loop_first():
    """A one-env handle whose step loop is resident: the expand ends the loop (it reads HBM, which holds the state only then), the count
    is not bound by the one env, and the env steps on correctly afterwards."""
    spec = T.build_spec('pogo10')
    A = len(spec.actions_id)
    seed = XO.good_seed(spec, 1)
    v = VecNovelGridworld(spec=spec, num_envs=1, seed=seed)
    o = Oracle(spec.compile(), 1, seed=seed)
    v.reset1(); o.reset()
    rs = np.random.RandomState(2)
    pool = v.snapshot(A)
    for rnd in range(3):
        for t in range(5):
            a = int(rs.randint(0, A))
            out = v.step1(a)
            o.step(np.array([a], np.int32))
            assert out[0] == int(o.reward[0]) and out[1] == bool(o.done[0]), (rnd, t)
        kids, rep = XO.oracle_expand(spec, o.st, np.zeros(A, np.int64), np.arange(A), False, 0)
        e = pool.expand_all([0], 0, from_envs=True)
        XO.assert_reports(e.reshape(A), rep, 'one env, round %d' % rnd)
        XO.assert_rows(pool.state(), kids, 'one env, round %d' % rnd)
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
    acts = torch.zeros(128, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    a, E = C.c_void_p(acts.data_ptr()), _cabi.E_INVALID_ARG
    X = L.ngw_snapshot_expand
    assert X(None, None, None, a, s._s, None, 1, None, None, None) == E and 'NULL' in _cabi.last_error()
    assert X(v._h, None, None, a, None, None, 1, None, None, None) == E and 'NULL' in _cabi.last_error()
    assert X(v._h, None, None, None, s._s, None, 1, None, None, None) == E and 'NULL' in _cabi.last_error()
    assert X(v._h, None, None, a, foreign._s, None, 1, None, None, None) == E and 'not an open snapshot' in _cabi.last_error()
    assert X(v._h, foreign._s, None, a, s._s, None, 1, None, None, None) == E and 'not an open snapshot' in _cabi.last_error()
    assert X(v._h, None, None, a, s._s, None, -1, None, None, None) == E and X(v._h, None, None, a, s._s, None, 9, None, None, None) == E
    assert 'slots' in _cabi.last_error()
    assert X(v._h, None, None, a, big._s, None, 71, None, None, None) == E and '70 envs' in _cabi.last_error()      # no list: above n_envs
    assert X(v._h, s._s, None, a, big._s, None, 9, None, None, None) == E and '8 slots' in _cabi.last_error()       # ... above src's capacity
    before = s.state()
    assert X(v._h, None, None, a, s._s, None, 0, None, None, None) == 0
    assert X(v._h, None, None, a, s._s, None, 8, None, None, None) == 0                                             # reports may all be NULL
    v.sync()
    after = s.state()
    assert (before['step_count'] == 0).all() and (after['step_count'] == 1).all()
    closed = v.snapshot(4)
    handle = closed._s
    closed.close()
    assert X(v._h, None, None, a, handle, None, 1, None, None, None) == E
    assert v.error_flags() == 0
    v.close(); w.close()
    huge = VecNovelGridworld(spec=make_spec(T.POGO, 64), num_envs=n, seed=4)
    huge.reset()
    hs = huge.snapshot(n)
    with pytest.raises(ValueError, match='64 maps in LDS') as ex:
        hs.expand(None, np.zeros(n, np.int64), None, from_envs=True)
    assert 'ngw_snapshot_expand' in str(ex.value) and 'map_size 64' in str(ex.value)
    hs.save()                                                   # saving and restoring need no LDS
    huge.close()
