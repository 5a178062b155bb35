"""One-step lookahead tables on the MI355X (csrc/ngw_lookahead.inc, include/ngw.h ngw_lookahead ...), held to the CPU oracle: the expected
table of a state is what the unmodified oracle reports when each action is stepped from a copy of it (tests/lookahead_oracle.py)."""
import ctypes as C

import numpy as np
import pytest

import lookahead_oracle as LO
import mask_oracle as M
import ngw_testlib as T
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.spec import make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_G4 = sorted(T.spec_json()['cfgs'])
CFG_ALL = sorted(T.CFGS)
STATE_KEYS = ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode')


def load_state(v, st):
    v.set_state(0, map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, selected=st.selected, step_count=st.step_count)


def oracle_state(spec, v):
    s = v.get_state()
    st = M.state_from(spec, s['map'], s['loc'], s['facing'], s['inv'], s['selected'], step_count=s['step_count'])
    st.episode[...] = s['episode']
    return st


def check(v, spec, st, where):
    exp = LO.oracle_lookahead(spec, st, autoreset=v.autoreset, horizon=v.horizon)
    got = v.lookahead(copy=True)
    LO.assert_table(got, exp, where)
    assert (got['result'] == v.action_masks()).all(), where + ": bit 0 of info is not the action mask"
    return got


def good_seed(spec, n, lo=4):
    return next(sd for sd in range(lo, lo + 40) if not Oracle(spec.compile(), n, seed=sd).reset() & 2)   # (tight maps can exhaust the placement)


@pytest.mark.parametrize('cfg', CFG_G4)
def test_injected_reference_states(cfg):
    """The injected G4 states (every action x front block x inventory profile) of every fixture configuration: the whole table is the
    oracle's, the entry of the recorded action is the reference's recorded outcome; then with autoreset on and step_count injected one
    step below the horizon for every third env, and with a goal item in the inventory of every fourth (sticky done, autoreset off)."""
    g = T.golden(cfg)
    spec = T.build_spec(cfg)
    st = M.state_from(spec, g['ss_pre_map'], g['ss_pre_loc'], g['ss_pre_facing'], g['ss_pre_inv'], g['ss_pre_sel'])
    n = st.n
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    load_state(v, st)
    got = check(v, spec, st, cfg + ' G4')
    rows, act = np.arange(n), g['ss_action'].astype(np.int64)
    assert (got['reward'][rows, act] == g['ss_reward']).all() and (got['done'][rows, act] == g['ss_done'].astype(bool)).all()
    assert (got['result'][rows, act] == g['ss_result'].astype(bool)).all()
    # sticky done, autoreset off: every action of an env that holds a goal item reports done with the forced reward
    cs = spec.compile()
    st2 = st.copy()
    st2.inv[0::4, cs.goal_item] = 1
    load_state(v, st2)
    got = check(v, spec, st2, cfg + ' G4 sticky done')
    died = ((got['info'][0::4] >> 8) & 255) == 14             # (FireWall's death runs after the goal test and overwrites its reward)
    assert got['done'][0::4].all() and (got['reward'][0::4][~died] == cs.reward_done).all()
    assert cs.fire_item or not died.any()
    v.close()
    # autoreset on, a third of the batch one step below the horizon
    H = 9
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1, autoreset=True, horizon=H)
    st.step_count[...] = np.where(np.arange(n) % 3 == 0, H - 1, np.arange(n) % 5)
    load_state(v, st)
    got = check(v, spec, st, cfg + ' G4 horizon')
    assert got['done'][0::3].all()
    assert (((got['info'][0::3] >> 1) & 1).astype(bool) <= got['done'][0::3]).all()
    v.close()


@pytest.mark.parametrize('cfg', CFG_ALL)
def test_after_reset_and_along_random_play(cfg):
    """Every test configuration (plain, the LUT novelties, the EXT stacks, v0): right after reset and after a few hundred random steps,
    515 envs (a partial last wave), autoreset on with a horizon and off."""
    spec = T.build_spec(cfg)
    n, A = 515, len(spec.actions_id)
    seed = good_seed(spec, n)
    for auto in (True, False):
        kw = dict(autoreset=True, horizon=25) if auto else {}
        v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
        o = Oracle(spec.compile(), n, seed=seed, **kw)
        v.reset(); o.reset()
        check(v, spec, o.st, '%s after reset auto=%d' % (cfg, auto))
        rs = np.random.RandomState(5)
        for t in range(240 if auto else 120):
            a = rs.randint(0, A, n).astype(np.int32)
            if o.step(a) & 2:                                   # a tight map exhausted the placement of an autoreset: stop here
                break
            v.step(a)
            if t % 60 == 59:
                check(v, spec, o.st, '%s random play t=%d auto=%d' % (cfg, t, auto))
        v.close()


@pytest.mark.parametrize('S', [9, 10, 20, 32, 64])
@pytest.mark.parametrize('n', [1, 63, 65, 1000, 4099])
def test_map_and_batch_sizes(S, n):
    """Odd and even map sizes up to 64 x 64, batch sizes around the wavefront width and with a partial last wave."""
    if S == 64 and n == 4099:
        n = 2049
    spec = make_spec(T.POGO, S)
    A = len(spec.actions_id)
    seed = good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=30)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=30)
    v.reset(); o.reset()
    check(v, spec, o.st, 'S=%d n=%d after reset' % (S, n))
    rs = np.random.RandomState(S + n)
    for t in range(70):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    check(v, spec, o.st, 'S=%d n=%d after 70 steps' % (S, n))
    dev = v.lookahead(device=True)
    host = v.lookahead()
    for k in ('reward', 'done', 'result'):
        assert tuple(dev[k].shape) == (n, A) and (dev[k].cpu().numpy() == host[k]).all(), k
    assert (dev['info'].cpu().numpy().view(np.uint32) == host['info']).all()
    v.close()


def _place_agents(spec, st, want, facing_to):
    """Moves each env's agent onto an air cell with a 4-neighbour holding item `want` (facing it when facing_to, else keeping the facing);
    returns the envs where one was found."""
    S = spec.map_size
    hit = []
    D = [(-1, 0, 0), (1, 0, 1), (0, -1, 2), (0, 1, 3)]                 # NORTH SOUTH WEST EAST
    for i in range(st.n):
        m = st.map[i].reshape(S, S)
        done = False
        for r in range(1, S - 1):
            for c in range(1, S - 1):
                if m[r, c] != 0 or done:
                    continue
                for dr, dc, f in D:
                    if m[r + dr, c + dc] == want:
                        st.loc[i] = (r, c)
                        if facing_to:
                            st.facing[i] = f
                        hit.append(i); done = True
                        break
    return np.array(hit, np.int64)


def test_firewall_beside_the_fire_crate_in_front_and_an_entity_picked_up():
    """FireWall hard with agents moved beside the fire (death entries: reward, done, message), a crate in front (Break hands out the
    ingredients first - the goal test sees them), and an env whose Forward picks up an entity that changes its inventory."""
    n = 300
    # FireWall hard: agents beside the fire, and agents one Forward away from it
    spec = T.build_spec('fire10h')
    cs = spec.compile()
    seed = good_seed(spec, n)
    o = Oracle(cs, n, seed=seed)
    o.reset()
    st = o.st.copy()
    hit = _place_agents(spec, st, cs.fire_item, facing_to=False)
    assert len(hit) > n // 4
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    v.reset()
    load_state(v, st)
    got = check(v, spec, st, 'fire10h beside the fire')
    msg = (got['info'][hit] >> 8) & 255
    assert (msg == 14).any() and got['done'][hit].any() and (got['reward'][hit][msg == 14] == cs.fire_reward).all()
    v.close()
    # Crate in front; with the goal recipe's ingredients in the crate a Break can finish the episode
    for cfg in ('crate12h', 'stk_crate_fr12', 'stk_fr_crate12'):
        spec = T.build_spec(cfg)
        cs = spec.compile()
        seed = good_seed(spec, n)
        o = Oracle(cs, n, seed=seed)
        o.reset()
        st = o.st.copy()
        hit = _place_agents(spec, st, cs.crate_item, facing_to=True)
        assert len(hit) > n // 4, cfg
        v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=40)
        v.reset()
        load_state(v, st)
        check(v, spec, st, cfg + ' crate in front')
        v.close()
    # an entity two cells ahead (and one diagonally ahead): Forward moves next to it and picks it up; as the goal item it ends the episode
    spec = T.build_spec('axe10')
    cs = spec.compile()
    ent = [i for i in range(cs.n_items) if cs.entity[i]]
    assert ent
    seed = good_seed(spec, n)
    o = Oracle(cs, n, seed=seed)
    o.reset()
    st = o.st.copy()
    S = spec.map_size
    put = 0
    for i in range(n):
        m = st.map[i].reshape(S, S)
        r, c = st.loc[i]
        dr, dc = [(-1, 0), (1, 0), (0, -1), (0, 1)][st.facing[i]]
        r1, c1, r2, c2 = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        if 0 < r2 < S - 1 and 0 < c2 < S - 1 and m[r1, c1] == 0:
            m[r2, c2] = ent[i % len(ent)] if i % 2 else cs.goal_item
            put += 1
    assert put > n // 4
    import copy
    spec_goal = copy.deepcopy(spec)
    spec_goal.entities.add(spec.item_names[cs.goal_item])               # (the goal item lying on the map as an entity: the pick-up feeds the goal test)
    for sp, name in ((spec, 'entity'), (spec_goal, 'goal entity')):
        v = VecNovelGridworld(spec=sp, num_envs=n, seed=seed)
        v.reset()
        load_state(v, st)
        got = check(v, sp, st, 'axe10 Forward picks up an ' + name)
        if sp is spec_goal:
            assert got['done'][:, sp.actions_id['Forward']].any()
        v.close()


def _snapshot_of_everything(v, lidar):
    st = v.get_state()
    reward, done, info = v.get_step_out(copy=True)
    out = {k: st[k].copy() for k in STATE_KEYS}
    out.update(reward=reward, done=done, words=v.action_mask_words(copy=True))
    out.update({'info_' + k: np.asarray(info[k]).copy() for k in ('result', 'step_cost_code', 'message_code', 'message_arg')})
    if lidar:
        rows = v.lidar_observation(copy=True)
        out['lidar'] = np.concatenate([np.asarray(x).reshape(len(st['loc']), -1) for x in rows], 1) if isinstance(rows, tuple) else np.asarray(rows).copy()
    return out


@pytest.mark.parametrize('cfg,lidar', [('pogo10', False), ('pogo10', True), ('fire10h', False), ('stk_fr_crate12', False), ('add32', False)])
def test_lookahead_commits_nothing(cfg, lidar):
    """State of all envs, the last step's outputs, the mask words and (fused lidar on) the lidar rows are byte-equal before and after the
    call - including entries that end an episode; then the env follows the oracle as if the lookahead had never run, through episode
    ends, so the prepared next episodes are shown unconsumed."""
    spec = T.build_spec(cfg)
    n, A, H = 1100, len(spec.actions_id), 12
    seed = good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    if lidar:
        v.lidar_configure(num_beams=8, fused=True)
    v.set_action_masks(True)
    v.reset(); o.reset()
    rs = np.random.RandomState(9)
    ends = 0
    for t in range(3 * H + 5):
        before = _snapshot_of_everything(v, lidar)
        tab = v.lookahead(copy=True)
        after = _snapshot_of_everything(v, lidar)
        for k in before:
            assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), (t, k)
        last = before['step_count'] >= H - 1
        assert tab['done'][last].all(), "one step below the horizon every entry ends the episode"
        a = rs.randint(0, A, n).astype(np.int32)
        assert not o.step(a) & 2
        _, reward, done, info = v.step(a, copy=True)
        rows = np.arange(n)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
        assert (tab['reward'][rows, a] == reward).all() and (tab['done'][rows, a] == done).all(), t
        assert (tab['result'][rows, a] == info['result']).all(), t
        ends += int(done.sum())
        s = v.get_state()
        for k, ref in zip(STATE_KEYS, (o.st.map, o.st.loc, o.st.facing, o.st.inv, o.st.selected, o.st.step_count, o.st.episode)):
            assert (s[k].reshape(ref.shape) == ref).all(), (t, k)
    assert ends >= 2 * n and v.error_flags() == 0
    v.close()


def _poison(v):
    """Overwrites the device table through the zero-copy views: a later query that launches nothing hands the poison back."""
    import torch
    d = v.lookahead(device=True)
    d['reward'].fill_(-77)
    torch.cuda.synchronize()


def _is_poisoned(v):
    return bool((v.lookahead(copy=True)['reward'] == -77).all())


def test_staleness_follows_every_state_changing_call():
    """After each state-changing call the next lookahead describes the new state; a second query without a change launches nothing (the
    device table, overwritten through its zero-copy view in between, comes back as it was left)."""
    import torch
    spec = T.build_spec('axe10')
    n, A, H = 700, len(spec.actions_id), 20
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=8, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=8, autoreset=True, horizon=H)
    v.reset(); o.reset()
    rs = np.random.RandomState(1)

    def fresh(where):
        check(v, spec, o.st, where)                            # recomputed: describes the new state
        _poison(v)
        assert _is_poisoned(v), where + ": a query on a current table launched the kernel"
        assert _is_poisoned(v)

    fresh('after reset')
    act = rs.randint(0, A, n).astype(np.int32)
    v.step(act); o.step(act)                                    # host step
    fresh('after a host step')
    ad = torch.from_numpy(rs.randint(0, A, (6, n)).astype(np.int32)).cuda()
    torch.cuda.synchronize()
    v.step_device(ad[0].data_ptr()); o.step(ad[0].cpu().numpy())
    fresh('after step_device')
    m = (rs.rand(n) < 0.4).astype(np.uint8)
    v.reset(m); o.reset(m)
    fresh('after a masked reset')
    inv = rs.randint(0, 4, (n, len(spec.items_id))).astype(np.int32)
    v.set_state(0, inv=inv); o.st.inv[...] = inv
    fresh('after set_state')
    snap = v.snapshot()
    snap.save()
    saved = o.st.copy()
    act = rs.randint(0, A, n).astype(np.int32)
    v.step(act); o.step(act)
    fresh('after a step behind the save')
    snap.restore()
    o.st = saved.copy()
    fresh('after a snapshot restore')
    src = rs.randint(0, n, n).astype(np.int32)
    v.fork(src, keep_episode=True)
    ep = o.st.episode.copy()
    for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count'):
        getattr(o.st, k)[...] = getattr(saved, k)[src]
    o.st.episode[...] = ep
    fresh('after a fork')
    v.rollout(13, action_seed=5); o.rollout(13, 5, 0)
    fresh('after a rollout')
    v.graph_build(ad.data_ptr(), n, 6)
    v.graph_launch(2)
    for rep in range(2):
        for t in range(6):
            o.step(ad[t].cpu().numpy())
    fresh('after a graph replay')
    v.set_autoreset(False)                                      # the setting changes what a step reports, not the state
    o.autoreset, o.horizon = 0, 0
    check(v, spec, o.st, 'after set_autoreset')
    # rebuild (inject_novelty): the buffers belong to the handle
    import copy
    from gym_novel_gridworlds_amd.novelty import apply_novelty
    spec2 = copy.deepcopy(v.spec)
    apply_novelty(spec2, 'axetobreak', 'hard', 'wooden', '')
    v.rebuild(spec2)
    v.reset()
    st = oracle_state(spec2, v)
    got = check(v, spec2, st, 'after rebuild')
    assert got['reward'].shape == (n, len(spec2.actions_id))
    assert v.error_flags() == 0
    v.close()


def _adapter_oracle_table(env):
    base = env
    while hasattr(base, 'env') and not hasattr(base, '_backend'):
        base = base.env
    spec = base._sync_spec()
    s = base._backend().get_state()
    st = M.state_from(spec, s['map'], s['loc'], s['facing'], s['inv'], s['selected'], step_count=s['step_count'])
    return LO.oracle_lookahead(spec, st)


@pytest.mark.parametrize('solo', ['1', '0'])
def test_single_env_adapter(solo, monkeypatch):
    """The adapter's lookahead() is the oracle's table of its state, bare and wrapped in LimitActions, in the reference's loop shape
    (the state read back before every step, a reset when an episode ends).  Then a tight lookahead() + step() loop with no call in between
    that ends the resident step loop, the expected tables taken from a CPU oracle stepped alongside (never from get_state): with the
    resident loop (solo = 1) every table equals the oracle's while the loop's start count rises by no more than its own idle-limit
    endings, so the answers came from the loop's speculated records and the loop kept running; NGW_SOLO=0: the kernel path gives the same
    values and no loop is ever started."""
    import gym_novel_gridworlds_amd as G
    from oracle.ngw_oracle import Oracle
    monkeypatch.setenv('NGW_SOLO', solo)
    L = _cabi.lib()
    L.ngw_debug_solo_starts.restype = C.c_longlong
    L.ngw_debug_solo_starts.argtypes = [C.c_void_p]
    np.random.seed(0)
    env = G.make('NovelGridworld-Pogostick-v1')
    env.reset()
    rs = np.random.RandomState(4)
    for i in range(40):
        t = env.lookahead()
        exp = _adapter_oracle_table(env)
        for k in ('reward', 'done', 'result', 'info'):
            assert t[k].shape == exp[k][0].shape and (t[k] == exp[k][0]).all(), (i, k)
        a = int(rs.randint(0, len(t.reward)))
        _, r, d, info = env.step(a)
        assert (r, d, info['result']) == (int(t.reward[a]), bool(t.done[a]), bool(t.result[a])), i
        if d:
            env.reset()
    # the tight loop: the oracle starts from the adapter's state once and is stepped alongside from there
    env.reset()
    vec = env._backend()
    spec = env._sync_spec()
    s = vec.get_state()
    o = Oracle(spec.compile(), 1, autoreset=False, horizon=0)
    o.st = M.state_from(spec, s['map'], s['loc'], s['facing'], s['inv'], s['selected'], step_count=s['step_count'])
    # (the oracle runs ahead: the actions do not depend on what the device answers, and host work between two steps of the tight loop
    # would only let the resident loop run into its idle limit)
    A = len(spec.actions_id)
    acts = rs.randint(0, A, 200)
    exps, outs = [], []
    for a in acts:
        exps.append(LO.oracle_lookahead(spec, o.st))
        o.step(np.array([a], np.int32))
        outs.append((int(o.reward[0]), bool(o.done[0]), bool(o.result[0])))
    starts, got, stepped = None, [], []
    for i in range(200):
        got.append(env.lookahead(copy=True))
        _, r, d, info = env.step(int(acts[i]))
        stepped.append((r, d, info['result']))
        if i == 5:
            starts = L.ngw_debug_solo_starts(vec._h)
    ends = L.ngw_debug_solo_starts(vec._h)
    for i in range(200):
        for k in ('reward', 'done', 'result', 'info'):
            assert got[i][k].shape == exps[i][k][0].shape and (got[i][k] == exps[i][k][0]).all(), (i, k)
        assert stepped[i] == outs[i], i
    assert env._backend() is vec
    if solo == '1':
        assert starts >= 1, "the resident loop never ran"
        assert ends - starts <= 2, "lookahead() ended the resident loop"   # (only the loop's own idle-limit endings may restart it)
    else:
        assert ends == 0
    limited = {'Forward', 'Left', 'Right', 'Break', 'Craft_plank', 'Craft_stick'}
    w = G.LimitActions(G.make('NovelGridworld-Pogostick-v1'), limited)
    w.reset()
    names = sorted(limited)
    for i in range(30):
        t = w.lookahead()
        full = _adapter_oracle_table(w)
        cols = [w.actions_id[nm] for nm in names]
        for k in ('reward', 'done', 'result', 'info'):
            assert t[k].shape == (len(limited),) and (t[k] == full[k][0][cols]).all(), (i, k)
        if i % 10 == 0:                                             # device=True: the same columns, as tensors
            td = w.lookahead(device=True)
            for k in ('reward', 'done', 'result'):
                assert td[k].is_cuda and (td[k].cpu().numpy() == t[k]).all(), (i, k)
            assert (td['info'].cpu().numpy().view(np.uint32) == t['info']).all(), i
        a = int(rs.randint(0, len(limited)))
        _, r, d, info = w.step(a)
        assert (r, d, info['result']) == (int(t.reward[a]), bool(t.done[a]), bool(t.result[a])), i
        if d or i % 10 == 9:
            w.reset()
    env.close(); w.close()


def test_sharded_env_and_cabi_errors():
    """The sharded env's table is the matching slice of one unsharded handle's (rank-local, no collective); NULL handle and NULL outputs
    at the C-ABI: a NULL handle is NGW_E_INVALID_ARG, any output pointer may be NULL."""
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    spec = T.build_spec('axe10')
    n = 2048
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=9, autoreset=True, horizon=20)
    v.reset()
    v.rollout(17, action_seed=3)
    host = v.lookahead(copy=True)
    sh = ShardedVecNovelGridworld(global_num_envs=n, spec=spec, seed=9, autoreset=True, horizon=20)
    sh.reset()
    sh.rollout(17, action_seed=3)
    lo = sh.local.env_index_base
    part = sh.lookahead()
    for k in ('reward', 'done', 'result', 'info'):
        assert (part[k] == host[k][lo:lo + sh.num_envs]).all(), k
    sh.close()
    L = _cabi.lib()
    assert L.ngw_lookahead(None) == _cabi.E_INVALID_ARG and 'NULL' in _cabi.last_error()
    assert L.ngw_get_lookahead(None, None, None, None) == _cabi.E_INVALID_ARG and 'NULL' in _cabi.last_error()
    assert L.ngw_lookahead_device_ptrs(None, None, None, None, None, None) == _cabi.E_INVALID_ARG and 'NULL' in _cabi.last_error()
    A = v.n_actions
    assert L.ngw_get_lookahead(v._h, None, None, None) == 0
    only = np.zeros((n, A), np.int32)
    assert L.ngw_get_lookahead(v._h, _cabi._ptr(only, np.int32), None, None) == 0 and (only == host['reward']).all()
    words = np.zeros((n, A), np.uint32)
    assert L.ngw_get_lookahead(v._h, None, None, _cabi._ptr(words, np.uint32)) == 0 and (words == host['info']).all()
    es, ast = C.c_int64(), C.c_int64()
    assert L.ngw_lookahead_device_ptrs(v._h, None, None, None, C.byref(es), C.byref(ast)) == 0
    assert es.value == 1 and ast.value == (n + 63) // 64 * 64
    p = C.c_void_p()
    assert L.ngw_lookahead_device_ptrs(v._h, C.byref(p), None, None, None, None) == 0 and p.value
    v.close()
