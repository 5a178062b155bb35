"""Device-side snapshots on the MI355X (csrc/ngw_snapshot.inc, include/ngw.h ngw_snapshot_*), held to the CPU oracle: the oracle twin is
driven with get_state()-style arrays and numpy indexing (tests/snapshot_oracle.py), every comparison is exact."""
import numpy as np
import pytest

import mask_oracle as M
import ngw_testlib as T
import snapshot_oracle as SO
from gym_novel_gridworlds_amd import VecNovelGridworld
from gym_novel_gridworlds_amd.lidar import LidarConfig
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX
from oracle.ngw_oracle import Oracle, agent_view, lidar

pytestmark = pytest.mark.gpu
KEYS = SO.STATE_KEYS


def same_state(v, o, where):
    st = v.get_state()
    for k in KEYS:
        bad = np.nonzero((st[k] != getattr(o.st, k)).reshape(v.num_envs, -1).any(1))[0]
        assert bad.size == 0, "%s: %s differs in %d envs, first %d" % (where, k, bad.size, bad[0])


def same_dict(a, b, where):
    for k in KEYS:
        assert (a[k] == b[k]).all(), (where, k)


def play(v, o, rs, k, where):
    """k host-API steps with random actions: reward, done and info equal the oracle's after every one."""
    A = len(v.actions_id)
    for t in range(k):
        a = rs.randint(0, A, v.num_envs).astype(np.int32)
        _, reward, done, info = v.step(a)
        assert o.step(a) == 0
        w = '%s step %d' % (where, t)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), w
        assert (info['result'] == o.result.astype(bool)).all() and (info['step_cost_code'] == o.cost_code).all(), w
        assert (info['message_code'] == o.msg_code).all() and (info['message_arg'] == o.msg_arg).all(), w


def pair(spec, n, seed, **kw):
    okw = {k: kw[k] for k in ('autoreset', 'horizon') if k in kw}
    return VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw), Oracle(spec.compile(), n, seed=seed, **okw)


ROUND_TRIP = [('pogo10', None), ('pogo10', 9), ('bow20', None), ('add32', None), ('fire10h', None), ('axe10', None), ('stk_fire_repl12', None),
              ('pogov0_10', None), ('pogo10', 48)]


@pytest.mark.parametrize('n', [1, 64, 1000, 4097])
@pytest.mark.parametrize('cfg,S', ROUND_TRIP)
def test_round_trip(cfg, S, n):
    """1 (+ 8): save all, play on, restore all: the seven arrays are those at the save, and the future is the oracle's from them."""
    spec = T.build_spec(cfg, S)
    seed = next(sd for sd in range(11, 60) if not Oracle(spec.compile(), n, seed=sd).reset() & 2)
    v, o = pair(spec, n, seed)
    v.reset(); o.reset()
    rs = np.random.RandomState(n + len(cfg))
    play(v, o, rs, 30, 'before the save')
    snap = v.snapshot()
    assert snap.capacity == n
    same_dict(snap.state(), SO.NumpySnapshot(spec.map_size, len(spec.items_id), n).state(), 'never-saved slots')
    snap.save()
    saved = SO.oracle_state(o)
    same_dict(snap.state(), saved, 'Snapshot.state()')
    play(v, o, rs, 30, 'after the save')
    snap.restore()
    SO.put_state(o, saved)
    same_dict(v.get_state(), saved, 'right after the restore')
    play(v, o, rs, 60, 'after the restore')
    same_state(v, o, 'end')
    assert v.error_flags() == 0
    snap.close()
    v.close()


@pytest.mark.parametrize('keep', [False, True])
@pytest.mark.parametrize('prefetch,depth', [(0, 0), ('auto', 0), ('auto', 4)])
@pytest.mark.parametrize('cfg', ['pogo10', 'bow20'])
def test_fork_by_index(cfg, prefetch, depth, keep):
    """2 + 3: a third of the envs saved into shuffled slots of a smaller snapshot, restored with repeated slots into a different half; envs
    not named keep every byte; then 40 steps under autoreset with horizon 16, in which every env ends at least two episodes."""
    spec = T.build_spec(cfg)
    n, H = 3001, 16
    v, o = pair(spec, n, 29, autoreset=True, horizon=H, reset_prefetch=prefetch, reset_prefetch_depth=depth)
    v.reset(); o.reset()
    rs = np.random.RandomState(7)
    play(v, o, rs, 5, 'warm-up')
    third = rs.choice(n, n // 3, replace=False)
    cap = n // 3 + 5
    slots = rs.permutation(cap)[:len(third)]
    snap, model = v.snapshot(cap), SO.NumpySnapshot(spec.map_size, len(spec.items_id), cap)
    snap.save(envs=third, slots=slots); model.save(o.st, third, slots)
    same_dict(snap.state(), model.state(), 'saved and never-saved slots')
    play(v, o, rs, 10, 'between')
    half = rs.choice(n, n // 2, replace=False)
    rslots = rs.choice(slots, len(half))
    assert len(np.unique(rslots)) < len(rslots)
    before = v.get_state()
    snap.restore(slots=rslots, envs=half, keep_episode=keep); model.restore(o.st, rslots, half, keep)
    after = v.get_state()
    others = np.setdiff1d(np.arange(n), half)
    for k in KEYS:
        assert after[k][others].tobytes() == before[k][others].tobytes(), k
    same_state(v, o, 'right after the restore')
    ends = np.zeros(n, np.int64)
    for t in range(40):
        play(v, o, rs, 1, 'after the fork, t=%d' % t)
        ends += o.done
    assert ends.min() >= 2, "every env ends at least two episodes in the 40 steps"
    same_state(v, o, 'end')
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('kind', ['random', 'constant'])
def test_fork_src(kind):
    """4: fork(src) with a random src (fixed points included) and a constant one."""
    spec = T.build_spec('pogo10')
    n = 2500
    v, o = pair(spec, n, 31, autoreset=True, horizon=16)
    v.reset(); o.reset()
    rs = np.random.RandomState(3)
    play(v, o, rs, 12, 'warm-up')
    src = rs.randint(0, n, n) if kind == 'random' else np.full(n, 1234)
    if kind == 'random':
        src[::7] = np.arange(n)[::7]
    v.fork(src)
    st = SO.oracle_state(o)
    SO.put_state(o, {k: st[k][src] for k in KEYS})
    same_state(v, o, 'right after fork')
    play(v, o, rs, 40, 'after fork')
    same_state(v, o, 'end')
    with pytest.raises(ValueError):
        v.fork(src[:-1])
    v.close()


@pytest.mark.parametrize('cfg,S', [('pogo10', None), ('add32', None), ('pogo10', 36)])
def test_restore_refreshes_the_fused_lidar(cfg, S):
    """5: fused LidarInFront: the observation right after a restore and after each of 10 more steps - from the occupancy bit rows (10 x 10,
    32 x 32) and, beyond 32 x 32, from the march over staged maps."""
    spec = T.build_spec(cfg, S)
    n = 1500
    v, o = pair(spec, n, 37, autoreset=True, horizon=14)
    lc = LidarConfig(spec, 8)
    v.lidar_configure(lc, fused=True, dtype=np.int16)
    cc = lc.compile(spec)

    def check(where):
        got = v.lidar_observation()
        exp = lidar(cc, spec.map_size, len(spec.items_id), o.st.map, o.st.loc, o.st.facing, o.st.inv)
        assert (got == exp).all(), where
    v.reset(); o.reset()
    rs = np.random.RandomState(4)
    play(v, o, rs, 8, 'a'); check('before')
    snap = v.snapshot(); snap.save(); saved = SO.oracle_state(o)
    play(v, o, rs, 9, 'b')
    perm = rs.permutation(n)
    snap.restore(slots=perm); SO.put_state(o, {k: saved[k][perm] for k in KEYS})
    check('right after the restore')
    for t in range(10):
        play(v, o, rs, 1, 'c'); check('step %d after the restore' % t)
    same_state(v, o, 'end')
    v.close()


def test_restore_around_masks_view_terminal_graph_rollout():
    """5: action masks (on), agent_view, the host step's mirror, terminal capture, a replayed graph before and after, a fused rollout after."""
    import torch
    spec = T.build_spec('pogo10')
    n, A, H = 5000, len(spec.actions_id), 12
    v, o = pair(spec, n, 41, autoreset=True, horizon=H, terminal_capture=True)
    v.set_action_masks(True)
    v.reset(); o.reset()
    rs = np.random.RandomState(6)
    play(v, o, rs, 7, 'a')
    snap = v.snapshot(); snap.save(); saved = SO.oracle_state(o)
    play(v, o, rs, 6, 'b')
    src = rs.randint(0, n, n)

    def restore():
        snap.restore(slots=src); SO.put_state(o, {k: saved[k][src] for k in KEYS})
    restore()
    assert (v.action_mask_words() == M.oracle_mask_words(spec, o.st)).all()
    assert (v.agent_view(5) == agent_view(o.st.map.reshape(n, spec.map_size, spec.map_size), o.st.loc, 5)).all()
    for t in range(10):                                                    # the host step: its page-locked mirror was stale after the restore
        a = rs.randint(0, A, n).astype(np.int32)
        o2 = Oracle(spec.compile(), n, seed=41)                            # (no autoreset: the state an episode ENDS in)
        o2.st = o.st.copy()
        o2.step(a)
        obs, reward, done, info = v.step(a, copy=True); o.step(a)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all()
        assert (obs['map'].reshape(n, -1) == o.st.map).all() and (obs['agent_location'] == o.st.loc).all()
        assert (obs['agent_facing_id'] == o.st.facing).all() and (obs['inventory_items_quantity'] == o.st.inv).all()
        term = v.terminal_observation()
        e = np.nonzero(o.done)[0]
        assert (term['map'].reshape(n, -1)[e] == o2.st.map[e]).all() and (term['agent_location'][e] == o2.st.loc[e]).all()
        assert (term['inventory_items_quantity'][e] == o2.st.inv[e]).all()
    assert (v.action_mask_words() == M.oracle_mask_words(spec, o.st)).all()
    acts = torch.randint(0, A, (20, n), dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    an = acts.cpu().numpy()
    v.graph_build(acts.data_ptr(), n, 20)
    for rep in range(2):
        v.graph_launch(1)
        for t in range(20):
            o.step(an[t])
        same_state(v, o, 'graph replay %d' % rep)
        restore()
        same_state(v, o, 'restore after replay %d' % rep)
    v.rollout(25, action_seed=7, t0=3); assert o.rollout(25, 7, 3) == 0
    same_state(v, o, 'rollout after a restore')
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('timeout_us', ['3', '300'])
def test_one_env_handle_restores_between_loop_steps(timeout_us, monkeypatch):
    """6: the one-env resident loop: a restore between its steps; the step after it is the oracle's."""
    monkeypatch.setenv('NGW_SOLO_TIMEOUT_US', timeout_us)
    spec = T.build_spec('pogo10')
    A = len(spec.actions_id)
    v, o = pair(spec, 1, 43)
    v.reset1(); o.reset()
    rs = np.random.RandomState(8)

    def step(where):
        a = int(rs.randint(0, A))
        got = v.step1(a)
        o.step(np.array([a], np.int32))
        assert got == (int(o.reward[0]), bool(o.done[0]), bool(o.result[0]), int(o.cost_code[0]), int(o.msg_code[0]), int(o.msg_arg[0])), where
        mb, r, c, f, ib, sel, steps = v.last_state1()
        assert (np.frombuffer(mb, np.int8) == o.st.map[0]).all() and (r, c, f) == (o.st.loc[0][0], o.st.loc[0][1], o.st.facing[0]), where
        assert (np.frombuffer(ib, np.int32) == o.st.inv[0]).all() and sel == o.st.selected[0] and steps == o.st.step_count[0], where
    for t in range(6):
        step('a%d' % t)
    snap = v.snapshot(3)
    snap.save(slots=[2]); saved = SO.oracle_state(o)
    for rep in range(3):
        for t in range(5):
            step('b%d.%d' % (rep, t))
        snap.restore(slots=[2]); SO.put_state(o, saved)
        step('right after restore %d' % rep)
        same_state(v, o, 'restore %d' % rep)
    assert v.error_flags() == 0
    v.close()


def test_bad_indices_and_misuse():
    """7: an out-of-range env or slot (device lists are not checked on the host) skips that one copy and raises F_BAD_INDEX; misuse raises."""
    import torch
    spec = T.build_spec('pogo10')
    n = 300
    v, o = pair(spec, n, 47)
    v.reset(); o.reset()
    rs = np.random.RandomState(9)
    play(v, o, rs, 10, 'a')
    snap, model = v.snapshot(100), SO.NumpySnapshot(spec.map_size, len(spec.items_id), 100)

    def dev(x):
        t = torch.tensor(x, dtype=torch.int32, device='cuda:0')
        torch.cuda.synchronize()
        return t
    envs, slots = [5, n, 7, -1, 9, 11], [0, 1, 2, 3, 100, -5]
    snap.save(envs=dev(envs), slots=dev(slots))
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0       # sticky until read
    model.save(o.st, [5, 7], [0, 2])
    SO_state = snap.state()
    for k in KEYS:
        assert (SO_state[k] == model.state()[k]).all(), k
    same_state(v, o, 'a save changes no env')
    play(v, o, rs, 5, 'b')
    before = v.get_state()
    snap.restore(slots=dev([0, 100, 2, -1, 2]), envs=dev([20, 21, n, 23, 24]))
    assert v.error_flags() == F_BAD_INDEX
    model.restore(o.st, [0, 2], [20, 24])
    same_state(v, o, 'only the two valid copies happened')
    after = v.get_state()
    for k in KEYS:
        assert after[k][[21, 23]].tobytes() == before[k][[21, 23]].tobytes(), k
    play(v, o, rs, 5, 'c')
    # host lists are checked before anything is launched
    for call in (lambda: snap.save(envs=[0, n]), lambda: snap.save(slots=[1, 1], envs=[0, 1]), lambda: snap.restore(envs=[3, 3], slots=[0, 1]),
                 lambda: snap.restore(slots=[100]), lambda: snap.save(envs=[1.0]), lambda: snap.save(envs=[1, 2], slots=[1]),
                 lambda: snap.save(), lambda: snap.restore(),                       # count = num_envs > capacity
                 lambda: snap.restore(slots=dev(np.zeros(n + 1, np.int32))),       # count above n_envs
                 lambda: snap.save(envs=dev(np.zeros(101, np.int32))),             # count above capacity
                 lambda: snap.save(envs=torch.zeros(3, dtype=torch.int64, device='cuda:0')), lambda: snap.save(envs=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError):
            call()
    assert v.error_flags() == 0
    same_state(v, o, 'refused calls change nothing')
    # a snapshot of another env
    w = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    w.reset()
    from gym_novel_gridworlds_amd import _cabi
    assert _cabi.lib().ngw_snapshot_save(w._h, snap._s, None, None, 10) == -1
    assert _cabi.lib().ngw_snapshot_restore(w._h, snap._s, None, None, 10, 0) == -1
    assert _cabi.lib().ngw_snapshot_restore(v._h, snap._s, None, None, 10, 2) == -1      # unknown flag
    w.close()
    # closed, and closed by rebuild()
    s2 = v.snapshot(4)
    s2.close()
    for call in (s2.save, s2.restore, s2.state):
        with pytest.raises(ValueError, match='closed'):
            call()
    v.rebuild(T.build_spec('axe10'))
    for call in (snap.save, snap.restore, snap.state):
        with pytest.raises(ValueError, match='closed'):
            call()
    v.reset()
    s3 = v.snapshot()
    s3.save(); s3.restore()
    v.close()
    with pytest.raises(ValueError, match='closed'):
        s3.save()
