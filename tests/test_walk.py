"""Walk distances and go-to plans on the MI355X (csrc/ngw_walk.inc, include/ngw.h ngw_snapshot_walk, Snapshot.walk_distances / walk_plans,
VecNovelGridworld.walk_distances / walk_plans, the adapter's walk_distances / walk_plan), held to the plain-Python oracle (tests/walk_oracle.py)
applied to a host copy of the rows - pool.state() / get_state() - never to the device's own answer."""
import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import walk_oracle as WO
import gym_novel_gridworlds_amd as G
from gym_novel_gridworlds_amd import VecNovelGridworld, walk
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_WALK = ['pogo10', 'pogo13', 'bow20', 'add32', 'add12m', 'remape10', 'fence12h', 'replwall12e', 'crate12h']
CFG_END_TO_END = ['pogo10', 'bow20', 'add32', 'remape10']


def dev_i32(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def grow(v, pool, n, rs, A):
    """Slots 0 .. n-1 := the envs, slots n .. 2n-1 := one generation of children of them: states no env is in."""
    pool.save(slots=np.arange(n))
    pool.expand(rs.randint(0, n, n), rs.randint(0, A, n), n + np.arange(n))


def assert_walk(got, rows, idx, K, items, steps, ids, where):
    """A WalkPlans (or the distances alone: items None) of rows idx against the oracle, every entry."""
    dist, plans, length = WO.walk_rows(rows, idx, K, items, steps, ids)
    if items is None:
        g = got.cpu().numpy() if hasattr(got, 'cpu') else got
        assert g.dtype == np.int32 and g.shape == dist.shape and (g == dist).all(), '%s: dist, first bad row %s' % (where, np.argwhere(g != dist)[:1])
        return
    gp, gl, gd = [x.cpu().numpy() if hasattr(x, 'cpu') else x for x in got]
    assert gd.dtype == np.int32 and gd.shape == dist.shape and (gd == dist).all(), '%s: dist, first bad %s' % (where, np.argwhere(gd != dist)[:1])
    assert gl.dtype == np.int32 and gl.shape == length.shape and (gl == length).all(), '%s: length, first bad %s' % (where, np.argwhere(gl != length)[:1])
    assert gp.dtype == np.int32 and gp.shape == plans.shape and (gp == plans).all(), '%s: plans, first bad %s' % (where, np.argwhere(gp != plans)[:1])


@pytest.mark.parametrize('cfg', CFG_WALK)
def test_every_configuration(cfg):
    """130 envs (two full waves and a partial one) after reset and after ~40 random steps; the pool holds the envs' states and a generation of
    children; 200 random slots with repeats: every distance, and the plan and length to a random item per row."""
    spec = T.build_spec(cfg)
    n, A, K = 130, len(spec.actions_id), len(spec.items_id)
    ids = walk.walk_action_ids(spec)
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=25)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=25)
    v.reset(); o.reset()
    pool = v.snapshot(2 * n)
    rs = np.random.RandomState(23)
    steps = 3 * spec.map_size
    for stage in ('after reset', 'after random play'):
        if stage == 'after random play':
            for t in range(40):
                a = rs.randint(0, A, n).astype(np.int32)
                if o.step(a) & 2:                               # a tight map exhausted the placement of an autoreset: stop here
                    break
                v.step(a)
        where = '%s %s' % (cfg, stage)
        grow(v, pool, n, rs, A)
        rows = pool.state()
        slots, items = rs.randint(0, 2 * n, 200), rs.randint(0, K, 200)
        assert_walk(pool.walk_distances(slots), rows, slots, K, None, 0, ids, where)
        assert_walk(pool.walk_plans(slots, items, steps), rows, slots, K, items, steps, ids, where)
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('S', [9, 10, 32, 33, 64])
@pytest.mark.parametrize('count', [1, 63, 65, 200])
def test_map_sizes_and_counts(S, count):
    """The row-word boundaries (32: the last size on 32-bit words, 33: the first on 64-bit ones, 64: the largest map), the odd sizes whose rows start
    at any byte, and counts around the wavefront width and far above the snapshot's capacity: host lists, device tensors with the results left
    on the device, slots=None."""
    import torch
    spec = make_spec(T.POGO, S)
    n, A, K, cap = 5, len(spec.actions_id), len(spec.items_id), 20
    ids = walk.walk_action_ids(spec)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n), autoreset=True, horizon=60)
    v.reset()
    rs = np.random.RandomState(S + count)
    pool = v.snapshot(cap)
    for first in range(0, cap, n):                           # (every size alike: expand is refused above 48 x 48)
        for t in range(6):
            v.step(rs.randint(0, A, n).astype(np.int32))
        pool.save(envs=np.arange(n), slots=first + np.arange(n))
    rows = pool.state()
    where = 'S=%d count=%d' % (S, count)
    steps = 24
    host, on_dev = rs.randint(0, cap, count), rs.randint(0, cap, count)
    items_h, items_d = rs.randint(0, K, count), rs.randint(0, K, count)
    assert_walk(pool.walk_distances(host), rows, host, K, None, 0, ids, where + ' host list')
    assert_walk(pool.walk_plans(host, items_h, steps), rows, host, K, items_h, steps, ids, where + ' host list')
    got = pool.walk_distances(dev_i32(on_dev), device=True)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and tuple(got.shape) == (count, K) and got.is_cuda
    assert_walk(got, rows, on_dev, K, None, 0, ids, where + ' device tensor')
    got = pool.walk_plans(dev_i32(on_dev), dev_i32(items_d), steps, device=True)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got) and tuple(got.plans.shape) == (steps, count)
    assert_walk(got, rows, on_dev, K, items_d, steps, ids, where + ' device tensor')
    item = int(rs.randint(1, K))
    assert_walk(pool.walk_distances(), rows, np.arange(cap), K, None, 0, ids, where + ' every slot')
    assert_walk(pool.walk_plans(None, item, steps), rows, np.arange(cap), K, np.full(cap, item), steps, ids, where + ' every slot, one item')
    assert v.error_flags() == 0
    v.close()


def hand_built(S, K, WALL, ITEM, OTHER):
    """Five states at S x S: (maps [5, S, S], poses)."""
    def room():
        m = np.zeros((S, S), np.int8)
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = WALL
        return m
    maps, poses = [], []
    m = room()                                               # 0: a serpentine corridor, the item at its far end
    for r in range(2, S - 2, 2):
        m[r, 1:S - 1] = WALL
        m[r, S - 2 if (r // 2) % 2 else 1] = 0
    m[S - 2, S - 2] = ITEM
    maps.append(m); poses.append((1, 1, 0))
    m = room()                                               # 1: walled in on all four sides
    m[9, 10] = m[11, 10] = m[10, 9] = WALL
    m[10, 11] = ITEM
    m[20, 20] = OTHER
    maps.append(m); poses.append((10, 10, 0))
    m = room()                                               # 2: one item inside a sealed pocket, one of the same id outside
    m[4:7, 4:7] = WALL
    m[5, 5] = ITEM
    m[S - 3, S - 3] = ITEM
    m[12, 3:20] = WALL
    maps.append(m); poses.append((2, 2, 1))
    m = room()                                               # 3: two goal poses at one distance
    m[13, 13], m[13, 17] = ITEM, ITEM
    maps.append(m); poses.append((15, 15, 0))
    m = room()                                               # 4: two paths of one length (around a block, either side)
    m[14:17, 14:17] = WALL
    m[10, 15] = ITEM
    maps.append(m); poses.append((20, 15, 0))
    return np.stack(maps), poses


def test_hand_built_states():
    """States put in through set_state and save, at 32 x 32: a walk of more than 255 and more than 2 * S moves (a narrow distance type, a fixed
    iteration bound, an early exit), an agent that cannot move, a sealed pocket, the tie rules, and plans cut at T with the true length."""
    S = 32
    spec = make_spec(T.POGO, S)
    K, ids = len(spec.items_id), walk.walk_action_ids(spec)
    WALL, ITEM, OTHER = spec.items_id['wall'], spec.items_id['tree_log'], spec.items_id['crafting_table']
    maps, poses = hand_built(S, K, WALL, ITEM, OTHER)
    n = len(maps)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset()
    v.set_state(0, map=maps.reshape(n, -1), loc=np.array([p[:2] for p in poses]), facing=np.array([p[2] for p in poses]))
    pool = v.snapshot(n)
    pool.save()
    rows = pool.state()
    assert (rows['map'].reshape(n, S, S) == maps).all()
    slots = np.arange(n)
    far = pool.walk_plans(slots, ITEM, 16)
    assert far.length[0] > 255 and far.length[0] > 2 * S and (far.plans[:, 0] >= 0).all()        # cut at T, the true length
    assert far.length[1] == 1 and far.dist[1, WALL] == 0 and far.dist[1, 0] == -1 and far.dist[1, OTHER] == -1
    assert sorted(k for k in range(K) if far.dist[1, k] >= 0) == sorted({WALL, ITEM})
    assert far.length[2] > 0 and far.length[3] > 0 and far.length[4] > 0
    for item in range(K):
        for steps in (16, 700):
            assert_walk(pool.walk_plans(slots, item, steps), rows, slots, K, np.full(n, item), steps, ids, 'hand-built item %d T %d' % (item, steps))
    m = maps[2].copy()
    m[S - 3, S - 3] = 0                                      # without the one outside, the pocket's item is out of reach
    v.set_state(2, map=m.reshape(1, -1))
    assert v.walk_plans(ITEM, 8, envs=[2]).length[0] == -1
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('cfg', CFG_END_TO_END)
def test_plans_rolled_out_leave_the_agent_facing_the_item(cfg):
    """walk_plans left on the device and fed to rollout with limits = length: every child faces a cell of the requested id after exactly
    `length` steps, none of which failed; an unreachable item leaves a copy of the parent."""
    import torch
    spec = T.build_spec(cfg)
    n, A, K = 130, len(spec.actions_id), len(spec.items_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n), autoreset=False)
    v.reset()
    rs = np.random.RandomState(31)
    for t in range(30):
        v.step(rs.randint(0, A, n).astype(np.int32))
    pool = v.snapshot(3 * n)
    grow(v, pool, n, rs, A)
    steps = 4 * spec.map_size
    parents, children = rs.randint(0, 2 * n, n), 2 * n + np.arange(n)
    maps = pool.state()['map']
    # four pairs in five ask for an id that lies on the parent's map (most ids are inventory-only and give -1), the others for any id
    items = np.array([rs.choice(np.unique(maps[q])) if rs.rand() < 0.8 else rs.randint(0, K) for q in parents])
    d_par, d_items, d_chi = dev_i32(parents), dev_i32(items), dev_i32(children)
    p = pool.walk_plans(d_par, d_items, steps, device=True)
    limits = p.length.clamp(0, steps)
    roll = pool.rollout(d_par, p.plans, children=d_chi, limits=limits, rewards=True, device=True)
    torch.cuda.synchronize()
    length, plans = p.length.cpu().numpy(), p.plans.cpu().numpy()
    got_len, ended, rewards, info = roll.length.cpu().numpy(), roll.ended.cpu().numpy(), roll.rewards.cpu().numpy(), roll.info.cpu().numpy()
    st = pool.state()
    step_reward = spec.compile().reward_step
    assert (length >= 0).sum() > n // 2, cfg                 # (the test means something)
    assert (got_len == np.clip(length, 0, steps)).all() and not ended.any()
    for j in range(n):
        where = '%s pair %d item %d length %d' % (cfg, j, items[j], length[j])
        if length[j] < 0:
            assert (plans[:, j] == -1).all(), where
            for name in ('map', 'loc', 'facing', 'inv', 'selected'):
                assert (st[name][children[j]] == st[name][parents[j]]).all(), where + ': the child is no copy of its parent'
            continue
        if length[j] > steps:                                # (cut at T: the walk is not over)
            assert (plans[:, j] >= 0).all(), where
            continue
        assert WO.faces(st, children[j], items[j]), where + ': the child does not face the item'
        assert (rewards[:length[j], j] == step_reward).all() and (rewards[length[j]:, j] == 0).all(), where
        assert length[j] == 0 or info[j] & 1, where + ': the last move failed'
    assert v.error_flags() == 0
    v.close()


def test_bad_index_and_bad_item_through_device_tensors():
    spec = make_spec(T.POGO, 10)
    n, K = 70, len(spec.items_id)
    ids = walk.walk_action_ids(spec)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n))
    v.reset()
    pool = v.snapshot(n)
    pool.save()
    rows = pool.state()
    slots, items = np.arange(n), np.full(n, spec.items_id['tree_log'])
    bad_slots, bad_items = slots.copy(), items.copy()
    bad_slots[3], bad_slots[66] = n, -1
    bad_items[9], bad_items[65] = K, -2
    got = pool.walk_plans(dev_i32(bad_slots), dev_i32(bad_items), 12)
    bad = [3, 66, 9, 65]
    assert (got.dist[bad] == -1).all() and (got.length[bad] == -1).all() and (got.plans[:, bad] == -1).all()
    good = np.setdiff1d(slots, bad)
    assert_walk(G.WalkPlans(got.plans[:, good], got.length[good], got.dist[good]), rows, good, K, items[good], 12, ids, 'beside bad rows')
    assert v.error_flags() & F_BAD_INDEX
    only = pool.walk_distances(dev_i32(bad_slots))
    assert (only[[3, 66]] == -1).all() and (only[good] == got.dist[good]).all()
    v.close()


def test_nothing_is_committed_and_the_live_env_calls_match_a_snapshot():
    spec = T.build_spec('bow20')
    n, A, K = 130, len(spec.actions_id), len(spec.items_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n), autoreset=True, horizon=40)
    v.reset()
    rs = np.random.RandomState(3)
    for t in range(20):
        v.step(rs.randint(0, A, n).astype(np.int32))
    snap = v.snapshot()
    snap.save()
    before = (v.state_keys(fields=G.KEY_ALL), snap.keys(fields=G.KEY_ALL), v.action_masks())
    items = rs.randint(0, K, n)
    live_d, live_p = v.walk_distances(), v.walk_plans(items, 50)
    saved_d, saved_p = snap.walk_distances(), snap.walk_plans(None, items, 50)
    some = rs.randint(0, n, 33)
    part = v.walk_plans(items[some], 50, envs=some)
    after = (v.state_keys(fields=G.KEY_ALL), snap.keys(fields=G.KEY_ALL), v.action_masks())
    assert all((a == b).all() for a, b in zip(before, after))
    assert (live_d == saved_d).all() and all((a == b).all() for a, b in zip(live_p, saved_p))
    assert (part.plans == live_p.plans[:, some]).all() and (part.length == live_p.length[some]).all() and (part.dist == live_d[some]).all()
    assert_walk(live_p, v.get_state(), np.arange(n), K, items, 50, walk.walk_action_ids(spec), 'live envs')
    assert v.error_flags() == 0
    v.close()


def test_host_validation_on_the_device_path():
    from gym_novel_gridworlds_amd import limit_actions_vec
    spec = make_spec(T.POGO, 10)
    K = len(spec.items_id)
    v = VecNovelGridworld(spec=spec, num_envs=4, seed=4)
    v.reset()
    pool = v.snapshot()
    pool.save()
    for bad, match in ((K, 'outside'), ([0, 1], 'items for 4 rows'), (None, 'expected')):
        with pytest.raises(ValueError, match=match):
            pool.walk_plans(None, bad, 8)
    with pytest.raises(ValueError, match='steps'):
        pool.walk_plans(None, 1, 0)
    with pytest.raises(ValueError, match='outside'):
        pool.walk_distances([4])
    no_left = limit_actions_vec(v, ['Forward', 'Right', 'Break'])
    no_left.reset()
    assert (no_left.walk_distances() == v.walk_distances()).all()
    with pytest.raises(ValueError, match='no Left'):
        no_left.walk_plans(1, 8)
    assert v.error_flags() == 0 and no_left.error_flags() == 0
    no_left.close()
    v.close()


def test_the_adapter_limit_actions_and_a_wrapper_forward():
    from gym_novel_gridworlds_amd import LimitActions
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    env = T.make_adapter_env('remape10', 'hip')
    env.reset()
    rs = np.random.RandomState(5)
    A = len(env.actions_id)
    for t in range(15):
        env.step(int(rs.randint(0, A)))
    vec = getattr(env, 'unwrapped', env)._backend()                # (remapaction easy returns the adapter itself)
    spec, rows = vec.spec, vec.get_state()
    K, ids = len(spec.items_id), walk.walk_action_ids(vec.spec)
    d = env.walk_distances()
    assert d.shape == (K,)
    wrapped = NoveltyWrapper(env)
    assert (wrapped.walk_distances() == d).all()
    names = ['Forward', 'Left', 'Right', 'Break']
    lim = LimitActions(env, set(names))
    assert (lim.walk_distances() == d).all()
    for item in range(K):
        dist, column, length = WO.walk(rows['map'][0], rows['loc'][0], rows['facing'][0], K, item, 64, ids)
        assert list(d) == dist
        plan, n = env.walk_plan(item, 64)
        assert (plan, n) == ([a for a in column if a >= 0], length) and wrapped.walk_plan(item, 64) == (plan, n)
        back = {lim.limited_actions_id[name]: env.actions_id[name] for name in names}
        lplan, ln = lim.walk_plan(item, 64)
        assert ln == n and [back[a] for a in lplan] == plan
    with pytest.raises(ValueError, match='Left is not among the limited actions'):
        LimitActions(env, {'Forward', 'Right', 'Break'}).walk_plan(1, 8)
    env.close()
