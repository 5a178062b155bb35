"""Search runs on the MI355X (csrc/ngw_search.inc, csrc/ngw_abi_search.cpp, include/ngw.h ngw_search_*; search.py, Snapshot.search): whole
iterations of the label-correcting loop enqueued from one call.  Held to two things: the model of tests/search_oracle.py on the CPU oracle -
the stored keys and every key's value, g and the key behind every slot's bucket, the parents, the pool's rows, the statistics, the goal -,
and the hand-written loop of tests/test_key_values.py (copied here) run on a second pool and table.
Which bucket a key gets is not part of the table's contract (two new keys of one call that collide race for it), so wherever a bucket is
compared between two tables - s.bucket, the tags - it is compared through the key it holds: the same states, values, parents and actions."""
import numpy as np
import pytest

import expand_oracle as XO
import key_table_oracle as KT
import key_value_oracle as KV
import ngw_testlib as T
import search_oracle as SX
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.frontier import select_reference
from gym_novel_gridworlds_amd.key_table import TAG_ROOT, VALUE_NONE, Trace, step_cost_values
from gym_novel_gridworlds_amd.search import Search, SearchGoal, SearchStats
from gym_novel_gridworlds_amd.snapshot import MapsTooLarge
from gym_novel_gridworlds_amd.spec import F_FRONTIER_FULL, IDX_NONE, make_spec

pytestmark = pytest.mark.gpu
S_SMALL = 9
CAP, CAP_POOL, CAP_TABLE = 256, 512, 2048


def dev(x, dtype=np.int32):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()
    torch.cuda.synchronize()
    return t


def host(x):
    return x.cpu().numpy() if hasattr(x, 'data_ptr') else np.asarray(x)


def padded(roots, capacity):
    return np.r_[np.asarray(roots, np.int64), np.full(capacity - len(roots), IDX_NONE)].astype(np.int32)


@pytest.fixture(scope='module')
def venv():
    """The 9 x 9 Pogostick env with 4 envs of tests/test_key_values.py."""
    spec = make_spec(T.POGO, S_SMALL)
    v = VecNovelGridworld(spec=spec, num_envs=4, seed=XO.good_seed(spec, 4))
    v.reset()
    yield v
    v.close()


def pool_of_envs(v, cap_pool=CAP_POOL, first_sequence=0):
    """A pool whose first slots hold the envs' states, and a valued table."""
    pool, table = v.snapshot(cap_pool), v.key_table(CAP_TABLE, values=True, _first_sequence=first_sequence)
    pool.save(envs=np.arange(v.num_envs), slots=np.arange(v.num_envs))
    return pool, table


def model_of(v, pool, capacity, n_slots, **kw):
    """The CPU model over the pool's first n_slots rows."""
    m = SX.SearchModel(v.spec, capacity, pool.capacity, **kw)
    m.save(pool.state(0, n_slots), np.arange(n_slots))
    m.cursor = n_slots
    return m


def hand_loop(v, pool, table, capacity, roots, iterations, cursor, costs=None, scale=1, keep=None):
    """The loop of tests/test_key_values.py::test_label_correcting_search_against_the_cpu_oracle - key_table.py's docstring with a Frontier -,
    with fr.select in the place of fr.compact where keep is given.  -> what it leaves, on the host, and per iteration (keys, values, best,
    p, a, c, parents)."""
    import torch
    A, cap_pool = v.n_actions, pool.capacity
    fr = pool.frontier(capacity)
    fr.reset_cursor(cursor)
    cost_t, arange_a = (None if costs is None else dev(costs)), dev(np.arange(A))
    parents = dev(padded(roots, capacity))
    g = torch.full((cap_pool + 1,), VALUE_NONE, dtype=torch.int32, device='cuda')          # (one more entry: where IDX_NONE slots write)
    bucket = torch.full((cap_pool + 1,), -1, dtype=torch.int32, device='cuda')
    keys, found = pool.insert_keys_min(table, parents, torch.zeros(capacity, dtype=torch.int32, device='cuda'), device=True)

    def note(slots, where):
        at = torch.where(slots != IDX_NONE, slots, cap_pool).long()
        g[at], bucket[at] = table.read(where, device=True)[0], where
        g[cap_pool], bucket[cap_pool] = VALUE_NONE, -1
    note(parents, found.where)
    seen, per_iteration = [host(keys)], []
    for it in range(iterations):
        succ = pool.successor_keys(parents, device=True)
        live, pi = (parents != IDX_NONE)[:, None], parents.clamp(min=0).long()
        step = cost_t[None, :] if costs is not None else step_cost_values(succ.info, scale)
        g_child = torch.where(live, g[pi][:, None] + step, VALUE_NONE).to(torch.int32).contiguous()
        tags = (bucket[pi][:, None] * A + arange_a[None, :]).to(torch.int32)
        found = table.insert_min(succ.keys.reshape(-1), g_child.reshape(-1), tags=tags.reshape(-1).contiguous(), device=True)
        if keep is None:
            p, a = fr.compact(found.best, A, parents)
        else:
            sel = fr.select(g_child, keep, A, parents, flags=found.best)
            p, a = sel.first, sel.second
        c = fr.alloc()
        pool.expand(p, a, c, device=True)
        note(c, table.lookup(pool.keys(c, device=True), device=True))
        per_iteration.append(tuple(host(x).copy() for x in (succ.keys.reshape(-1), g_child.reshape(-1), found.best, p, a, c, parents)))
        seen.append(per_iteration[-1][0])
        parents = c.clone()
    out = dict(g=host(g)[:cap_pool], bucket=host(bucket)[:cap_pool], parents=host(parents), cursor=int(host(fr.cursor)[0]),
               seen=np.unique(np.concatenate(seen).view(np.uint64)), iterations=per_iteration)
    fr.close()
    return out


def table_by_key(table, seen, A):
    """What the table holds, free of bucket numbers: {key: (value, the key of the tag's parent bucket or None for a root, the tag's action)}
    over the keys `seen` (uint64; 0 skipped), and {bucket: key}."""
    ks = seen[seen != 0]
    where = table.lookup(ks)
    assert (where >= 0).all() and len(table) == len(ks), "the table holds other keys than the loop offered"
    value, tag = table.read(where)
    key_of = dict(zip(where.tolist(), ks.tolist()))
    return {k: (int(x), None if t == TAG_ROOT else key_of[t // A], None if t == TAG_ROOT else t % A)
            for k, x, t in zip(ks.tolist(), value.tolist(), tag.tolist())}, key_of


def assert_same_bytes(v, loop, pool_l, table_l, s, pool_s, table_s, what):
    """A search against the hand-written loop on a second pool and table: the tables, g, the key behind every slot's bucket, the final
    parents, the cursor and every row of the pool that was handed out."""
    A = v.n_actions
    st = s.stats()
    held_l, key_of_l = table_by_key(table_l, loop['seen'], A)
    held_s, key_of_s = table_by_key(table_s, loop['seen'], A)
    assert held_l == held_s, "%s: the tables differ" % what
    assert st.cursor == loop['cursor'] and (host(s.parents) == loop['parents']).all(), "%s: the parents" % what
    assert (host(s.g) == loop['g']).all(), "%s: g" % what
    b_s, b_l = host(s.bucket), loop['bucket']
    assert ((b_s >= 0) == (b_l >= 0)).all() and [key_of_s[b] for b in b_s[b_s >= 0].tolist()] == [key_of_l[b] for b in b_l[b_l >= 0].tolist()], "%s: bucket" % what
    n_slots = min(st.cursor, pool_s.capacity)
    XO.assert_rows(pool_s.state(0, n_slots), pool_l.state(0, n_slots), what)
    assert (pool_s.keys(np.arange(n_slots)) == pool_l.keys(np.arange(n_slots))).all()
    assert [key_of_s[b] for b in b_s[:n_slots].tolist() if b >= 0] == [int(k) for k, b in zip(pool_s.keys(np.arange(n_slots)), b_s[:n_slots]) if b >= 0]
    return st


def assert_model(v, s, pool, table, m, what, flags=None):
    """A search against the CPU model: parents, g, the key behind every bucket, the table's keys and values, the pool's rows, the
    statistics, the goal.  -> the statistics."""
    st = s.stats()
    assert isinstance(st, SearchStats) and st.iterations == len(m.iterations) and st.cursor == m.cursor, what
    assert host(s.parents).tolist() == m.parents, "%s: the parents" % what
    assert host(s.g).tolist() == m.g, "%s: g" % what
    reached = [slot for slot in range(pool.capacity) if m.g[slot] != VALUE_NONE]
    b = host(s.bucket)
    assert (b[[slot for slot in range(pool.capacity) if slot not in set(reached)]] == -1).all()
    if reached:
        assert (table.lookup(np.array([m.key[slot] for slot in reached], np.uint64)) == b[reached]).all(), "%s: bucket" % what
    ks = np.array(list(m.table.held), np.uint64)
    assert len(table) == len(m.table), "%s: the stored keys" % what
    if len(ks):
        assert (table.lookup(ks) >= 0).all() and (table.get(ks)[0] == m.table.get(ks)[0]).all(), "%s: the values" % what
    rows = min(len(m.iterations), 64)
    for name in ('offered', 'improved', 'expanded', 'overflow'):
        assert getattr(st, name).tolist() == [r[name] for r in m.iterations[-rows:]] if rows else len(getattr(st, name)) == 0, "%s: %s" % (what, name)
    assert st.overflowed == m.overflowed
    XO.assert_rows(pool.state(0, min(m.cursor, pool.capacity)), {k: x[:m.cursor] for k, x in m.rows.items()}, what)
    value, goal_keys = m.goal()
    got = s.goal()
    assert isinstance(got, SearchGoal) and got.value == value, "%s: the goal's value" % what
    assert got.bucket == (min(table.lookup(np.array(sorted(goal_keys), np.uint64)).tolist()) if goal_keys else -1), "%s: the goal's bucket" % what
    if flags is not None:
        assert st.flags == flags and v.error_flags() == flags, what
    return st


# ------------------------------------------------------------------ 1. against the CPU oracle, iteration by iteration
def test_against_the_cpu_oracle_iteration_by_iteration(venv):
    """s.run(1) four times beside key_value_oracle.label_correcting with the synthetic costs: after every iteration the stored keys, every
    key's value, the improved count and the cursor agree; a stored state was reopened."""
    v, n, A = venv, venv.num_envs, venv.n_actions
    costs = KV.synthetic_costs(v.spec)
    cpu = KV.label_correcting(v.spec, v.get_state(), costs, 4)
    pool, table = pool_of_envs(v)
    s = pool.search(table, CAP, costs=costs)
    assert isinstance(s, Search) and tuple(s.parents.shape) == (CAP,) and tuple(s.g.shape) == tuple(s.bucket.shape) == (CAP_POOL,)
    assert (host(s.parents) == IDX_NONE).all() and (host(s.g) == VALUE_NONE).all() and (host(s.bucket) == -1).all()
    assert s.goal() == (VALUE_NONE, -1) and s.stats().iterations == 0
    s.reset_cursor(n)
    s.start(np.arange(n))
    model, e_keys, _, _ = next(cpu)
    assert host(s.parents).tolist() == padded(np.arange(n), CAP).tolist() and host(s.g)[:n].tolist() == [0] * n
    assert (table.lookup(e_keys) == host(s.bucket)[:n]).all() and (table.read(host(s.bucket)[:n])[1] == TAG_ROOT).all()
    cursor = n
    for it in range(4):
        s.run(1)
        model, e_keys, e_values, e_best = next(cpu)
        st = s.stats()
        cursor += int(e_best.sum())
        assert st.iterations == it + 1 and st.improved[-1] == st.expanded[-1] == int(e_best.sum()) and st.cursor == cursor, "iteration %d" % it
        assert st.offered[-1] == len(e_keys) and st.overflow[-1] == 0
        ks = np.array(list(model.held), np.uint64)
        assert len(table) == len(model) and (table.lookup(ks) >= 0).all() and (table.get(ks)[0] == model.get(ks)[0]).all(), "iteration %d: the values" % it
        kids = host(s.parents)
        assert (kids[:st.improved[-1]] == np.arange(cursor - st.improved[-1], cursor)).all() and (kids[st.improved[-1]:] == IDX_NONE).all()
        assert set(KT.as_u64(pool.keys(kids[:st.improved[-1]])).tolist()) == set(e_keys[e_best].tolist()), "iteration %d: the improved states" % it
    assert model.reopened >= n, "no stored state was improved: the costs no longer exercise the reopening"
    assert s.goal() == (VALUE_NONE, -1) and s.stats().flags == 0 and v.error_flags() == 0
    for x in (s, pool, table):
        x.close()
    assert s.closed


# ------------------------------------------------------------------ 2. against the hand-written loop
def test_one_run_of_four_against_the_hand_written_loop(venv):
    """The hand-written loop on one pool and table, s.run(4) as one call on a second pair made with the same first_sequence, and four
    calls of s.run(1) on a third: the same tables, g, buckets' keys, parents and pool rows."""
    v, n = venv, venv.num_envs
    costs = KV.synthetic_costs(v.spec)
    pool_l, table_l = pool_of_envs(v, first_sequence=5)
    loop = hand_loop(v, pool_l, table_l, CAP, np.arange(n), 4, n, costs=costs)
    stats = []
    for calls in ((4,), (1, 1, 1, 1)):
        pool_s, table_s = pool_of_envs(v, first_sequence=5)
        s = pool_s.search(table_s, CAP, costs=costs)
        s.reset_cursor(n)
        s.start(dev(np.arange(n)))
        for k in calls:
            s.run(k)
        stats.append(assert_same_bytes(v, loop, pool_l, table_l, s, pool_s, table_s, 'run%r' % (calls,)))
        assert stats[-1].iterations == 4 and stats[-1].improved.tolist() == [int(it[2].sum()) for it in loop['iterations']]
        for x in (s, pool_s, table_s):
            x.close()
    assert all((a == b).all() for a, b in zip(stats[0][1:5], stats[1][1:5])) and stats[0].cursor == stats[1].cursor
    assert v.error_flags() == 0
    pool_l.close(), table_l.close()


# ------------------------------------------------------------------ 3. roots
@pytest.mark.parametrize('count', [0, 1, 63, 64, 65, 'special'])
def test_roots(venv, count):
    """Roots among 72 slots - the envs and every action's child of each, so many slots hold one state -: none, one, a partial wave, the wave
    boundary and one beyond; and a list with IDX_NONE, a slot twice and two slots of one state.  Only the first position of a state is
    expanded.  Start and one iteration against the model."""
    v, n, A = venv, venv.num_envs, venv.n_actions
    pool, table = pool_of_envs(v)
    pool.expand_all(np.arange(n), n)
    n_slots = n + n * A
    keys = pool.keys(np.arange(n_slots))
    if count == 'special':
        twin = next(int(c) for c in range(n, n_slots) if keys[c] == keys[0])               # (a failed action leaves the parent's state)
        roots = np.array([0, IDX_NONE, 5, 0, twin, IDX_NONE, 2], np.int32)
    else:
        roots = (np.arange(count) * 7 % n_slots).astype(np.int32)                          # distinct slots, repeated states
    m = model_of(v, pool, CAP, n_slots)
    s = pool.search(table, CAP)
    s.reset_cursor(n_slots)
    s.start(roots if count == 'special' else dev(roots))
    best = m.start(roots)
    if count == 'special':
        assert best.tolist() == [True, False, True, False, False, False, True] and m.parents[:7] == [0, IDX_NONE, 5, IDX_NONE, IDX_NONE, IDX_NONE, 2]
    elif count >= 63:
        assert 0 < int(best.sum()) < count, "no repeated state among the roots"
    assert_model(v, s, pool, table, m, 'the roots')
    s.run(1)
    m.iterate()
    st = assert_model(v, s, pool, table, m, 'one iteration')
    assert bool(st.flags & F_FRONTIER_FULL) == m.full and not st.flags & ~F_FRONTIER_FULL
    v.error_flags()
    for x in (s, pool, table):
        x.close()


def test_roots_are_refused_on_the_host(venv):
    pool, table = pool_of_envs(venv)
    s = pool.search(table, 8)
    for bad, what in (([CAP_POOL], 'outside'), ([-1], 'outside'), (list(range(9)), 'capacity'), (dev(np.arange(9)), 'capacity'), ([0.5], 'integer')):
        with pytest.raises(ValueError, match=what):
            s.start(bad)
    with pytest.raises(ValueError, match='iterations'):
        s.run(-1)
    assert s.stats().iterations == 0 and venv.error_flags() == 0
    for x in (s, pool, table):
        x.close()


# ------------------------------------------------------------------ 4. full lists
@pytest.mark.parametrize('capacity,cap_pool', [(16, CAP_POOL), (64, 72)])
def test_full_lists(venv, capacity, cap_pool):
    """A frontier smaller than the improved states - the first ones are kept -, and a pool that fills up - IDX_NONE children, nothing
    written past them -: F_FRONTIER_FULL, the model's lists and the hand-written loop's bytes."""
    v, n = venv, venv.num_envs
    costs = KV.synthetic_costs(v.spec)
    pool_l, table_l = pool_of_envs(v, cap_pool)
    loop = hand_loop(v, pool_l, table_l, capacity, np.arange(n), 3, n, costs=costs)
    assert v.error_flags() == F_FRONTIER_FULL
    pool_s, table_s = pool_of_envs(v, cap_pool)
    m = model_of(v, pool_s, capacity, n, costs=costs)
    s = pool_s.search(table_s, capacity, costs=costs)
    s.reset_cursor(n)
    s.start(np.arange(n))
    s.run(3)
    m.start(np.arange(n))
    for _ in range(3):
        m.iterate()
    assert m.full and (capacity < max(r['improved'] for r in m.iterations) or m.cursor == cap_pool)
    assert_same_bytes(v, loop, pool_l, table_l, s, pool_s, table_s, 'full lists')
    st = assert_model(v, s, pool_s, table_s, m, 'full lists', flags=F_FRONTIER_FULL)
    assert st.cursor <= cap_pool and (st.expanded <= capacity).all() and (st.expanded < st.improved).any()
    for x in (s, pool_s, table_s, pool_l, table_l):
        x.close()


# ------------------------------------------------------------------ 5. keep = k
@pytest.mark.parametrize('keep', [1, 8, CAP])
def test_keep(venv, keep):
    """The k cheapest improved states go on: the hand-written loop with fr.select(..., flags=found.best), frontier.select_reference on host
    copies of its values and flags, and the model."""
    v, n, A = venv, venv.num_envs, venv.n_actions
    costs = KV.synthetic_costs(v.spec)
    pool_l, table_l = pool_of_envs(v)
    loop = hand_loop(v, pool_l, table_l, CAP, np.arange(n), 4, n, costs=costs, keep=keep)
    for keys, values, best, p, a, c, parents in loop['iterations']:
        first, second, taken, _, count = select_reference(values, keep, A, parents, best, capacity=CAP)
        assert (first == p).all() and (second == a).all() and count[0] == taken[0] == int((c != IDX_NONE).sum())
    pool_s, table_s = pool_of_envs(v)
    m = model_of(v, pool_s, CAP, n, costs=costs, keep=keep)
    s = pool_s.search(table_s, CAP, costs=costs, keep=keep)
    s.reset_cursor(n)
    s.start(np.arange(n))
    s.run(4)
    m.start(np.arange(n))
    for _ in range(4):
        m.iterate()
    assert_same_bytes(v, loop, pool_l, table_l, s, pool_s, table_s, 'keep=%d' % keep)
    st = assert_model(v, s, pool_s, table_s, m, 'keep=%d' % keep, flags=0)
    assert (st.expanded == np.minimum(st.improved, keep)).all() and ((st.expanded < st.improved).any() or keep == CAP)
    for x in (s, pool_s, table_s, pool_l, table_l):
        x.close()


def test_more_iterations_than_stats_rows(venv):
    """Seventy iterations with keep=8 - the improved count differs from iteration to iteration and never dies out, the model says - read
    after 63, 64, 65 and 70: stats() holds the last min(iterations, 64) rows, oldest first, each what its iteration counted - also the
    oldest one, whose place in the ring the next iteration's row must not have taken."""
    v, n = venv, venv.num_envs
    costs = KV.synthetic_costs(v.spec)
    pool, table = pool_of_envs(v, 1024)
    m = model_of(v, pool, 16, n, costs=costs, keep=8)
    s = pool.search(table, 16, costs=costs, keep=8)
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    for k in (63, 1, 1, 5):
        s.run(k)
        for _ in range(k):
            m.iterate()
        st = assert_model(v, s, pool, table, m, '%d iterations' % len(m.iterations), flags=0)
        assert len(st.improved) == min(len(m.iterations), 64) and (st.offered > 0).all() and (st.improved > 0).all() and (st.expanded == 8).all()
    assert len(m.iterations) == 70 and len({r['improved'] for r in m.iterations}) > 4 and m.iterations[0]['offered'] != m.iterations[6]['offered']
    for x in (s, pool, table):
        x.close()


# ------------------------------------------------------------------ 6. the goal
def goal_state(v):
    """The envs' states with the Pogostick two moves and a craft away: stick 4, plank 2, rubber 1, no crafting table in the inventory; a
    crafting table at (4, 4), the agent at (3, 3) facing EAST: Forward, Right faces it from (3, 4) - and Right, Forward, Left from (4, 3), one
    move later and dearer, a second goal state."""
    S, ids, st = v.map_size, v.spec.items_id, v.get_state()
    m = st['map'].reshape(v.num_envs, S, S)
    m[:, 3, 3] = m[:, 3, 4] = m[:, 4, 3] = 0
    m[:, 4, 4] = ids['crafting_table']
    st['loc'][:], st['facing'][:], st['inv'][:] = [3, 3], 3, 0
    for name, q in (('stick', 4), ('plank', 2), ('rubber', 1)):
        st['inv'][:, ids[name]] = q
    return st


@pytest.fixture(scope='module')
def goal_env():
    spec = make_spec(T.POGO, S_SMALL)
    v = VecNovelGridworld(spec=spec, num_envs=4, seed=XO.good_seed(spec, 4))
    v.reset()
    st = goal_state(v)
    v.set_state(0, map=st['map'], loc=st['loc'], facing=st['facing'], inv=st['inv'], selected=st['selected'], step_count=st['step_count'])
    yield v
    v.close()


@pytest.mark.parametrize('stop', [False, True])
def test_goal(goal_env, stop):
    """The real step costs from two roots, four iterations.  On the model first: the goal is reached, by offers of different cost.  Then the
    device: goal() is the model's cheapest (value, bucket of that key); the traced plan, rolled out from its root, ends in a goal and costs
    no more than the stored value.  stop_at_goals: no parent list ever holds an ended state, and the table still holds the goal's key."""
    import torch
    v, A = goal_env, goal_env.n_actions
    roots = np.arange(2)
    pool, table = pool_of_envs(v)
    m = model_of(v, pool, CAP, v.num_envs, scale=1, stop_at_goals=stop)
    m.start(roots)
    for _ in range(4):
        m.iterate()
    value, goal_keys = m.goal()
    assert value != VALUE_NONE and len({x for x, _ in m.goals}) >= 2 and value == min(x for x, _ in m.goals), "the state no longer exercises the goal's minimum"
    assert not m.full
    s = pool.search(table, CAP, scale=1, stop_at_goals=stop)
    s.reset_cursor(v.num_envs)
    s.start(roots)
    for it in range(4):
        s.run(1)
        if stop:                                                                          # no ended state among the parents
            kids = host(s.parents)
            kids = kids[kids != IDX_NONE]
            if len(kids):
                assert not (pool.state(int(kids.min()), int(kids.max() - kids.min() + 1))['inv'][:, v.spec.items_id['pogo_stick']] > 0).any()
    assert_model(v, s, pool, table, m, 'goal, stop=%r' % stop, flags=0)
    goal = s.goal()
    assert goal.value == value and (table.lookup(np.array(sorted(goal_keys), np.uint64)) >= 0).all()
    tr = s.goal_plan(8, device=True)
    assert isinstance(tr, Trace) and tuple(tr.plans.shape) == (8, 1) and int(tr.length[0]) == 3
    root_slot = int(np.flatnonzero(host(s.bucket)[:2] == int(tr.root[0]))[0])
    ends = v.snapshot(2)
    r = ends.rollout(dev([root_slot]), tr.plans, children=dev([0]), source=pool, limits=tr.length.clamp(0, 8), device=True)
    assert bool(r.goal[0]) and int(r.length[0]) == 3
    assert int(KT.as_u64(ends.keys([0]))[0]) in goal_keys
    cost, src, slot = 0, pool, root_slot                                                    # the plan's cost, step by step
    for i, a in enumerate(host(tr.plans)[:3, 0].tolist()):
        e = ends.expand([slot], [a], [i % 2], source=src)
        cost += int(step_cost_values(e.info)[0])
        src, slot = ends, i % 2
    assert bool(e.goal[0]) and cost <= goal.value
    assert v.error_flags() == 0
    for x in (ends, s, pool, table):
        x.close()


# ------------------------------------------------------------------ 7. saturation
def test_saturation(venv):
    """Roots started by hand at g = VALUE_NONE - 10 with costs 1, 10 and 11: an offer that would reach or pass VALUE_NONE is none - its key
    is stored and never valued -, and stats() counts it."""
    import torch
    v, n, A = venv, venv.num_envs, venv.n_actions
    costs = np.where(KV.synthetic_costs(v.spec) == 5, 11, KV.synthetic_costs(v.spec)).astype(np.int32)
    pool, table = pool_of_envs(v)
    start = np.full(n, VALUE_NONE - 10, np.int32)
    s = pool.search(table, CAP, costs=costs)
    s.reset_cursor(n)
    keys, found = pool.insert_keys_min(table, np.arange(n), start)                         # the hand-made start, with values given
    assert found.best.all()
    s.g[:n], s.bucket[:n], s.parents[:n] = dev(start), dev(found.where), dev(np.arange(n))
    torch.cuda.synchronize()
    m = model_of(v, pool, CAP, n, costs=costs)
    m.table.insert_min(keys, start, [KV.ROOT] * n)
    m.parents[:n] = list(range(n))
    for r in range(n):
        m.g[r], m.key[r] = int(start[r]), int(keys[r])
    s.run(2)
    for _ in range(2):
        m.iterate()
    st = assert_model(v, s, pool, table, m, 'saturation', flags=0)
    assert st.overflow[0] == n * (A - 1) and st.offered[0] == n and st.overflow[1] > 0 and st.overflowed == int(st.overflow.sum())
    unvalued = [k for k, x in m.table.held.items() if x[0] == VALUE_NONE]
    assert unvalued and (table.get(np.array(unvalued, np.uint64))[0] == VALUE_NONE).all()
    assert max(x[0] for x in m.table.held.values() if x[0] != VALUE_NONE) < VALUE_NONE and min(x[0] for x in m.table.held.values()) >= VALUE_NONE - 10
    for x in (s, pool, table):
        x.close()


# ------------------------------------------------------------------ 8. nothing is committed
def test_nothing_is_committed(venv):
    v, n = venv, venv.num_envs
    before = v.get_state(), v.action_masks(copy=True), v.lookahead(copy=True)
    pool, table = pool_of_envs(v)
    s = pool.search(table, CAP)
    s.reset_cursor(n)
    s.start(np.arange(n))
    s.run(3)
    assert s.stats().iterations == 3
    after = v.get_state(), v.action_masks(copy=True), v.lookahead(copy=True)
    for k in before[0]:
        assert (before[0][k] == after[0][k]).all(), k
    assert (before[1] == after[1]).all() and all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(before[2], after[2]))
    assert v.error_flags() == 0
    for x in (s, pool, table):
        x.close()


# ------------------------------------------------------------------ 9. refusals
def test_refusals(venv):
    v = venv
    pool, table, plain = v.snapshot(64), v.key_table(64, values=True), v.key_table(64)
    with pytest.raises(ValueError, match='without values'):
        pool.search(plain, 16)
    with pytest.raises(ValueError, match='keep'):
        pool.search(table, 16, keep=17)
    with pytest.raises(ValueError, match='capacity'):
        pool.search(table, 65)
    with pytest.raises(ValueError, match='costs'):
        pool.search(table, 16, costs=[1, 2, 3])
    s = pool.search(table, 16, keep=16)
    s.close()
    with pytest.raises(ValueError, match='search is closed'):
        s.run(1)
    s = pool.search(table, 16)
    table.close()
    with pytest.raises(ValueError, match='closed'):
        s.run(1)
    table = v.key_table(64, values=True)
    s = pool.search(table, 16)
    pool.close()
    assert s.closed
    for call in (lambda: s.run(1), lambda: s.start([0]), lambda: s.goal(), lambda: s.stats(), lambda: s.parents, lambda: pool.search(table, 16)):
        with pytest.raises(ValueError, match='closed'):
            call()
    table.close()
    assert v.error_flags() == 0


def test_maps_beyond_the_successor_keys_limit_are_refused():
    big = VecNovelGridworld(spec=make_spec(T.POGO, 36), num_envs=2, seed=4)
    big.reset()
    pool, table = big.snapshot(16), big.key_table(64, values=True)
    with pytest.raises(MapsTooLarge, match='map_size 36'):
        pool.search(table, 8)
    with pytest.raises(_cabi.NgwError):
        pool.search(table, 8)
    big.close()
