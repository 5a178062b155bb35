"""Open-list search runs on the MI355X (csrc/ngw_search.inc, csrc/ngw_abi_search.cpp, include/ngw.h ngw_search_create_open; search.py,
Snapshot.search(open_list=True)): a best-first search over an open list, held to the model of tests/best_first_oracle.py on the CPU oracle -
f and h of the whole pool, g, the key behind every slot's bucket, the parents and the chosen slots, the table by key, the pool's rows, both
statistics, the goal - and to the layered search it becomes when the whole open list is chosen.  As in tests/test_search_run.py, whose
helpers are used, buckets are compared through the keys they hold."""
import numpy as np
import pytest

import best_first_oracle as BF
import expand_oracle as XO
import key_table_oracle as KT
import key_value_oracle as KV
import ngw_testlib as T
from gym_novel_gridworlds_amd import VecNovelGridworld
from gym_novel_gridworlds_amd.key_table import VALUE_NONE, step_cost_values
from gym_novel_gridworlds_amd.search import OpenStats, WalkHeuristic, priority_reference, walk_heuristic_reference
from gym_novel_gridworlds_amd.snapshot import MapsTooLarge
from gym_novel_gridworlds_amd.spec import F_FRONTIER_FULL, IDX_NONE, make_spec
from test_best_first_cpu import superseding_costs
from test_search_run import CAP, CAP_POOL, CAP_TABLE, assert_model, dev, goal_env, goal_state, host, padded, pool_of_envs, table_by_key, venv  # noqa: F401

pytestmark = pytest.mark.gpu
OPEN_COLUMNS = ('chosen', 'pruned', 'superseded', 'open', 'f_min', 'f_bound')


def model_of(v, pool, capacity, n_slots, keep, **kw):
    m = BF.BestFirstModel(v.spec, capacity, pool.capacity, keep, **kw)
    m.save(pool.state(0, n_slots), np.arange(n_slots))
    m.cursor = n_slots
    return m


def heuristic_of(v, mode, weight=24, items=('crafting_table', 'tree_log', 'wall')):
    """Weights with zeros: `weight` on a few items, 0 elsewhere."""
    w = np.zeros(v.n_items, np.int32)
    w[[v.spec.items_id[name] for name in items if name in v.spec.items_id]] = weight
    assert (w > 0).any() and (w == 0).any()
    return WalkHeuristic(w, mode)


def assert_open(v, s, pool, table, m, what, flags=None):
    """assert_model of tests/test_search_run.py and the open list: f and h over the whole pool, the chosen slots, open_stats()."""
    st = assert_model(v, s, pool, table, m, what, flags)
    assert host(s.f).tolist() == m.f, "%s: f" % what
    assert host(s.h).tolist() == m.h, "%s: h" % what
    os_ = s.open_stats()
    assert isinstance(os_, OpenStats) and os_.iterations == len(m.open_rows), what
    rows = m.open_rows[-64:]
    for name in OPEN_COLUMNS:
        assert getattr(os_, name).tolist() == [r[name] for r in rows], "%s: %s" % (what, name)
    assert s.proven() == m.proven(), "%s: proven" % what
    return st, os_


def run_both(s, m, iterations=1):
    """One run on the device, the same iterations on the model -> the parent lists the model expanded (IDX_NONE where pruned)."""
    s.run(iterations)
    taken = []
    for _ in range(iterations):
        before = len(m.expanded_slots)
        m.iterate()
        taken.append([p if p in m.expanded_slots[before:] else IDX_NONE for p in m.chosen])
    return taken


# ------------------------------------------------------------------ 1. iteration by iteration against the model
@pytest.mark.parametrize('costs', ['real', 'synthetic'])
def test_iteration_by_iteration_against_the_model(venv, costs):
    v, n = venv, venv.num_envs
    kw = dict(scale=1) if costs == 'real' else dict(costs=KV.synthetic_costs(v.spec))
    pool, table = pool_of_envs(v)
    m = model_of(v, pool, CAP, n, 8, **kw)
    s = pool.search(table, CAP, keep=8, open_list=True, **kw)
    assert tuple(s.f.shape) == tuple(s.h.shape) == (CAP_POOL,) and (host(s.f) == VALUE_NONE).all() and not host(s.h).any()
    assert s.open_stats().iterations == 0 and len(s.open_stats().chosen) == 0 and not s.proven()
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    assert (host(s.parents) == IDX_NONE).all() and host(s.f)[:n].tolist() == [0] * n
    assert_open(v, s, pool, table, m, 'the roots', flags=0)
    for it in range(6):
        taken = run_both(s, m)
        assert_open(v, s, pool, table, m, '%s costs, iteration %d' % (costs, it), flags=0)
        assert host(s.chosen).tolist() == taken[0], "iteration %d: the chosen slots" % it
    assert sum(r['chosen'] for r in m.open_rows) > 8 + n and max(r['open'] for r in m.open_rows) > 8, "the open list never held more than one iteration chose"
    # the same six iterations from one call, on a second pool and table: the same end state
    pool2, table2 = pool_of_envs(v)
    s2 = pool2.search(table2, CAP, keep=8, open_list=True, **kw)
    s2.reset_cursor(n)
    s2.start(dev(np.arange(n)))
    s2.run(6)
    assert_open(v, s2, pool2, table2, m, 'run(6)', flags=0)
    assert host(s2.chosen).tolist() == host(s.chosen).tolist()
    for x in (s, pool, table, s2, pool2, table2):
        x.close()


# ------------------------------------------------------------------ 2. the layered search recovered
def test_the_whole_open_list_is_the_layered_search(venv):
    """open_list=True with keep=capacity, no heuristic, no pruning, beside pool.search(table2, CAP): every open state is a child of the last
    iteration, so both expand the same parents in the same order and allocate the children in the same ascending position order - the
    tables by key, g and the pool's rows agree slot for slot after the start and after every iteration.  The open run's parents are chosen
    in run(), so the slots open iteration i + 1 chose are the closed run's parents after iteration i."""
    v, n, A = venv, venv.num_envs, venv.n_actions
    costs = KV.synthetic_costs(v.spec)
    pool_o, table_o = pool_of_envs(v)
    pool_c, table_c = pool_of_envs(v)
    so = pool_o.search(table_o, CAP, costs=costs, keep=CAP, open_list=True)
    sc = pool_c.search(table_c, CAP, costs=costs)
    seen, cursor = [pool_o.keys(np.arange(n))], n
    for s in (so, sc):
        s.reset_cursor(n)
        s.start(np.arange(n))
    for it in range(5):
        if it:
            before = host(sc.parents).copy()
            so.run(1), sc.run(1)
            assert host(so.chosen).tolist() == before.tolist(), "iteration %d: the open run chose other slots than the layered run expanded" % it
            seen.append(host(pool_o.successor_keys(np.arange(cursor)).keys).reshape(-1))       # every slot handed out before this iteration is expanded by now
        cursor = sc.stats().cursor
        assert so.stats().cursor == cursor
        seen.append(pool_o.keys(np.arange(cursor)))
        keys = np.unique(np.concatenate([KT.as_u64(k) for k in seen]))
        assert table_by_key(table_o, keys, A)[0] == table_by_key(table_c, keys, A)[0], "iteration %d: the tables" % it
        assert (host(so.g) == host(sc.g)).all(), "iteration %d: g" % it
        XO.assert_rows(pool_o.state(0, cursor), pool_c.state(0, cursor), 'iteration %d' % it)
        assert (host(so.parents) == host(sc.parents)).all() or it == 0
        open_slots = np.flatnonzero(host(so.f) != VALUE_NONE)
        assert open_slots.tolist() == sorted(p for p in host(sc.parents).tolist() if p != IDX_NONE), "iteration %d: the open list is the layered frontier" % it
    assert so.stats().improved.tolist() == sc.stats().improved.tolist() and so.open_stats().superseded.sum() > 0
    assert v.error_flags() == 0
    for x in (so, sc, pool_o, table_o, pool_c, table_c):
        x.close()


# ------------------------------------------------------------------ 3. the heuristic
@pytest.mark.parametrize('mode', ['min', 'max'])
def test_walk_heuristic(venv, mode):
    v, n = venv, venv.num_envs
    heur = heuristic_of(v, mode)
    pool, table = pool_of_envs(v)
    m = model_of(v, pool, CAP, n, 8, scale=1, heuristic=heur)
    s = pool.search(table, CAP, scale=1, keep=8, open_list=True, heuristic=heur)
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    for it in range(3):
        taken = run_both(s, m)
        assert host(s.chosen).tolist() == taken[0], "iteration %d: the order of expansion" % it
    assert_open(v, s, pool, table, m, 'heuristic %s' % mode, flags=0)
    g, f, h = host(s.g), host(s.f), host(s.h)
    reached = np.flatnonzero(g != VALUE_NONE)
    assert len(reached) == m.cursor and (h[reached] == walk_heuristic_reference(pool.walk_distances(reached), heur.weights, mode)).all() and h[reached].any()
    open_slots = f != VALUE_NONE
    assert (f[open_slots] == priority_reference(g[open_slots], h[open_slots])).all() and open_slots.sum() == sum(x != VALUE_NONE for x in m.f) > 0
    assert not open_slots[g == VALUE_NONE].any() and v.error_flags() == 0
    for x in (s, pool, table):
        x.close()


# ------------------------------------------------------------------ 4. widths around the wavefront
@pytest.fixture(scope='module')
def varied_rows(venv):
    """130 different-looking states: the envs saved again and again between a few random committed steps."""
    v, n = venv, venv.num_envs
    keep_state = v.get_state()
    rs = np.random.RandomState(5)
    pool = v.snapshot(136)
    for r in range(34):
        pool.save(envs=np.arange(n), slots=np.arange(n) + r * n)
        v.step(rs.randint(0, v.n_actions, n).astype(np.int32))
    rows = pool.state(0, 136)
    pool.close()
    v.set_state(0, **{k: keep_state[k] for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count')})
    v.error_flags()
    return rows


@pytest.mark.parametrize('keep', [1, 63, 64, 65])
def test_widths_around_the_wavefront(venv, varied_rows, keep):
    """keep below, at and beyond a wavefront with lists of 17 * 65 entries; 1, 64 and 65 roots, among them IDX_NONE and a repeated state -
    its second copy is not opened."""
    v, A = venv, venv.n_actions
    capacity, cap_pool = 17 * 65, 4096
    for count in (1, 64, 65):
        pool, table = v.snapshot(cap_pool), v.key_table(8192, values=True)
        seed_pool(v, pool, varied_rows)
        roots = np.arange(count).astype(np.int32)
        if count > 1:
            roots[1], roots[count - 1] = IDX_NONE, roots[0] + 0                        # a padded root, and slot 0 a second time
        m = model_of(v, pool, capacity, 136, keep, scale=1)
        s = pool.search(table, capacity, scale=1, keep=keep, open_list=True)
        s.reset_cursor(136)
        s.start(dev(roots))
        best = m.start(roots)
        if count > 1:
            assert not best[count - 1] and not best[1]
        assert (host(s.f) != VALUE_NONE).sum() == int(best.sum()) and host(s.f).tolist() == m.f
        for it in range(2 if count == 65 else 1):
            taken = run_both(s, m)
            assert_open(v, s, pool, table, m, 'keep %d, %d roots, iteration %d' % (keep, count, it), flags=0)
            assert host(s.chosen).tolist() == taken[0]
        assert m.open_rows[0]['chosen'] == min(keep, int(best.sum()))
        for x in (s, pool, table):
            x.close()


def seed_pool(v, pool, rows):
    """Slots 0 .. of `pool` := rows, through the envs: set_state four rows at a time, save."""
    n, keep_state = v.num_envs, v.get_state()
    for r in range(len(rows['facing']) // n):
        at = slice(r * n, (r + 1) * n)
        v.set_state(0, **{k: rows[k][at] for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count')})
        pool.save(envs=np.arange(n), slots=np.arange(n) + r * n)
    v.set_state(0, **{k: keep_state[k] for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count')})
    v.error_flags()


# ------------------------------------------------------------------ 5. superseding on the device
def test_superseding(venv):
    """The scenario of tests/test_best_first_cpu.py - Right 1, Left 10, keep=1, one root -: superseded per iteration equals the model's, the
    superseded slot's f is VALUE_NONE and it is never chosen."""
    v, n = venv, venv.num_envs
    costs = superseding_costs(v.spec)
    pool, table = pool_of_envs(v)
    m = model_of(v, pool, CAP, n, 1, costs=costs)
    s = pool.search(table, CAP, costs=costs, keep=1, open_list=True)
    s.reset_cursor(n)
    s.start([0])
    m.start([0])
    chosen, gone = [], set()
    for it in range(8):
        open_before = {slot for slot, x in enumerate(m.f) if x != VALUE_NONE}
        taken = run_both(s, m)
        chosen += [p for p in host(s.chosen).tolist() if p != IDX_NONE]
        gone |= {slot for slot in open_before if m.f[slot] == VALUE_NONE and slot not in taken[0]}
        assert_open(v, s, pool, table, m, 'superseding, iteration %d' % it, flags=0)
    assert sum(r['superseded'] for r in m.open_rows) > 0 and gone, "the scenario no longer supersedes"
    assert (host(s.f)[sorted(gone)] == VALUE_NONE).all() and not gone & set(chosen) and chosen == m.expanded_slots
    for x in (s, pool, table):
        x.close()


# ------------------------------------------------------------------ 6. goal, pruning, proof
@pytest.mark.parametrize('stop', [False, True])
@pytest.mark.parametrize('costs', ['real', 'synthetic'])
def test_goal_pruning_and_proof(goal_env, costs, stop):
    """run(2) until proven(), at most 40 iterations.  Real costs, keep=32: proven() comes with the pool of 512 exhausted (F_FRONTIER_FULL) -
    the craft costs 8400 against 24 to 28 a move, tests/test_best_first_cpu.py says why that is no proof.  Synthetic costs, keep=4, the walk
    heuristic with weight 1: a proof with no state lost.  Either way goal() is the model's, the traced plan ends in a goal at no more than
    the stored value, and two more iterations expand nothing and change neither the table nor the pool."""
    v, A = goal_env, goal_env.n_actions
    real = costs == 'real'
    w = np.zeros(v.n_items, np.int32)
    w[v.spec.items_id['crafting_table']] = 24 if real else 1
    heur = WalkHeuristic(w, 'min')
    kw = dict(scale=1) if real else dict(costs=KV.synthetic_costs(v.spec))
    keep = 32 if real else 4
    pool, table = pool_of_envs(v)
    m = model_of(v, pool, CAP, v.num_envs, keep, prune=True, stop_at_goals=stop, heuristic=heur, **kw)
    s = pool.search(table, CAP, keep=keep, open_list=True, prune=True, stop_at_goals=stop, heuristic=heur, **kw)
    s.reset_cursor(v.num_envs)
    s.start(np.arange(2))
    m.start(np.arange(2))
    while not s.proven():
        assert len(m.iterations) < 40, "no proof within 40 iterations"
        run_both(s, m, 2)
        assert s.proven() == m.proven()
    flags = F_FRONTIER_FULL if m.full else 0
    assert m.full == real
    assert_open(v, s, pool, table, m, 'proven', flags=None)
    value, goal_keys = m.goal()
    goal = s.goal()
    assert goal.value == value != VALUE_NONE and s.stats().flags == flags
    tr = s.goal_plan(16, device=True)
    length = int(tr.length[0])
    assert 0 < length <= 16
    root_slot = int(np.flatnonzero(host(s.bucket)[:2] == int(tr.root[0]))[0])
    ends = v.snapshot(2)
    cost, src, slot = 0, pool, root_slot
    lut = None if real else KV.synthetic_costs(v.spec)
    for i, a in enumerate(host(tr.plans)[:length, 0].tolist()):
        e = ends.expand([slot], [a], [i % 2], source=src)
        cost += int(step_cost_values(e.info)[0]) if real else int(lut[a])
        src, slot = ends, i % 2
    assert bool(e.goal[0]) and cost <= goal.value and int(KT.as_u64(ends.keys([slot]))[0]) in goal_keys
    seen = np.unique(KT.as_u64(pool.keys(np.arange(min(m.cursor, pool.capacity)))))
    before = table_by_key_subset(table, seen), pool.state(0, pool.capacity), len(table)
    for _ in range(2):
        run_both(s, m)
        os_ = s.open_stats()
        assert os_.chosen[-1] - os_.pruned[-1] == 0
    after = table_by_key_subset(table, seen), pool.state(0, pool.capacity), len(table)
    assert before[0] == after[0] and before[2] == after[2]
    XO.assert_rows(after[1], before[1], 'after the proof')
    assert_open(v, s, pool, table, m, 'after the proof', flags=None)
    v.error_flags()
    for x in (ends, s, pool, table):
        x.close()


def table_by_key_subset(table, keys):
    where = table.lookup(keys)
    value, tag = table.read(where[where >= 0])
    return keys[where >= 0].tolist(), value.tolist(), tag.tolist()


# ------------------------------------------------------------------ 7. a full pool, saturation
def test_a_full_pool(venv):
    """A pool with 8 free slots: F_FRONTIER_FULL, the entries beyond are IDX_NONE, f is written only for the children that got a slot."""
    v, n = venv, venv.num_envs
    pool, table = pool_of_envs(v, n + 8)
    costs = KV.synthetic_costs(v.spec)
    m = model_of(v, pool, n + 8, n, 4, costs=costs)
    s = pool.search(table, n + 8, costs=costs, keep=4, open_list=True)
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    run_both(s, m)
    assert m.full and m.cursor == n + 8
    st, _ = assert_open(v, s, pool, table, m, 'a full pool', flags=F_FRONTIER_FULL)
    kids = host(s.parents)
    assert kids[:8].tolist() == list(range(n, n + 8)) and (kids[8:] == IDX_NONE).all() and st.expanded.tolist() == [8] and st.improved[0] > 8
    assert np.flatnonzero(host(s.f) != VALUE_NONE).tolist() == list(range(n, n + 8))       # the roots are closed; only the children with a slot are open
    run_both(s, m)                                                                          # no slot is left: improved children, none written
    st, _ = assert_open(v, s, pool, table, m, 'a full pool, the second iteration', flags=F_FRONTIER_FULL)
    assert (host(s.parents) == IDX_NONE).all() and st.expanded.tolist() == [8, 0] and st.improved[1] > 0
    assert (host(s.f) != VALUE_NONE).sum() == 4                                             # four of the eight were chosen and closed, nothing was opened
    for x in (s, pool, table):
        x.close()


def test_f_saturates(venv):
    """Roots opened by hand at g = VALUE_NONE - 40 under a heuristic of weight 2^30: f clamps to VALUE_NONE - 1, stays a candidate - the
    next iteration chooses it - and does not wrap."""
    import torch
    v, n = venv, venv.num_envs
    heur = heuristic_of(v, 'max', weight=1 << 30)
    pool, table = pool_of_envs(v)
    costs = np.full(v.n_actions, 3, np.int32)
    s = pool.search(table, CAP, costs=costs, keep=2, open_list=True, heuristic=heur)
    s.reset_cursor(n)
    start = np.full(n, VALUE_NONE - 40, np.int32)
    keys, found = pool.insert_keys_min(table, np.arange(n), start)
    s.g[:n], s.bucket[:n], s.f[:n] = dev(start), dev(found.where), dev(start)
    torch.cuda.synchronize()
    s.run(1)
    os_ = s.open_stats()
    assert os_.chosen.tolist() == [2] and os_.open.tolist() == [n] and os_.f_min.tolist() == [VALUE_NONE - 40]
    kids = host(s.parents)
    kids = kids[kids != IDX_NONE]
    g, f, h = host(s.g), host(s.f), host(s.h)
    assert len(kids) and (g[kids] == VALUE_NONE - 37).all() and (h[kids] > 1 << 30).any()
    assert (f[kids] == priority_reference(g[kids], h[kids])).all() and (f[kids][h[kids] > 40] == VALUE_NONE - 1).all() and (f[kids] > 0).all()
    assert host(s.f)[:2].tolist() == [VALUE_NONE, VALUE_NONE]
    s.run(1)                                                                           # the two remaining roots first, then the clamped children
    s.run(1)
    os_ = s.open_stats()
    assert os_.f_bound[-1] == VALUE_NONE - 1 and os_.chosen[-1] == 2 and s.stats().flags == 0
    for x in (s, pool, table):
        x.close()


# ------------------------------------------------------------------ 8. nothing is committed
def test_nothing_is_committed(venv):
    v, n = venv, venv.num_envs
    before = v.get_state(), v.action_masks(copy=True), v.lookahead(copy=True)
    pool, table = pool_of_envs(v)
    s = pool.search(table, CAP, keep=8, open_list=True, heuristic=heuristic_of(v, 'min'), prune=True)
    s.reset_cursor(n)
    s.start(np.arange(n))
    s.run(4)
    assert s.stats().iterations == 4 and s.open_stats().iterations == 4
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
    K = v.n_items
    good = np.ones(K, np.int32)
    for kw, what in ((dict(open_list=True), 'keep'), (dict(open_list=True, keep=0), 'keep'), (dict(open_list=True, keep=17), 'keep'),
                     (dict(open_list=True, keep=4, heuristic=WalkHeuristic(-good, 'min')), 'weights'),
                     (dict(open_list=True, keep=4, heuristic=WalkHeuristic(good[:-1], 'min')), 'weights'),
                     (dict(open_list=True, keep=4, heuristic=WalkHeuristic(good, 'mean')), 'mode'),
                     (dict(keep=4, heuristic=WalkHeuristic(good, 'min')), 'open_list'), (dict(keep=4, prune=True), 'open_list'), (dict(prune=True), 'open_list')):
        with pytest.raises(ValueError, match=what):
            pool.search(table, 16, **kw)
    with pytest.raises(ValueError, match='without values'):
        pool.search(plain, 16, keep=4, open_list=True)
    with pytest.raises(ValueError, match='capacity'):
        pool.search(table, 65, keep=4, open_list=True)
    with pytest.raises(ValueError, match='costs'):
        pool.search(table, 16, costs=[1, 2, 3], keep=4, open_list=True)
    s = pool.search(table, 16, keep=16, open_list=True, heuristic=WalkHeuristic(good, 'max'), prune=True)
    s.close()
    for call in (lambda: s.run(1), lambda: s.open_stats(), lambda: s.proven(), lambda: s.chosen):
        with pytest.raises(ValueError, match='search is closed'):
            call()
    assert s.f is None and s.h is None
    s = pool.search(table, 16, keep=4, open_list=True)
    table.close()
    for call in (lambda: s.run(1), lambda: s.open_stats()):
        with pytest.raises(ValueError, match='closed'):
            call()
    table = v.key_table(64, values=True)
    s = pool.search(table, 16, keep=4, open_list=True)
    pool.close()
    assert s.closed
    for call in (lambda: s.run(1), lambda: s.start([0]), lambda: s.open_stats(), lambda: s.proven(), lambda: pool.search(table, 16, keep=4, open_list=True)):
        with pytest.raises(ValueError, match='closed'):
            call()
    table.close()
    assert v.error_flags() == 0


def test_maps_beyond_the_successor_keys_limit_are_refused():
    big = VecNovelGridworld(spec=make_spec(T.POGO, 36), num_envs=2, seed=4)
    big.reset()
    pool, table = big.snapshot(16), big.key_table(64, values=True)
    with pytest.raises(MapsTooLarge, match='map_size 36'):
        pool.search(table, 8, keep=2, open_list=True)
    big.close()


def test_a_pool_beyond_the_selection_limit_is_refused(venv):
    """A pool of 2^24 + 1 slots (some 2.5 GB of 9 x 9 states): refused by Search and, called directly, by ngw_search_create_open; a closed
    search over the same pool is made."""
    import ctypes as C
    from gym_novel_gridworlds_amd import _cabi
    v = venv
    pool, table = v.snapshot((1 << 24) + 1), v.key_table(64, values=True)
    with pytest.raises(ValueError, match='2\\^24'):
        pool.search(table, 16, keep=4, open_list=True)
    costs = np.zeros(64, np.int32)
    opt = _cabi.SearchOptions(16, _cabi._ptr(costs, np.int32), 0, 4, 0, 0, _cabi.SEARCH_H_NONE, 0, None)
    arrays, out = _cabi.SearchArraysOpen(), C.c_void_p()
    assert _cabi.lib().ngw_search_create_open(v._h, pool._s, table._t, C.byref(opt), C.byref(arrays), C.byref(out)) == _cabi.E_INVALID_ARG and not out
    assert b'2^24' in _cabi.lib().ngw_last_error()
    s = pool.search(table, 16, keep=4)
    s.close()
    pool.close(), table.close()
    small, table = v.snapshot(64), v.key_table(64, values=True)                        # the limit is the pool's, not the capacity's
    s = small.search(table, 16, keep=4, open_list=True)
    for x in (s, small, table):
        x.close()
    assert v.error_flags() == 0


# ------------------------------------------------------------------ 10. the closed forms are untouched
def test_the_closed_forms_have_no_open_list(venv):
    pool, table = pool_of_envs(venv)
    for kw in ({}, dict(keep=8)):
        s = pool.search(table, CAP, **kw)
        assert s.f is None and s.h is None and not s.open_list
        for call in (lambda: s.open_stats(), lambda: s.proven(), lambda: s.chosen):
            with pytest.raises(ValueError, match='open_list'):
                call()
        s.close()
    pool.close(), table.close()
