"""The recipe heuristic on the MI355X (csrc/ngw_recipe.inc, csrc/ngw_abi_recipe.cpp, include/ngw.h ngw_snapshot_recipe_costs /
ngw_search_set_recipe; search.py RecipeHeuristic, Snapshot.recipe_costs, VecNovelGridworld.recipe_costs).  Every cost is held to
search.recipe_cost_reference of pool.state() / get_state() - never to the kernel's own output -, the search to the model of
tests/recipe_oracle.py on the CPU oracle, iteration by iteration."""
import ctypes as C

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import recipe_oracle as RO
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd import search as S
from gym_novel_gridworlds_amd.key_table import VALUE_NONE
from gym_novel_gridworlds_amd.search import RecipeHeuristic, WalkHeuristic
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, IDX_NONE, make_spec
from test_best_first import OPEN_COLUMNS, assert_open, run_both, seed_pool, varied_rows  # noqa: F401
from test_search_run import CAP, CAP_POOL, dev, host, pool_of_envs, venv  # noqa: F401

pytestmark = pytest.mark.gpu
POGO_V0 = 'NovelGridworld-Pogostick-v0'
STATE = ('map', 'loc', 'facing', 'inv', 'selected', 'step_count')


def reference(v, st, **kw):
    """recipe_cost_reference of get_state()-style rows under the env's spec."""
    return S.recipe_cost_reference(st['inv'], S.map_item_counts(st['map'], v.n_items), S.recipe_program(v.spec, **kw))


def put(v, st, first=0):
    v.set_state(first, **{k: st[k] for k in STATE})


# ------------------------------------------------------------------ 1. specs, sizes and states
@pytest.mark.parametrize('env_id,size', [(T.POGO, 10), (T.POGO, 9), (T.BOW, 12), (POGO_V0, 10), (T.POGO, 64)])
def test_costs_against_the_reference(env_id, size):
    """Fresh resets, states after 20 random valid steps, and - S2 a multiple of 16, of 4, odd - the row tail; the v0 id's pre-placed tap counts."""
    spec = make_spec(env_id, size)
    n = 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, 4))
    v.reset()
    pool = v.snapshot(2 * n)
    pool.save(envs=np.arange(n), slots=np.arange(n))
    fresh = reference(v, pool.state(0, n))
    assert pool.recipe_costs(np.arange(n)).tolist() == fresh.tolist() and v.recipe_costs().tolist() == fresh.tolist()
    if env_id == POGO_V0:
        tap = spec.items_id['tree_tap']
        assert ((v.get_state()['map'] == tap).sum(axis=1) == 1).all() and (fresh == 8400 + 50000).all()      # the pre-placed tap: no tap craft
    elif env_id == T.POGO:
        assert (fresh == 84800).all()
    else:
        assert (fresh == 8400 + 2400 + 1200 + 5000 + 3600).all() and S.recipe_program(spec).map_items == 0
    rs = np.random.RandomState(11)
    for _ in range(20):                                                                # random valid steps (an action that fails changes nothing)
        masks = v.action_masks(copy=True)
        a = np.array([rs.choice(np.flatnonzero(m)) if m.any() else 0 for m in masks], np.int32)
        v.step(a)
    pool.save(envs=np.arange(n), slots=np.arange(n) + n)
    st = pool.state(0, 2 * n)
    want = reference(v, st)
    got = pool.recipe_costs()
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert v.recipe_costs().tolist() == want[n:].tolist() == pool.recipe_costs(from_envs=True).tolist()
    assert v.recipe_costs(scale=3).tolist() == reference(v, v.get_state(), scale=3).tolist()
    assert v.error_flags() == 0
    v.close()


def test_along_a_golden_solved_episode():
    """The states of a golden solved episode of pogo10, put in with set_state on a 10 x 10 env: h falls from 84800 to 0."""
    spec, rows = RO.solved_states('pogo10')
    n = len(rows['facing'])
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset()
    put(v, rows)
    want = reference(v, v.get_state())
    assert v.recipe_costs().tolist() == want.tolist() == RO.costs_of_rows(rows, S.recipe_program(spec)).tolist()
    assert want.max() == 84800 and want.min() == 0 and len(set(want.tolist())) > 8
    v.close()


def test_tap_positions(venv):
    """A tap in the map's first cell and in its last (the row tail of the odd 9 x 9 map), both, one in the inventory as well, and none."""
    v, n, S2 = venv, venv.num_envs, venv.map_size ** 2
    keep = v.get_state()
    st = {k: x.copy() for k, x in keep.items()}
    tap = v.spec.items_id['tree_tap']
    st['inv'][:] = 0
    st['map'][0, 0], st['map'][1, S2 - 1] = tap, tap
    st['map'][2, 0] = st['map'][2, S2 - 1] = st['map'][2, S2 - 2] = tap
    st['map'][3, S2 - 1], st['inv'][3, tap] = tap, 1
    put(v, st)
    want = reference(v, v.get_state())
    assert v.recipe_costs().tolist() == want.tolist() and want.tolist() == [84800 - 7200 - 2400 - 2 * 1200 - 2 * 3600] * 4
    st['map'][3, S2 - 1] = 0                                                           # the last cell of the LAST row cleared: the tap in the inventory remains
    st['inv'][2, tap] = 0
    st['map'][0, 0] = 0                                                                # none at all ...
    st['map'][1, S2 - 1], st['map'][1, 0] = 0, tap                                     # ... and the NEXT row's tap in its first cell: a read past S * S of row 0 would count it
    put(v, st)
    want = reference(v, v.get_state())
    got = v.recipe_costs()
    assert got.tolist() == want.tolist() and got[0] == 84800 and got[3] == got[1] == got[2] < 84800
    assert v.recipe_costs([0]).tolist() == [84800] and v.recipe_costs([0, 0, 1, 0]).tolist() == [84800, 84800, int(want[1]), 84800]
    put(v, keep)
    v.error_flags()


# ------------------------------------------------------------------ 2. index forms
def test_index_forms(venv, varied_rows):
    v = venv
    pool, other = v.snapshot(256), v.snapshot(136)
    seed_pool(v, pool, varied_rows)
    other.copy(np.arange(136), np.arange(136)[::-1].copy(), source=pool)
    want = reference(v, pool.state(0, 136))
    assert len(set(want.tolist())) > 1
    for count in (1, 63, 64, 65):
        slots = (np.arange(count) * 7) % 136
        assert pool.recipe_costs(slots).tolist() == want[slots].tolist(), count
        assert host(pool.recipe_costs(dev(slots), device=True)).tolist() == want[slots].tolist(), count
    rep = np.array([5, 5, 0, 135, 5, 0], np.int32)                                     # repeated slots
    assert pool.recipe_costs(rep).tolist() == want[rep].tolist()
    assert v.error_flags() == 0
    idx = np.array([3, IDX_NONE, 135, IDX_NONE], np.int32)                             # a pair that is not there: 0, no flag
    assert host(pool.recipe_costs(dev(idx), device=True)).tolist() == [want[3], 0, want[135], 0] and v.error_flags() == 0
    idx = np.array([3, 256, -1, 4], np.int32)                                          # out of range: 0 and F_BAD_INDEX
    assert host(pool.recipe_costs(dev(idx), device=True)).tolist() == [want[3], 0, 0, want[4]] and v.error_flags() == F_BAD_INDEX
    with pytest.raises(ValueError):
        pool.recipe_costs([256])
    src_want = reference(v, other.state(0, 136))
    small = v.snapshot(4)
    assert small.recipe_costs(np.arange(136), source=other).tolist() == src_want.tolist()
    assert small.recipe_costs(from_envs=True).tolist() == reference(v, v.get_state()).tolist() == v.recipe_costs(np.arange(v.num_envs)).tolist()
    with pytest.raises(ValueError, match='either'):
        small.recipe_costs(source=other, from_envs=True)
    for x in (small, other, pool):
        x.close()
    assert v.error_flags() == 0


def test_clamping_and_costs(venv):
    """A scale that takes the sum beyond int32 clamps to VALUE_NONE - 1; per-action costs; the refusals of recipe_program reach the caller."""
    v = venv
    assert 84800 * 40000 > VALUE_NONE
    got = v.recipe_costs(scale=40000)
    assert got.tolist() == reference(v, v.get_state(), scale=40000).tolist() == [VALUE_NONE - 1] * v.num_envs
    costs = (np.arange(v.n_actions) * 3 + 1).astype(np.int32)
    assert v.recipe_costs(costs=costs).tolist() == reference(v, v.get_state(), costs=costs).tolist()
    with pytest.raises(ValueError, match='negative'):
        v.recipe_costs(costs=-costs)
    with pytest.raises(ValueError, match='costs'):
        v.recipe_costs(costs=costs[:-1])
    # the C ABI refuses a program that breaks its rules: producers before consumers, a flagged item that a rule consumes
    p = S.recipe_program(v.spec)
    out = dev(np.zeros(4, np.int32))
    bad = p._replace(rules=p.rules[::-1]).struct()
    assert _cabi.lib().ngw_snapshot_recipe_costs(v._h, None, None, 4, C.byref(bad), C.c_void_p(out.data_ptr())) == _cabi.E_INVALID_ARG
    assert b'consumers come first' in _cabi.lib().ngw_last_error()
    bad = p._replace(map_items=1 << v.spec.items_id['plank']).struct()
    assert _cabi.lib().ngw_snapshot_recipe_costs(v._h, None, None, 4, C.byref(bad), C.c_void_p(out.data_ptr())) == _cabi.E_INVALID_ARG
    assert v.error_flags() == 0


@pytest.mark.parametrize('size', [9, 10, 12])
def test_two_and_four_flagged_items(size):
    """Hand-made programs through the C ABI that flag 2 and 4 items (recipe_program never flags more than the tap): a chain of tools, goal <-
    tree_tap <- tree_log <- crafting_table <- wall, each rule's cost a different power of ten, so that h names exactly which of the flagged
    items the kernel found on the map.  Maps with and without each item - the walls' 4 (S - 1) cells fill a 16-bit count well beyond 1 -,
    a tap in the row's last cell, and the row behind an empty one full of everything.  9 x 9, 10 x 10, 12 x 12: the byte tail, dwords, 16-byte pieces."""
    spec = make_spec(T.POGO, size)
    v = VecNovelGridworld(spec=spec, num_envs=8, seed=XO.good_seed(spec, 8))
    v.reset()
    ids, S2 = spec.items_id, size * size
    chain = [ids[name] for name in ('pogo_stick', 'tree_tap', 'tree_log', 'crafting_table', 'wall')]
    rules = tuple(S.RecipeRule(item, 1, 10 ** (4 - i), (), chain[i + 1] if i < 4 else -1) for i, item in enumerate(chain))
    st = v.get_state()
    m = st['map']
    st['inv'][:] = 0
    m[1][m[1] == ids['tree_log']] = 0                                                   # no log
    m[2][(m[2] == ids['tree_log']) | (m[2] == ids['crafting_table'])] = 0               # no log, no table
    m[3][:] = 0                                                                         # nothing at all, not even a wall ...
    m[4][:] = ids['wall']                                                               # ... in front of a row that is all wall
    m[4][:4] = [ids['tree_tap'], ids['tree_log'], ids['crafting_table'], ids['tree_tap']]
    m[5][S2 - 1] = ids['tree_tap']                                                      # a tap in the last cell
    m[6][:] = 0
    m[6][S2 - 1] = ids['crafting_table']                                                # only a table, in the last cell
    m[7][:] = 0
    st['inv'][7, ids['tree_log']] = 1                                                   # nothing on the map, a log held
    put(v, st)
    counts = S.map_item_counts(v.get_state()['map'], v.n_items)
    assert counts[0, ids['wall']] == 4 * (size - 1) and counts[0, ids['tree_tap']] == 0 and counts[0, ids['tree_log']] > 1
    out = dev(np.full(8, -7, np.int32))
    for flagged, by_hand in ((chain[1:], [11000, 11100, 11110, 11111, 10000, 10000, 11100, 11000]),
                             (chain[1:3], [11000, 11111, 11111, 11111, 10000, 10000, 11111, 11000]),
                             ([chain[4], chain[2]], [11000, 11110, 11110, 11111, 11000, 11000, 11111, 11000])):
        program = S.RecipeProgram(chain[0], rules, sum(1 << k for k in flagged))
        assert _cabi.lib().ngw_snapshot_recipe_costs(v._h, None, None, 8, C.byref(program.struct()), C.c_void_p(out.data_ptr())) == 0
        v.sync()
        want = S.recipe_cost_reference(st['inv'], counts, program)
        assert host(out).tolist() == want.tolist() == by_hand, flagged
    five = S.RecipeProgram(chain[0], rules, sum(1 << k for k in chain)).struct()
    assert _cabi.lib().ngw_snapshot_recipe_costs(v._h, None, None, 8, C.byref(five), C.c_void_p(out.data_ptr())) == _cabi.E_INVALID_ARG
    assert b'more than 4' in _cabi.lib().ngw_last_error() and v.error_flags() == 0
    v.close()


def test_nothing_is_committed(venv):
    v, n = venv, venv.num_envs
    before = v.get_state(), v.action_masks(copy=True), v.lookahead(copy=True)
    pool, table = pool_of_envs(v)
    v.recipe_costs(), pool.recipe_costs(), pool.recipe_costs(from_envs=True)
    s = pool.search(table, CAP, keep=8, open_list=True, heuristic=RecipeHeuristic(), prune=True)
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


# ------------------------------------------------------------------ 3. the search, iteration by iteration against the extended model
def walk_of(v):
    w = np.zeros(v.n_items, np.int32)
    w[[v.spec.items_id[name] for name in ('crafting_table', 'tree_log')]] = 24
    return WalkHeuristic(w, 'min')


def model_of(v, pool, capacity, n_slots, keep, walk, **kw):
    m = RO.RecipeBestFirstModel(v.spec, capacity, pool.capacity, keep, S.recipe_program(v.spec, None, 1), walk=None if walk is None else tuple(walk), scale=1, **kw)
    m.save(pool.state(0, n_slots), np.arange(n_slots))
    m.cursor = n_slots
    return m


@pytest.mark.parametrize('with_walk', [False, True])
def test_search_iteration_by_iteration(venv, with_walk):
    v, n = venv, venv.num_envs
    walk = walk_of(v) if with_walk else None
    heur = RecipeHeuristic(walk)
    pool, table = pool_of_envs(v)
    m = model_of(v, pool, CAP, n, 8, walk)
    s = pool.search(table, CAP, scale=1, keep=8, open_list=True, heuristic=heur)
    assert s.recipe == S.recipe_program(v.spec, None, 1)
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    assert_open(v, s, pool, table, m, 'the roots', flags=0)
    assert (host(s.h)[:n] >= 84800).all()
    for it in range(6):
        taken = run_both(s, m)
        assert_open(v, s, pool, table, m, 'iteration %d' % it, flags=0)
        assert host(s.chosen).tolist() == taken[0], it
    reached = np.flatnonzero(host(s.g) != VALUE_NONE)
    want = reference(v, pool.state(0, int(reached.max()) + 1))[reached].astype(np.int64)
    if with_walk:
        want += S.walk_heuristic_reference(pool.walk_distances(reached), walk.weights, 'min')
    assert host(s.h)[reached].tolist() == want.tolist() and len(set(want.tolist())) > 1
    pool2, table2 = pool_of_envs(v)                                                    # the same six iterations from one call
    s2 = pool2.search(table2, CAP, scale=1, keep=8, open_list=True, heuristic=heur)
    s2.reset_cursor(n)
    s2.start(dev(np.arange(n)))
    s2.run(6)
    assert_open(v, s2, pool2, table2, m, 'run(6)', flags=0)
    for x in (s, pool, table, s2, pool2, table2):
        x.close()


@pytest.mark.parametrize('keep,count', [(1, 1), (65, 65), (1, 65), (65, 1)])
def test_search_widths(venv, varied_rows, keep, count):
    v = venv
    capacity, cap_pool = 17 * 65, 4096
    pool, table = v.snapshot(cap_pool), v.key_table(8192, values=True)
    seed_pool(v, pool, varied_rows)
    roots = np.arange(count).astype(np.int32)
    if count > 1:
        roots[1] = IDX_NONE
    walk = walk_of(v)
    m = model_of(v, pool, capacity, 136, keep, walk)
    s = pool.search(table, capacity, scale=1, keep=keep, open_list=True, heuristic=RecipeHeuristic(walk))
    s.reset_cursor(136)
    s.start(dev(roots))
    m.start(roots)
    assert host(s.f).tolist() == m.f and host(s.h).tolist() == m.h
    for it in range(2):
        taken = run_both(s, m)
        assert_open(v, s, pool, table, m, 'keep %d, %d roots, iteration %d' % (keep, count, it), flags=0)
        assert host(s.chosen).tolist() == taken[0]
    for x in (s, pool, table):
        x.close()


@pytest.mark.parametrize('with_walk', [False, True])
def test_proven_and_pruned_on_the_late_stage_scenario(venv, with_walk):
    """The scenario of tests/test_recipe_heuristic_cpu.py under the real costs: proven() with no flag at the goal value 8532 after as many
    expansions as the model makes - 39, where h = 0 needs 616."""
    from test_recipe_heuristic_cpu import EXPANDED, KEEP
    v, n = venv, venv.num_envs
    keep_state = v.get_state()
    put(v, RO.late_stage_state(v.spec, {k: x.copy() for k, x in keep_state.items()}))
    walk = None
    if with_walk:
        w = np.zeros(v.n_items, np.int32)
        w[v.spec.items_id['crafting_table']] = 24
        walk = WalkHeuristic(w, 'min')
    pool, table = pool_of_envs(v, 1024)
    m = model_of(v, pool, CAP, n, KEEP, walk, prune=True)
    s = pool.search(table, CAP, scale=1, keep=KEEP, open_list=True, prune=True, heuristic=RecipeHeuristic(walk))
    s.reset_cursor(n)
    s.start(np.arange(1))
    m.start(np.arange(1))
    while not s.proven():
        assert len(m.iterations) < 40, "no proof within 40 iterations"
        run_both(s, m, 2)
        assert s.proven() == m.proven()
    assert_open(v, s, pool, table, m, 'proven', flags=0)
    os_ = s.open_stats()
    assert s.goal().value == m.goal()[0] == 8532 and s.stats().flags == 0 and not m.full
    assert int((os_.chosen - os_.pruned).sum()) == sum(r['chosen'] - r['pruned'] for r in m.open_rows) == EXPANDED['recipe+walk' if with_walk else 'recipe']
    assert 0 < int(s.goal_plan(16).length[0]) <= 16
    for x in (s, pool, table):
        x.close()
    put(v, keep_state)
    v.error_flags()


def test_set_recipe_refusals(venv):
    v = venv
    pool, table = pool_of_envs(v)
    program = S.recipe_program(v.spec).struct()
    L = _cabi.lib()
    s = pool.search(table, CAP, keep=4, open_list=True, heuristic=RecipeHeuristic())
    s.reset_cursor(v.num_envs)
    s.start([0])
    assert L.ngw_search_set_recipe(v._h, s._s, C.byref(program)) == _cabi.E_INVALID_ARG and b'before ngw_search_start' in L.ngw_last_error()
    closed = pool.search(table, CAP, keep=4)
    assert L.ngw_search_set_recipe(v._h, closed._s, C.byref(program)) == _cabi.E_INVALID_ARG and b'open list' in L.ngw_last_error()
    with pytest.raises(ValueError, match='open_list'):
        pool.search(table, CAP, keep=4, heuristic=RecipeHeuristic())
    plain = pool.search(table, CAP, keep=4, open_list=True)                            # set before the start: legal, twice
    assert L.ngw_search_set_recipe(v._h, plain._s, C.byref(program)) == 0 == L.ngw_search_set_recipe(v._h, plain._s, C.byref(program))
    for x in (s, closed, plain, pool, table):
        x.close()
    assert v.error_flags() == 0


# ------------------------------------------------------------------ 4. the adapter, a wrapper, LimitActions, the sharded env
def adapter_reference(env, spec, **kw):
    """recipe_cost_reference of the adapter's public attributes under `spec`."""
    base = env
    while getattr(base, 'env', None) is not None:                                                      # (through the wrapper stack to the adapter)
        base = base.env
    inv = np.array([base.inventory_items_quantity.get(name, 0) for name in spec.item_names], np.int32)
    counts = S.map_item_counts(np.asarray(base.map).reshape(1, -1), len(inv))[0]
    return int(S.recipe_cost_reference(inv, counts, S.recipe_program(spec, **kw)))


def test_adapter_and_limit_actions():
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    env = T.make_adapter_env('pogo10')
    env.reset()
    spec = make_spec(T.POGO, 10)
    assert isinstance(env.recipe_cost(), int) and env.recipe_cost() == adapter_reference(env, spec) == 84800
    env.inventory_items_quantity['tree_tap'] = 1                                        # an edited attribute reaches the device first
    assert env.recipe_cost() == adapter_reference(env, spec) == 84800 - 7200 - 2400 - 2 * 1200 - 2 * 3600
    env.inventory_items_quantity['tree_tap'] = 0
    names = ['Forward', 'Left', 'Right', 'Break', 'Craft_plank', 'Craft_stick', 'Craft_pogo_stick', 'Extract_rubber']
    lim = LimitActions(env, set(names))
    assert lim.recipe_cost() == 84800 and lim.recipe_cost(scale=2) == 2 * 84800
    costs = np.arange(len(names)).astype(np.int32) + 10                                 # in the limited id space: sorted names
    full = np.zeros(len(spec.actions_id), np.int32)
    for name, c in zip(sorted(names), costs.tolist()):
        full[spec.actions_id[name]] = c
    assert lim.recipe_cost(costs=costs) == adapter_reference(env, spec, costs=full) == env.recipe_cost(costs=full)
    assert lim.recipe_cost(costs=costs) == 12 + 14 + 0 + 2 * 13 + 3 * 11 + 3 * 10      # Craft_tree_tap is not limited: its rule costs 0
    with pytest.raises(ValueError, match='limited'):
        lim.recipe_cost(costs=costs[:-1])
    env.close()


def test_wrappers_pass_through_and_spec_changing():
    """NoveltyWrapper.recipe_cost through an observation wrapper and SaveTrajectories; AxeEasy, BreakIncrease and ExtractIncDec held to
    recipe_cost_reference of their OWN compiled spec, fresh and after steps."""
    import tempfile
    from gym_novel_gridworlds_amd import LidarInFront
    from gym_novel_gridworlds_amd.wrappers import SaveTrajectories
    env = T.make_adapter_env('pogo10')
    spec = make_spec(T.POGO, 10)
    for wrapped in (LidarInFront(env, num_beams=8), SaveTrajectories(env, tempfile.mkdtemp()), LidarInFront(SaveTrajectories(env, tempfile.mkdtemp()))):
        wrapped.reset()
        assert wrapped.recipe_cost() == adapter_reference(env, spec) == 84800
        assert wrapped.recipe_cost(scale=3) == adapter_reference(env, spec, scale=3)
    env.close()
    rs = np.random.RandomState(2)
    for cfg, fresh in (('axeeasy10', 84800 - 3 * 1800), ('brkinc10', 84800 - 3600), ('extdec10', 8400 + 2400 + 1200 + 2 * 5000 + 3600)):
        env, spec = T.make_adapter_env(cfg), T.build_spec(cfg)
        env.reset()
        assert env.recipe_cost() == adapter_reference(env, spec) == fresh, cfg
        for _ in range(25):
            env.step(int(rs.randint(0, len(spec.actions_id))))
            assert env.recipe_cost() == adapter_reference(env, spec), cfg
        env.close()


def test_sharded_env_one_gpu_rehearsal():
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    spec = make_spec(T.POGO, 10)
    sh = ShardedVecNovelGridworld(global_num_envs=16, spec=spec, seed=9)
    sh.reset()
    st = sh.local.get_state()
    want = S.recipe_cost_reference(st['inv'], S.map_item_counts(st['map'], sh.local.n_items), S.recipe_program(spec))
    assert sh.recipe_costs().tolist() == want.tolist() and sh.recipe_costs([1, 0]).tolist() == want[[1, 0]].tolist()
    sh.close()
