"""Search runs on the MI355X across spec classes (csrc/ngw_search.inc, csrc/ngw_abi_search.cpp; search.py, Snapshot.search): the tests of
tests/test_search_run.py, test_best_first.py and test_recipe_heuristic.py drive every run through Pogostick 9 x 9 - 9 items, 17 actions, an odd
S * S, no entity, no Jump, no FireWall, one flagged map item.  Here the same comparisons run over the matrix of tests/test_search_specs_cpu.py:
K in every residue mod 4 (the three load widths of the walk term), A from 15 to 20 (q / A, the tags, the slab layout), dword and 16-byte
maps, an entity, a Jump action, FireWall deaths, recipe programs with no map item and with one rule, a goal and a proof that are not the
Pogostick craft.  Every expectation is the CPU models' (search_oracle, best_first_oracle, recipe_oracle) or walk_heuristic_reference /
recipe_cost_reference of pool.state(); the scenarios, and the facts that keep them from going vacuous, are in the CPU file."""
import numpy as np
import pytest

import key_value_oracle as KV
import test_search_specs_cpu as X
from gym_novel_gridworlds_amd import VecNovelGridworld
from gym_novel_gridworlds_amd import search as S
from gym_novel_gridworlds_amd.key_table import TAG_ROOT, VALUE_NONE
from gym_novel_gridworlds_amd.search import RecipeHeuristic, WalkHeuristic, walk_heuristic_reference
from gym_novel_gridworlds_amd.spec import F_FRONTIER_FULL
from test_best_first import assert_open, run_both, seed_pool
from test_search_run import CAP_TABLE, assert_model, dev, host, pool_of_envs
from test_search_specs_cpu import CAP, CAP_POOL, KEEP, N_ENVS

pytestmark = pytest.mark.gpu
STATE = ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode')


@pytest.fixture(scope='module')
def envs():
    """name -> the env of a matrix row: four envs under the row's seed, made at its first use, put into the CPU oracle's reset states at every
    use (so the CPU file's facts are about these very roots) and with no error flag standing."""
    made = {}

    def get(name):
        spec, seed, st = X.oracle_env(name)
        if name not in made:
            made[name] = VecNovelGridworld(spec=spec, num_envs=N_ENVS, seed=seed)
            made[name].reset()
        v = made[name]
        v.set_state(0, **{k: st[k] for k in STATE})
        v.error_flags()
        return v
    yield get
    for v in made.values():
        v.close()


def flags_of(m):
    return F_FRONTIER_FULL if m.full else 0


def closing(*handles):
    for x in handles:
        x.close()


def assert_tags(v, table, m, what):
    """The table's tags against the model's, free of bucket numbers: behind every stored key the key of the parent whose offer valued it and
    that offer's action (assert_model compares the values alone; tag = bucket * A + a is where A enters)."""
    A, ks = v.n_actions, np.array(list(m.table.held), np.uint64)
    where = table.lookup(ks)
    assert (where >= 0).all() and len(table) == len(ks), "%s: the stored keys" % what
    value, tag = table.read(where)
    key_of = dict(zip(where.tolist(), ks.tolist()))
    held = {k: (x, None, None) if t == TAG_ROOT else (x, key_of.get(t // A), t % A) for k, x, t in zip(ks.tolist(), value.tolist(), tag.tolist())}
    want = {k: (x, None, None) if t == KV.ROOT else (x,) + tuple(m.links[t]) for k, (x, t) in m.table.held.items()}
    assert held == want, "%s: the tags" % what


def seeded_pool(v, rows, cap_pool=CAP_POOL):
    """A pool whose first slots hold `rows` (through the envs, four at a time), and a valued table."""
    pool, table = v.snapshot(cap_pool), v.key_table(CAP_TABLE, values=True)
    seed_pool(v, pool, rows)
    return pool, table


# ------------------------------------------------------------------ A. closed runs against SearchModel, the whole matrix
@pytest.mark.parametrize('costs', ['real', 'synthetic'])
@pytest.mark.parametrize('keep', [None, KEEP])
@pytest.mark.parametrize('name', list(X.MATRIX))
def test_closed_runs(envs, name, keep, costs):
    """The layered search and the beam under the real and the per-action costs: the roots and each of four iterations against the model -
    parents, g, the key behind every bucket, the table, the pool's rows, the statistics.  No flag but where the model's own lists fill up
    (jump12, layered, synthetic costs, the fourth iteration: the CPU file says why)."""
    v, n = envs(name), N_ENVS
    kw = X.costs_kw(v.spec, costs)
    pool, table = pool_of_envs(v)
    m = X.closed_model(v.spec, pool.state(0, n), n, keep=keep, **kw)
    s = pool.search(table, CAP, keep=keep, **kw)
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    assert_model(v, s, pool, table, m, '%s: the roots' % name, flags=0)
    for it in range(X.ITERATIONS['A']):
        s.run(1)
        m.iterate()
        assert_model(v, s, pool, table, m, '%s, keep %r, %s costs, iteration %d' % (name, keep, costs, it), flags=flags_of(m))
        assert_tags(v, table, m, '%s, keep %r, %s costs, iteration %d' % (name, keep, costs, it))
    assert m.full == ((name, keep, costs) == ('jump12', None, 'synthetic'))
    closing(s, pool, table)


# ------------------------------------------------------------------ B. the open list with the walk heuristic against BestFirstModel
@pytest.mark.parametrize('mode', ['min', 'max'])
@pytest.mark.parametrize('name', X.GROUP_B)
def test_walk_heuristic(envs, name, mode):
    """Weights 20 + k on the item ids with k % 3 != 0: every lane of an int4 / int2 load has a weight of its own.  Five iterations, the open
    list and the chosen slots after each; at the end h of every reached slot against walk_heuristic_reference of the pool's distances."""
    v, n = envs(name), N_ENVS
    heur = WalkHeuristic(X.walk_weights(v.spec), mode)
    pool, table = pool_of_envs(v)
    m = X.walk_model(v.spec, pool.state(0, n), n, mode)
    s = pool.search(table, CAP, scale=1, keep=KEEP, open_list=True, heuristic=heur)
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    assert_open(v, s, pool, table, m, '%s: the roots' % name, flags=0)
    for it in range(X.ITERATIONS['B']):
        taken = run_both(s, m)
        assert_open(v, s, pool, table, m, '%s, %s, iteration %d' % (name, mode, it), flags=0)
        assert host(s.chosen).tolist() == taken[0], "iteration %d: the chosen slots" % it
    reached = np.array(X.reached(m))
    assert (host(s.g)[reached] != VALUE_NONE).all() and len(reached) == m.cursor
    want = walk_heuristic_reference(pool.walk_distances(reached), heur.weights, mode)
    assert host(s.h)[reached].tolist() == want.tolist() and len(set(want.tolist())) > 4
    closing(s, pool, table)


@pytest.mark.parametrize('mode', ['min', 'max'])
@pytest.mark.parametrize('name', X.GROUP_B)
def test_walk_heuristic_of_65_roots(envs, name, mode):
    """The roots kernel's dist + j * K: 65 roots over varied rows, IDX_NONE in place 1, repeated states among them - h and f of the roots
    before any iteration, then one iteration."""
    v = envs(name)
    pool, table = seeded_pool(v, X.varied_rows(name))
    roots = X.roots_65()
    m = X.walk_model(v.spec, pool.state(0, 68), 68, mode)
    s = pool.search(table, CAP, scale=1, keep=KEEP, open_list=True, heuristic=WalkHeuristic(X.walk_weights(v.spec), mode))
    s.reset_cursor(68)
    s.start(dev(roots))
    best = m.start(roots)
    opened = np.flatnonzero(best)
    assert host(s.h).tolist() == m.h and host(s.f).tolist() == m.f and (host(s.f)[roots[opened]] != VALUE_NONE).all()
    want = walk_heuristic_reference(pool.walk_distances(roots[opened]), X.walk_weights(v.spec), mode)
    assert host(s.h)[roots[opened]].tolist() == want.tolist() and len(set(want.tolist())) > 4
    assert_open(v, s, pool, table, m, '%s: 65 roots' % name, flags=0)
    taken = run_both(s, m)
    assert_open(v, s, pool, table, m, '%s: 65 roots, one iteration' % name, flags=0)
    assert host(s.chosen).tolist() == taken[0]
    closing(s, pool, table)


# ------------------------------------------------------------------ C. recipe and recipe + walk against RecipeBestFirstModel
@pytest.mark.parametrize('with_walk', [False, True])
@pytest.mark.parametrize('name', X.GROUP_C)
def test_recipe_heuristic(envs, name, with_walk):
    """The recipe term of the spec's own program - no map item (bow10, jump12), one rule (crate10m), a flagged tap on dword and 16-byte maps -
    as the heuristic of a pruning run: five iterations against the model, then h of every reached slot against recipe_cost_reference of
    pool.state() plus the walk term."""
    v, n = envs(name), N_ENVS
    walk = WalkHeuristic(X.walk_weights(v.spec), 'min') if with_walk else None
    program = S.recipe_program(v.spec, None, 1)
    pool, table = pool_of_envs(v)
    m = X.recipe_model(v.spec, pool.state(0, n), n, walk='min' if with_walk else None, prune=True)
    s = pool.search(table, CAP, scale=1, keep=KEEP, open_list=True, prune=True, heuristic=RecipeHeuristic(walk))
    assert s.recipe == program == m.program
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    assert_open(v, s, pool, table, m, '%s: the roots' % name, flags=0)
    for it in range(X.ITERATIONS['C']):
        taken = run_both(s, m)
        assert_open(v, s, pool, table, m, '%s, iteration %d' % (name, it), flags=0)
        assert host(s.chosen).tolist() == taken[0], "iteration %d: the chosen slots" % it
    reached = np.array(X.reached(m))
    st = pool.state(0, int(reached.max()) + 1)
    want = S.recipe_cost_reference(st['inv'], S.map_item_counts(st['map'], v.n_items), program)[reached].astype(np.int64)
    if with_walk:
        want += walk_heuristic_reference(pool.walk_distances(reached), walk.weights, 'min')
    assert host(s.h)[reached].tolist() == want.tolist()
    assert len(set(want.tolist())) > 1 or (name == 'crate10m' and not with_walk)
    closing(s, pool, table)


# ------------------------------------------------------------------ D. FireWall deaths
@pytest.mark.parametrize('stop', [False, True])
@pytest.mark.parametrize('costs', ['real', 'synthetic'])
@pytest.mark.parametrize('kind', ['open', 'beam'])
def test_firewall_deaths(envs, kind, costs, stop):
    """fire10h: steps that end the episode with message code 14 improve their keys within six iterations (the CPU file counts them).  A
    death is an ended state that is no goal: goal() stays (VALUE_NONE, -1); with stop_at_goals no slot the search handed out holds an ended
    state, without it exactly the model's dead children do."""
    v, n = envs('fire10h'), N_ENVS
    kw = X.costs_kw(v.spec, costs)
    pool, table = pool_of_envs(v)
    if kind == 'open':
        m = X.recipe_model(v.spec, pool.state(0, n), n, walk='min', costs=costs, stop_at_goals=stop)
        s = pool.search(table, CAP, keep=KEEP, open_list=True, stop_at_goals=stop, heuristic=RecipeHeuristic(WalkHeuristic(X.walk_weights(v.spec), 'min')), **kw)
        check = assert_open
    else:
        m = X.closed_model(v.spec, pool.state(0, n), n, keep=KEEP, stop_at_goals=stop, **kw)
        s = pool.search(table, CAP, keep=KEEP, stop_at_goals=stop, **kw)
        check = assert_model
    s.reset_cursor(n)
    s.start(np.arange(n))
    m.start(np.arange(n))
    ended = set()
    for it in range(X.ITERATIONS['D']):
        s.run(1)
        ended |= X.iterate(m)[1]
        check(v, s, pool, table, m, 'deaths, %s, %s costs, stop %r, iteration %d' % (kind, costs, stop, it), flags=0)
    assert X.deaths(m) >= 2
    assert s.goal() == (VALUE_NONE, -1), "a death was taken for a goal"
    cursor = s.stats().cursor
    looks = set(np.flatnonzero(X.looks_ended(v.spec, pool.state(0, cursor))).tolist())
    assert looks == ended and bool(ended) != stop
    closing(s, pool, table)


# ------------------------------------------------------------------ E. a goal, a proof and a plan away from Pogostick
@pytest.mark.parametrize('cfg', sorted(X.BACK))
def test_goal_proof_and_plan(envs, cfg):
    """The state BACK[cfg] steps before the goal of the configuration's golden solved episode as the only root (bow10: the Bow craft 14 steps
    away; axe10: the Pogostick under the axe novelty, 4 steps, the rubber's extract among them): recipe + walk, pruning, stop_at_goals, two
    iterations at a time until proven().  The goal's value is the model's; the traced plan, replayed on the CPU oracle from the root,
    succeeds at every step, ends in a goal and costs exactly that value."""
    v, n = envs(cfg), N_ENVS
    spec, rows = X.solved_episode(cfg)
    at = len(rows['facing']) - 1 - X.BACK[cfg]
    v.set_state(0, **{k: np.repeat(rows[k][at:at + 1], n, axis=0) for k in STATE})
    pool, table = pool_of_envs(v, X.E_POOL)
    m = X.recipe_model(v.spec, pool.state(0, n), n, walk='min', cap_pool=X.E_POOL, keep=X.E_KEEP, stop_at_goals=True, prune=True)
    s = pool.search(table, CAP, scale=1, keep=X.E_KEEP, open_list=True, stop_at_goals=True, prune=True,
                    heuristic=RecipeHeuristic(WalkHeuristic(X.walk_weights(v.spec), 'min')))
    s.reset_cursor(n)
    s.start([0])
    m.start([0])
    while not s.proven():
        assert len(m.iterations) < 40, "no proof within 40 iterations"
        run_both(s, m, 2)
        assert s.proven() == m.proven()
        assert_open(v, s, pool, table, m, '%s, %d iterations' % (cfg, len(m.iterations)), flags=0)
    value, goal_keys = m.goal()
    goal = s.goal()
    assert goal.value == value != VALUE_NONE and not m.full
    tr = s.goal_plan(32)
    length = int(host(tr.length)[0])
    assert 2 <= length <= 32 and int(host(tr.root)[0]) == int(host(s.bucket)[0])
    actions = host(tr.plans)[:length, 0].tolist()
    assert X.replay(v.spec, pool.state(0, 1), actions) == goal.value
    closing(s, pool, table)


# ------------------------------------------------------------------ F. layout residues
@pytest.mark.parametrize('name,capacity', X.GROUP_F)
def test_layout_residues(envs, name, capacity):
    """Lists of 33 to 36 entries with A odd and even: capacity * A takes every residue mod 4, so the weights and the distances behind the
    scratch of capacity * A words are placed after every padding.  As many varied roots as the lists hold, two iterations against the model."""
    v = envs(name)
    pool, table = seeded_pool(v, X.varied_rows(name, 36))
    mode = 'min' if capacity & 1 else 'max'
    m = X.walk_model(v.spec, pool.state(0, capacity), capacity, mode, capacity=capacity, keep=2)
    s = pool.search(table, capacity, scale=1, keep=2, open_list=True, heuristic=WalkHeuristic(X.walk_weights(v.spec), mode))
    s.reset_cursor(capacity)
    s.start(dev(np.arange(capacity)))
    best = m.start(np.arange(capacity))
    assert_open(v, s, pool, table, m, '%s, capacity %d: the roots' % (name, capacity), flags=0)
    for it in range(X.ITERATIONS['F']):
        taken = run_both(s, m)
        assert_open(v, s, pool, table, m, '%s, capacity %d, iteration %d' % (name, capacity, it), flags=flags_of(m))
        assert host(s.chosen).tolist() == taken[0]
    opened = np.array([slot for slot in X.reached(m) if slot >= capacity or best[slot]])    # (a repeated root is valued and never opened: its h stays 0)
    want = walk_heuristic_reference(pool.walk_distances(opened), X.walk_weights(v.spec), mode)
    assert host(s.h)[opened].tolist() == want.tolist() and len(opened) >= 16
    closing(s, pool, table)
