"""The scenarios of tests/test_search_specs.py without a GPU: the spec matrix the search runs are driven through - its K, A, S and entity
columns -, the weights that tell the lanes of a vector load apart, the varied rows, and for every group the facts that keep its device test
from going vacuous - a reopened state away from A = 17, a heuristic that varies over the reached slots, FireWall deaths that improve their
key, a proof away from Pogostick found in a later iteration, every residue of capacity * A mod 4.  Everything here runs the models of
tests/search_oracle.py, tests/best_first_oracle.py and tests/recipe_oracle.py on the CPU oracle; the device file imports the scenarios from
here, so both look at the same roots, weights and costs."""
import functools

import numpy as np
import pytest

import best_first_oracle as BF
import expand_oracle as XO
import key_value_oracle as KV
import ngw_testlib as T
import recipe_oracle as RO
import search_oracle as SX
import snapshot_oracle as SO
from gym_novel_gridworlds_amd import search as S
from gym_novel_gridworlds_amd.key_table import VALUE_NONE
from gym_novel_gridworlds_amd.novelty import apply_novelty
from gym_novel_gridworlds_amd.spec import IDX_NONE, make_spec
from test_step_plain import ADD4

N_ENVS, CAP, CAP_POOL, KEEP = 4, 256, 512, 8
# name: (S, K, A, n_entities) as spec.compile() gives them, and what the row is there for
MATRIX = {
    'pogo10': (10, 9, 17, 0, 'dword maps, the baseline'),
    'bow10': (10, 9, 15, 0, 'odd A, a recipe program that reads no map byte'),
    'axe10': (10, 10, 18, 1, 'an entity, int2 walk rows'),
    'fire10h': (10, 10, 18, 0, 'FireWall deaths (message code 14)'),
    'jump12': (12, 9, 16, 0, 'a Jump action, 16-byte maps'),
    'add12m': (12, 10, 18, 0, 'an added item, 16-byte maps'),
    'crate10m': (10, 10, 18, 0, 'a recipe program of one rule'),
    'stk_add_axe12': (12, 11, 19, 1, 'K = 3 mod 4, a stack of two novelties, an entity'),
    'add3_12': (12, 12, 20, 0, 'int4 walk rows'),
}
GROUP_B = ('pogo10', 'bow10', 'axe10', 'stk_add_axe12', 'add3_12')
GROUP_C = ('bow10', 'crate10m', 'axe10', 'add12m', 'jump12', 'add3_12')
GROUP_F = [(name, capacity) for name in ('bow10', 'axe10') for capacity in (33, 34, 35, 36)]
ITERATIONS = dict(A=4, B=5, C=5, D=6, F=2)
# group E: how many steps before the end of the configuration's first golden solved episode the only root is taken (test_a_proof_on_the_model says how they were chosen)
BACK = {'bow10': 14, 'axe10': 4}
E_KEEP, E_POOL = 8, 1024


def spec_of(name):
    if name != 'add3_12':
        return T.build_spec(name)
    spec = make_spec(T.POGO, 12)
    for nov in ADD4[:3]:
        apply_novelty(spec, *nov)
    return spec


@functools.lru_cache(maxsize=None)
def oracle_env(name):
    """The four envs of a matrix row after a reset on the CPU oracle -> (spec, seed, their states)."""
    from oracle.ngw_oracle import Oracle
    spec = spec_of(name)
    seed = XO.good_seed(spec, N_ENVS)
    o = Oracle(spec.compile(), N_ENVS, seed=seed)
    o.reset()
    return spec, seed, SO.oracle_state(o)


def walk_weights(spec):
    """w[k] = 20 + k for the item ids with k % 3 != 0, 0 elsewhere: no two lanes of a vector load carry the same weight."""
    K = len(spec.items_id)
    return np.array([20 + k if k % 3 else 0 for k in range(K)], np.int32)


@functools.lru_cache(maxsize=None)
def varied_rows(name, count=68, seed=5):
    """`count` different-looking states, as the varied_rows of tests/test_best_first.py are made: the four envs saved again and again between
    random committed steps (three between two saves: most random steps fail), here on the CPU oracle."""
    from oracle.ngw_oracle import Oracle
    spec, sd, _ = oracle_env(name)
    o = Oracle(spec.compile(), N_ENVS, seed=sd)
    o.reset()
    rs, A, seen = np.random.RandomState(seed), spec.compile().n_actions, []
    for _ in range(count // N_ENVS):
        seen.append(SO.oracle_state(o))
        for _ in range(3):
            o.step(rs.randint(0, A, N_ENVS).astype(np.int32))
    return RO.concat(seen)


def roots_65():
    """65 roots over the varied rows with IDX_NONE in place 1."""
    roots = np.arange(65).astype(np.int32)
    roots[1] = IDX_NONE
    return roots


def costs_kw(spec, costs):
    return dict(scale=1) if costs == 'real' else dict(costs=KV.synthetic_costs(spec))


def seeded(m, rows, n_slots):
    m.save({k: x[:n_slots] for k, x in rows.items()}, np.arange(n_slots))
    m.cursor = n_slots
    return m


def closed_model(spec, rows, n_slots, capacity=CAP, cap_pool=CAP_POOL, **kw):
    return seeded(SX.SearchModel(spec, capacity, cap_pool, **kw), rows, n_slots)


def walk_model(spec, rows, n_slots, mode, capacity=CAP, cap_pool=CAP_POOL, keep=KEEP, **kw):
    return seeded(BF.BestFirstModel(spec, capacity, cap_pool, keep, scale=1, heuristic=(walk_weights(spec), mode), **kw), rows, n_slots)


def recipe_model(spec, rows, n_slots, walk=None, capacity=CAP, cap_pool=CAP_POOL, keep=KEEP, costs='real', **kw):
    """walk: None or a mode - the recipe term of the spec's own program under the search's costs, plus the walk term of walk_weights."""
    kw.update(costs_kw(spec, costs))
    program = S.recipe_program(spec, kw.get('costs'), kw.get('scale', 1))
    return seeded(RO.RecipeBestFirstModel(spec, capacity, cap_pool, keep, program, walk=None if walk is None else (walk_weights(spec), walk), **kw), rows, n_slots)


def reached(m):
    return [slot for slot in range(m.pool_capacity) if m.g[slot] != VALUE_NONE]


def deaths(m):
    """The improving offers of a model's iterations whose step ended the episode with message code 14."""
    return sum(1 for r in m.iterations for w in r['info'][r['best']].tolist() if (w >> 1) & 1 and (w >> 8) & 255 == 14)


def iterate(m):
    """One iteration of a closed or an open-list model -> (its record, the slots it wrote whose step reported done)."""
    before = list(m.parents)
    rec = m.iterate()
    lists = m.chosen if hasattr(m, 'chosen') else before
    ended = {c for p, a, c in rec['pairs'] if c != IDX_NONE and (int(rec['info'][lists.index(p) * m.A + a]) >> 1) & 1}
    return rec, ended


def looks_ended(spec, rows):
    """bool [n]: the rows an ended step leaves under a FireWall spec, told from the state alone - the goal item held, or the agent beside a
    fire cell (the oracle's FireWall check after every step).  test_deaths_on_the_model holds it to the steps' own done bits."""
    cs, S_ = spec.compile(), spec.map_size
    m = np.asarray(rows['map']).reshape(-1, S_, S_)
    loc = np.asarray(rows['loc']).reshape(-1, 2)
    i, r, c = np.arange(len(m)), loc[:, 0], loc[:, 1]
    fire = int(cs.fire_item)
    beside = (m[i, r - 1, c] == fire) | (m[i, r + 1, c] == fire) | (m[i, r, c - 1] == fire) | (m[i, r, c + 1] == fire)
    return beside | (np.asarray(rows['inv']).reshape(len(m), -1)[:, int(cs.goal_item)] > 0)


def solved_episode(cfg, k=0):
    """The states of the configuration's k-th golden solved episode, its start first and its goal state last (the recording goes on for a few
    steps behind the first done: those are left out) -> (spec, rows)."""
    spec, rows = RO.solved_states(cfg)
    g, n = T.golden(cfg), T.spec_json()['cfgs'][cfg]['n_solved']
    lens = [len(g['so%d_action' % i]) for i in range(n)]
    at, first = [k], n
    for t in range(int(np.flatnonzero(g['so%d_done' % k])[0]) + 1):
        alive = [i for i in range(n) if t < lens[i]]
        at.append(first + alive.index(k))
        first += len(alive)
    return spec, {key: x[at] for key, x in rows.items()}


def proof_model(cfg, back):
    """Group E's search on the model: the state `back` steps before the end of the golden solved episode as the only root, recipe + walk ('min'),
    real costs, keep 8, stop_at_goals, prune, two iterations at a time until proven() or 40 -> (the model, the iteration that first found a goal)."""
    spec, rows = solved_episode(cfg)
    n = len(rows['facing'])
    root = {k: np.repeat(x[n - 1 - back:n - back], N_ENVS, axis=0) for k, x in rows.items()}
    m = recipe_model(spec, root, N_ENVS, walk='min', cap_pool=E_POOL, keep=E_KEEP, stop_at_goals=True, prune=True)
    m.start(np.arange(1))
    found = None
    while not m.proven() and len(m.iterations) < 40:
        for _ in range(2):
            m.iterate()
            if found is None and m.goal()[0] != VALUE_NONE:
                found = len(m.iterations)
    return m, found


# ------------------------------------------------------------------ the matrix
def test_the_matrix_columns():
    """S, K, A and n_entities of every row as spec.compile() gives them; the K values cover all four residues mod 4 - the three load widths of
    the walk term and both odd forms -, the A values are not all 17, one spec has a Jump action and one a FireWall."""
    from gym_novel_gridworlds_amd.spec import ACT_JUMP
    for name, (size, K, A, n_entities, _) in MATRIX.items():
        spec = spec_of(name)
        cs = spec.compile()
        assert (spec.map_size, int(cs.n_items), int(cs.n_actions), int(cs.n_entities)) == (size, K, A, n_entities), name
        assert len(spec.items_id) == K and len(spec.actions_id) == A, name
    assert {row[1] % 4 for row in MATRIX.values()} == {0, 1, 2, 3}
    assert {row[2] for row in MATRIX.values()} == {15, 16, 17, 18, 19, 20}
    assert {row[0] for row in MATRIX.values()} == {10, 12}
    kinds = lambda name: [int(spec_of(name).compile().act_kind[a]) for a in range(MATRIX[name][2])]      # noqa: E731
    assert ACT_JUMP in kinds('jump12') and ACT_JUMP not in kinds('pogo10')
    assert int(spec_of('fire10h').compile().fire_item) and not int(spec_of('pogo10').compile().fire_item)
    assert set(GROUP_B) | set(GROUP_C) | {'fire10h'} == set(MATRIX)


# ------------------------------------------------------------------ A. closed runs
def closed_run(name, keep, costs):
    spec, _, st = oracle_env(name)
    m = closed_model(spec, st, N_ENVS, keep=keep, **costs_kw(spec, costs))
    m.start(np.arange(N_ENVS))
    for _ in range(ITERATIONS['A']):
        m.iterate()
    return m


def test_closed_runs_on_the_model():
    """Every closed run of group A expands something in every iteration and keeps the table of 2048 far from full; with the synthetic costs a
    stored state is reopened on every spec, those with A != 17 among them; the beam drops improved states.  One run fills its lists: the
    layered search of jump12 under the synthetic costs improves 269 states in its fourth iteration, 13 more than the 256 entries - the device
    raises F_FRONTIER_FULL there and nowhere else."""
    full = []
    for name in MATRIX:
        for keep in (None, KEEP):
            for costs in ('real', 'synthetic'):
                m = closed_run(name, keep, costs)
                assert all(r['expanded'] > 0 for r in m.iterations) and len(m.table) < 1024 and m.cursor <= CAP_POOL, (name, keep, costs)
                assert costs == 'real' or m.table.reopened > 0, (name, keep)
                assert keep is None or any(r['expanded'] < r['improved'] for r in m.iterations), (name, costs)
                full += [(name, keep, costs)] if m.full else []
    assert full == [('jump12', None, 'synthetic')]


# ------------------------------------------------------------------ B. the walk heuristic
@pytest.mark.parametrize('name', GROUP_B)
def test_the_weights_tell_the_lanes_apart(name):
    spec = spec_of(name)
    w = walk_weights(spec)
    positive = [k for k in range(len(w)) if w[k] > 0]
    assert {k % 4 for k in positive} == {0, 1, 2, 3} and (w == 0).any() and len(set(w[positive].tolist())) == len(positive)
    assert {k % 2 for k in positive} == {0, 1}


@pytest.mark.parametrize('mode', ['min', 'max'])
@pytest.mark.parametrize('name', GROUP_B)
def test_the_walk_term_varies_on_the_model(name, mode):
    """Over the slots five iterations reach h takes more than 4 values, and the item that gives the term is not the same for all of them - a
    swapped pair of lanes changes some h."""
    from gym_novel_gridworlds_amd.walk import shortest_walk
    spec, _, st = oracle_env(name)
    w = walk_weights(spec)
    m = walk_model(spec, st, N_ENVS, mode)
    m.start(np.arange(N_ENVS))
    for _ in range(ITERATIONS['B']):
        m.iterate()
    assert not m.full and len({m.h[slot] for slot in reached(m)}) > 4
    arg = set()
    for slot in reached(m):
        loc = m.rows['loc'][slot].reshape(-1)
        dist = shortest_walk(m.rows['map'][slot], (int(loc[0]), int(loc[1]), int(m.rows['facing'][slot])), spec).dist
        terms = [(int(w[k]) * int(dist[k]), k) for k in range(len(w)) if w[k] > 0 and dist[k] >= 0]
        assert BF.heuristic_of(dist, w, mode) == m.h[slot]
        arg.add((max if mode == 'max' else min)(terms)[1])
    assert len(arg) > 1


@pytest.mark.parametrize('name', GROUP_B)
def test_the_65_roots_on_the_model(name):
    """The 65 roots over the varied rows: several states, repeated ones that are not opened, h of the opened ones not constant and opened roots
    beyond the first wave's first rows."""
    spec, _, _ = oracle_env(name)
    rows = varied_rows(name)
    assert len(rows['facing']) == 68
    m = walk_model(spec, rows, 68, 'max')
    best = m.start(roots_65())
    opened = np.flatnonzero(best)
    assert 8 <= len(opened) < 64 and not best[1] and opened.max() >= 32
    assert len({m.h[r] for r in opened.tolist()}) > 4


# ------------------------------------------------------------------ C. the recipe term
def test_the_recipe_programs_of_group_c():
    programs = {name: S.recipe_program(spec_of(name), None, 1) for name in GROUP_C}
    assert programs['bow10'].map_items == 0 and programs['jump12'].map_items == 0 and len(programs['bow10'].rules) == 5
    assert len(programs['crate10m'].rules) == 1 and programs['crate10m'].map_items == 0
    for name in ('axe10', 'add12m', 'add3_12'):
        assert bin(programs[name].map_items).count('1') == 1 and len(programs[name].rules) == 6, name


@pytest.mark.parametrize('with_walk', [False, True])
@pytest.mark.parametrize('name', GROUP_C)
def test_the_recipe_term_varies_on_the_model(name, with_walk):
    spec, _, st = oracle_env(name)
    m = recipe_model(spec, st, N_ENVS, walk='min' if with_walk else None, prune=True)
    m.start(np.arange(N_ENVS))
    for _ in range(ITERATIONS['C']):
        m.iterate()
    values = {m.h[slot] for slot in reached(m)}
    assert not m.full and len(reached(m)) > 64
    assert len(values) > 1 or (name == 'crate10m' and not with_walk), "h is constant over the reached slots"


# ------------------------------------------------------------------ D. FireWall deaths
def death_run(kind, costs, stop):
    """kind 'open': an open list with keep 8 under recipe + walk; 'beam': a closed run with keep 8 -> (the model, the ended slots it wrote)."""
    spec, _, st = oracle_env('fire10h')
    if kind == 'open':
        m = recipe_model(spec, st, N_ENVS, walk='min', costs=costs, stop_at_goals=stop)
    else:
        m = closed_model(spec, st, N_ENVS, keep=KEEP, stop_at_goals=stop, **costs_kw(spec, costs))
    m.start(np.arange(N_ENVS))
    ended = set()
    for _ in range(ITERATIONS['D']):
        ended |= iterate(m)[1]
    return spec, m, ended


@pytest.mark.parametrize('stop', [False, True])
@pytest.mark.parametrize('costs', ['real', 'synthetic'])
@pytest.mark.parametrize('kind', ['open', 'beam'])
def test_deaths_on_the_model(kind, costs, stop):
    """Within the six iterations deaths - done with message code 14 - improve their keys (measured: open 2 with the real costs and 3 with the
    synthetic ones under stop, 5 and 6 without; the beam 7 to 22), no goal is reached, nothing is lost; without stop the dead children get
    slots and are expanded, with it none does - and looks_ended tells exactly those slots from their rows."""
    spec, m, ended = death_run(kind, costs, stop)
    assert deaths(m) >= 2 and m.goal() == (VALUE_NONE, set()) and not m.full
    rows = {k: x[:m.cursor] for k, x in m.rows.items()}
    assert set(np.flatnonzero(looks_ended(spec, rows)).tolist()) == ended
    assert bool(ended) != stop
    if kind == 'open' and costs == 'synthetic':
        assert sum(r['superseded'] for r in m.open_rows) >= 1


# ------------------------------------------------------------------ E. a goal, a proof and a plan away from Pogostick
def test_the_chosen_depths():
    assert BACK == {'bow10': 14, 'axe10': 4}


@pytest.mark.parametrize('cfg', sorted(BACK))
def test_a_proof_on_the_model(cfg):
    """BACK[cfg] steps before the goal of the golden solved episode: proven() within 40 iterations with no state lost, the goal first found in
    iteration 2 or later - and one step further back at least one of the three fails, so BACK is the largest such number.  The chain of the
    model's tags from the goal's key, replayed on the CPU oracle from the root: every step succeeds, the last one ends the episode in a goal,
    and the step costs add up to the goal's value."""
    back = BACK[cfg]
    m, found = proof_model(cfg, back)
    assert m.proven() and len(m.iterations) <= 40 and not m.full and found >= 2
    further, found_further = proof_model(cfg, back + 1)
    assert not (further.proven() and not further.full and found_further is not None and found_further >= 2)
    value, keys = m.goal()
    key, acts = min(keys), []
    while m.table.held[key][1] != KV.ROOT:
        key, a = m.links[m.table.held[key][1]]
        acts.append(a)
    assert key == m.key[0] and 2 <= len(acts) <= back + 2
    assert replay(m.spec, {k: x[:1] for k, x in m.rows.items()}, acts[::-1]) == value


def replay(spec, root, actions):
    """The actions from the one row `root` on the CPU oracle: every step succeeds, only the last one is done, with a goal -> the summed real
    step costs at scale 1."""
    lut, rows, cost = SX.step_cost_table(1), KV._rows(root), 0
    for i, a in enumerate(actions):
        rows, rep = XO.oracle_expand(spec, rows, [0], [a])
        rows, w = KV._rows(rows), int(rep['info'][0])
        last = i == len(actions) - 1
        assert w & 1, "step %d (action %d) failed" % (i, a)
        assert bool((w >> 1) & 1) == last and (not last or (w >> 8) & 255 != 14), "step %d: done %d" % (i, (w >> 1) & 1)
        cost += lut[(w >> 2) & 63]
    return cost


# ------------------------------------------------------------------ F. layout residues
def layout_model(name, capacity):
    spec, _, _ = oracle_env(name)
    rows = varied_rows(name, 36)
    m = walk_model(spec, rows, capacity, 'min' if capacity & 1 else 'max', capacity=capacity, keep=2)
    m.start(np.arange(capacity))
    return spec, m


def test_the_layout_residues():
    """capacity * A takes every residue mod 4 over the eight cases, and on the model two iterations open and expand states in each."""
    assert {capacity * MATRIX[name][2] % 4 for name, capacity in GROUP_F} == {0, 1, 2, 3}
    assert {capacity * MATRIX[name][2] % 4 for name, capacity in GROUP_F if name == 'bow10'} == {0, 1, 2, 3}
    for name, capacity in GROUP_F:
        spec, m = layout_model(name, capacity)
        for _ in range(ITERATIONS['F']):
            m.iterate()
        assert all(r['chosen'] == 2 and r['expanded'] > 0 for r in m.iterations) and not m.full, (name, capacity)
        assert len({m.h[slot] for slot in reached(m)}) > 2, (name, capacity)
