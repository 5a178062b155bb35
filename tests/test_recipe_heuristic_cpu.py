"""The recipe heuristic without a GPU (gym_novel_gridworlds_amd/search.py recipe_program, recipe_cost_reference, RecipeHeuristic; include/ngw.h
ngw_snapshot_recipe_costs): the programs of the four base ids, written out by hand for Pogostick-v1 and Bow-v1; the worked example; the
refusals; the numpy reference against the plain-Python statement of tests/recipe_oracle.py; CONSISTENCY - h(s) - h(s') <= cost(s, a) for every
action from every sampled state, h = 0 at every goal state -, which gives admissibility, on the CPU oracle; and the open-list model with the
term: under the REAL costs the recipe and the recipe + walk searches prove the goal h = 0 proves, with fewer expansions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import best_first_oracle as BF
import expand_oracle as XO
import ngw_testlib as T
import recipe_oracle as RO
import snapshot_oracle as SO
from gym_novel_gridworlds_amd import _cabi, search as S
from gym_novel_gridworlds_amd.key_table import VALUE_NONE
from gym_novel_gridworlds_amd.spec import STEP_COSTS, make_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POGO_V0, BOW_V0 = 'NovelGridworld-Pogostick-v0', 'NovelGridworld-Bow-v0'


def named(spec, program):
    """The program with item names: (goal, [(out, out_qty, cost, {input: qty}, tool or None)], [map items])."""
    n = spec.item_names
    rules = [(n[u.out_item], u.out_qty, u.cost, {n[i]: q for i, q in u.inputs}, n[u.tool_item] if u.tool_item >= 0 else None) for u in program.rules]
    return n[program.goal_item], rules, [n[k] for k in range(len(n)) if (program.map_items >> k) & 1]


# ------------------------------------------------------------------ programs
def test_the_pogostick_program_by_hand():
    spec = make_spec(T.POGO, 10)
    goal, rules, on_map = named(spec, S.recipe_program(spec))
    assert goal == 'pogo_stick' and on_map == ['tree_tap']
    assert rules == [('pogo_stick', 1, 8400, {'stick': 4, 'plank': 2, 'rubber': 1}, None),
                     ('rubber', 1, 50000, {}, 'tree_tap'),
                     ('tree_tap', 1, 7200, {'plank': 5, 'stick': 1}, None),
                     ('stick', 4, 2400, {'plank': 2}, None),
                     ('plank', 4, 1200, {'tree_log': 1}, None),
                     ('tree_log', 1, 3600, {}, None)]


def test_the_bow_program_by_hand():
    """The extract consumes a wool BLOCK in front of the agent, not an inventory item: the rule has no input, and wool no rule."""
    spec = make_spec(T.BOW, 12)
    goal, rules, on_map = named(spec, S.recipe_program(spec))
    assert goal == 'bow' and on_map == []
    assert rules == [('bow', 1, 8400, {'stick': 3, 'string': 3}, None),
                     ('stick', 4, 2400, {'plank': 2}, None),
                     ('plank', 4, 1200, {'tree_log': 1}, None),
                     ('string', 4, 5000, {}, None),
                     ('tree_log', 1, 3600, {}, None)]


def test_the_worked_example():
    """Pogostick-v1, empty inventory, no tap on the map: 1 pogo craft, 1 extract, 1 tap craft, 2 stick crafts (demand 5), 3 plank crafts
    (demand 11), 3 tree_log breaks - the total from STEP_COSTS."""
    spec = make_spec(T.POGO, 10)
    program = S.recipe_program(spec)
    cs, ids = spec.compile(), spec.items_id
    craft = {spec.item_names[int(cs.recipe_out_item[r])]: int(round(STEP_COSTS[int(cs.cost_ok[r])])) for r in range(cs.n_recipes)}   # by the spec's cost codes
    extract, brk = int(round(STEP_COSTS[int(cs.ext_cost_ok)])), int(round(STEP_COSTS[int(cs.cost_break)]))
    total = craft['pogo_stick'] + extract + craft['tree_tap'] + 2 * craft['stick'] + 3 * craft['plank'] + 3 * brk
    K = len(spec.items_id)
    empty = np.zeros(K, np.int32)
    assert int(S.recipe_cost_reference(empty, None, program)) == RO.recipe_cost(empty, None, program) == total == 84800
    # a tap on the map or in the inventory: no tap craft, and its planks and stick go - 1 stick craft (demand 4), 1 plank craft (demand 4), 1 break
    less = craft['pogo_stick'] + extract + craft['stick'] + craft['plank'] + brk
    on_map = np.zeros(K, np.int32)
    on_map[spec.items_id['tree_tap']] = 1
    held = empty.copy()
    held[spec.items_id['tree_tap']] = 1
    assert int(S.recipe_cost_reference(empty, on_map, program)) == int(S.recipe_cost_reference(held, None, program)) == less
    on_map[spec.items_id['tree_log']] = 5                                           # logs on the map are not flagged: they count for nothing
    assert int(S.recipe_cost_reference(empty, on_map, program)) == less
    assert int(S.recipe_cost_reference(empty, None, S.recipe_program(spec, scale=2))) == 2 * total
    done = empty.copy()
    done[spec.items_id['pogo_stick']] = 1
    assert int(S.recipe_cost_reference(done, None, program)) == 0


def test_the_v0_ids_give_no_rule_for_items_that_also_lie_on_the_map():
    spec = make_spec(POGO_V0, 10)
    goal, rules, on_map = named(spec, S.recipe_program(spec))
    assert [r[0] for r in rules] == ['pogo_stick', 'rubber', 'tree_tap'] and on_map == ['tree_tap']     # stick and plank: a recipe AND the map
    spec = make_spec(BOW_V0, 10)
    goal, rules, on_map = named(spec, S.recipe_program(spec))
    assert [r[0] for r in rules] == ['bow'] and on_map == []                                            # stick and string likewise


def test_the_branches_for_specs_that_wrappers_change():
    """AxeEasy / AxeMedium: the break rule takes the cheaper of the two break costs; BreakIncrease: break_qty; ExtractIncDec: ext_qty; AddChopAction: a
    second way to the logs, so tree_log has no rule; Crate: its contents have a second source and lose their rules, and what only they demanded."""
    rules = lambda cfg: {r[0]: r for r in named(T.build_spec(cfg), S.recipe_program(T.build_spec(cfg)))[1]}      # noqa: E731
    cs = T.build_spec('axeeasy10').compile()
    assert int(cs.axe_item) and int(round(STEP_COSTS[int(cs.axe_cost)])) == 1800 < int(round(STEP_COSTS[int(cs.cost_break)]))
    assert rules('axeeasy10')['tree_log'] == ('tree_log', 1, 1800, {}, None) == rules('axe10')['tree_log']
    assert rules('brkinc10')['tree_log'] == ('tree_log', 2, 3600, {}, None)
    assert rules('extdec10')['string'] == ('string', 2, 5000, {}, None)
    assert sorted(rules('chop10')) == ['plank', 'pogo_stick', 'rubber', 'stick', 'tree_tap']
    assert sorted(rules('crate10m')) == ['pogo_stick'] and named(T.build_spec('crate10m'), S.recipe_program(T.build_spec('crate10m')))[2] == []


@pytest.mark.parametrize('cfg', ['axeeasy10', 'axe10', 'brkinc10', 'chop10', 'crate10m', 'extdec10'])
def test_consistency_under_spec_changing_wrappers(cfg):
    """The inequality of test_consistency_on_the_cpu_oracle for the committed configurations whose novelty reaches a branch of recipe_program, on
    states after random valid steps and - where the configuration has them - along its golden solved episodes."""
    spec = T.build_spec(cfg)
    rows = RO.random_states(spec, 8, 40, 3)
    if T.spec_json()['cfgs'][cfg]['n_solved']:
        rows = RO.concat([rows, RO.solved_states(cfg)[1]])
    program = S.recipe_program(spec)
    lut, _ = S.cost_table(None, 1, spec.compile().n_actions)
    h, h_after, cost, goal = RO.transitions(spec, rows, program, lut)
    assert (h[None] - h_after <= cost).all() and (h_after[goal] == 0).all() and (h_after != h[None]).any()


def test_costs_by_action_and_refusals():
    spec = make_spec(T.POGO, 10)
    A = spec.compile().n_actions
    costs = np.arange(A).astype(np.int32) + 100
    p = S.recipe_program(spec, costs=costs)
    ids = spec.actions_id
    assert [u.cost for u in p.rules] == [100 + ids[a] for a in ('Craft_pogo_stick', 'Extract_rubber', 'Craft_tree_tap', 'Craft_stick', 'Craft_plank', 'Break')]
    bad = costs.copy()
    bad[ids['Craft_stick']] = -1
    with pytest.raises(ValueError, match='negative'):
        S.recipe_program(spec, costs=bad)
    with pytest.raises(ValueError, match='costs'):
        S.recipe_program(spec, costs=costs[:-1])
    with pytest.raises(ValueError, match='costs'):
        S.recipe_program(spec, costs=costs.astype(np.float32))
    cyclic = make_spec(T.POGO, 10)
    cyclic.recipes['plank'] = {'input': {'stick': 1}, 'output': {'plank': 4}}        # plank <- stick <- plank
    with pytest.raises(ValueError, match='cycle'):
        S.recipe_program(cyclic)


def test_header_binding_and_struct():
    text = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    for name, value in (('RULES', _cabi.RECIPE_MAX_RULES), ('INPUTS', _cabi.RECIPE_MAX_INPUTS), ('MAP_ITEMS', _cabi.RECIPE_MAX_MAP_ITEMS)):
        assert int(re.search(r'#define NGW_RECIPE_MAX_%s (\d+)' % name, text).group(1)) == value
    assert C.sizeof(_cabi.RecipeRule) == 13 * 4 and C.sizeof(_cabi.RecipeProgram) == 16 + 16 * 52
    assert re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', text)
    spec = make_spec(T.POGO, 10)
    p = S.recipe_program(spec).struct()
    assert (p.goal_item, p.n_rules, p.map_items) == (spec.items_id['pogo_stick'], 6, 1 << spec.items_id['tree_tap'])
    assert p.rules[1].tool_item == spec.items_id['tree_tap'] and p.rules[0].tool_item == -1 and p.rules[0].n_in == 3
    L = _cabi.lib()
    assert L.ngw_snapshot_recipe_costs(None, None, None, 0, None, None) == _cabi.E_INVALID_ARG and L.ngw_search_set_recipe(None, None, None) == _cabi.E_INVALID_ARG


# ------------------------------------------------------------------ the reference against the plain statement
def test_the_numpy_reference_against_the_plain_statement():
    rs = np.random.RandomState(7)
    for env_id in (T.POGO, T.BOW, POGO_V0):
        spec = make_spec(env_id, 10)
        K = len(spec.items_id)
        for scale in (1, 3):
            program = S.recipe_program(spec, scale=scale)
            inv = rs.randint(0, 7, (200, K)).astype(np.int32) * (rs.rand(200, K) < 0.4)
            counts = rs.randint(0, 3, (200, K)).astype(np.int32)
            got = S.recipe_cost_reference(inv, counts, program)
            assert got.dtype == np.int32 and got.tolist() == [RO.recipe_cost(inv[i], counts[i], program) for i in range(200)]
            assert S.recipe_cost_reference(inv, None, program).tolist() == [RO.recipe_cost(inv[i], None, program) for i in range(200)]
    # the clamp: a scale that takes the sum beyond int32
    spec = make_spec(T.POGO, 10)
    big = S.recipe_program(spec, scale=40000)
    empty = np.zeros(len(spec.items_id), np.int32)
    assert 84800 * 40000 > VALUE_NONE and int(S.recipe_cost_reference(empty, None, big)) == RO.recipe_cost(empty, None, big) == VALUE_NONE - 1
    maps = np.array([[0, 7, 7, 1], [2, 2, 2, 2]], np.int8)
    assert S.map_item_counts(maps, 9).tolist() == [[1, 1, 0, 0, 0, 0, 0, 2, 0], [0, 0, 4, 0, 0, 0, 0, 0, 0]]


# ------------------------------------------------------------------ consistency, which gives admissibility
@pytest.fixture(scope='module')
def sampled():
    """(spec, rows, from the golden episodes?) per sample: the golden solved episodes of the base Pogostick-v1 and Bow-v1 configurations, and
    states after random valid steps from resets of both."""
    out = [RO.solved_states(cfg) + (True,) for cfg in ('pogo10', 'pogo13', 'bow10', 'bow20')]
    for env_id in (T.POGO, T.BOW):
        spec = make_spec(env_id, 10)
        out.append((spec, RO.random_states(spec, 8, 40, 3), False))
    return out


def test_consistency_on_the_cpu_oracle(sampled):
    """h(s) - h(s') <= cost(s, a) for every action a from every sampled state, and h = 0 wherever a step reached the goal.  A consistent h
    that is 0 at the goals never exceeds the cheapest cost to one.  (The first statement of the Bow extract rule - one inventory wool
    consumed - failed here: Extract_string takes the wool block in front of the agent, so h fell by the extract AND the wool's break, 8600,
    for a step of 5000; the rule lost its input.)"""
    changed_golden = changed = 0
    for spec, rows, golden in sampled:
        A = spec.compile().n_actions
        for scale in (1, 3):
            program = S.recipe_program(spec, scale=scale)
            lut, by_action = S.cost_table(None, scale, A)
            h, h_after, cost, goal = RO.transitions(spec, rows, program, lut)
            worst = h[None] - h_after - cost
            assert (worst <= 0).all(), (spec.env_id, scale, np.argwhere(worst > 0)[:5].tolist())
            assert goal.any() or not golden
            assert (h_after[goal] == 0).all() and (h >= 0).all()
            if scale == 1:
                changed += int((h_after != h[None]).sum())
                changed_golden += int((h_after != h[None]).sum()) if golden else 0
    print('transitions on which h changes: %d, %d of them from the golden episodes' % (changed, changed_golden))
    assert changed_golden >= 200, "the golden episodes alone no longer supply 200 transitions on which h changes"


# ------------------------------------------------------------------ the search model
CAP, CAP_POOL, KEEP = 256, 1024, 8


def late_stage(spec_size=9):
    from oracle.ngw_oracle import Oracle
    spec = make_spec(T.POGO, spec_size)
    o = Oracle(spec.compile(), 4, seed=XO.good_seed(spec, 4))
    o.reset()
    return spec, RO.late_stage_state(spec, SO.oracle_state(o))


def late_stage_model(spec, st, heuristic):
    """heuristic: None (h = 0), 'recipe' or 'recipe+walk' (weight 24, the cheapest movement cost, on the crafting table) - one root, real costs,
    keep 8, prune, iterated until proven() or 120 iterations."""
    if heuristic is None:
        m = BF.BestFirstModel(spec, CAP, CAP_POOL, KEEP, scale=1, prune=True)
    else:
        w = np.zeros(len(spec.items_id), np.int32)
        w[spec.items_id['crafting_table']] = 24
        m = RO.RecipeBestFirstModel(spec, CAP, CAP_POOL, KEEP, S.recipe_program(spec, None, 1), walk=(w, 'min') if heuristic == 'recipe+walk' else None, scale=1, prune=True)
    m.save(st, np.arange(4))
    m.cursor = 4
    m.start(np.arange(1))
    while not m.proven() and len(m.iterations) < 120:
        m.iterate()
    return m


EXPANDED = {None: 616, 'recipe': 39, 'recipe+walk': 39}      # (the figures DESIGN.md 4.27 and the README quote)


def test_the_recipe_term_proves_the_goal_under_the_real_costs():
    """A late-stage root - stick 4, plank 2, rubber 1 held, the crafting table across a walled room of 3 x 3 - under the REAL costs at scale 1:
    h = 0, the recipe term and recipe + walk all reach proven() with no state lost at the same goal value, 8532 (the craft's 8400 and five
    moves); h = 0 expands every state cheaper than that, 616; either heuristic 39 (the walk term adds nothing here: within 132 of the goal
    the recipe term has already cut everything that is not on the way)."""
    spec, st = late_stage()
    runs = {name: late_stage_model(spec, st, name) for name in EXPANDED}
    expanded = {name: sum(r['chosen'] - r['pruned'] for r in m.open_rows) for name, m in runs.items()}
    print('real costs, states expanded until proven():', expanded, {name: len(m.iterations) for name, m in runs.items()})
    for name, m in runs.items():
        assert m.proven() and not m.full and m.goal()[0] == 8532, name
    assert expanded['recipe'] < expanded[None] and expanded['recipe+walk'] < expanded[None]
    assert expanded == EXPANDED
    guided = runs['recipe+walk']
    assert guided.h[0] == 8400 + 24 * 5                                                 # the craft, and five moves to face the table


def test_recipe_heuristic_is_checked_on_the_host():
    assert S.RecipeHeuristic().walk is None and S.RecipeHeuristic(S.WalkHeuristic([1], 'min')).walk.mode == 'min'
    assert S.check_heuristic(S.RecipeHeuristic().walk, 3) == (_cabi.SEARCH_H_NONE, None)
    with pytest.raises(ValueError, match='mode'):
        S.check_heuristic(S.RecipeHeuristic(S.WalkHeuristic([0, 1, 2], 'mean')).walk, 3)
