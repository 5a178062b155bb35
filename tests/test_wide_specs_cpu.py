"""The wide specs of tests/wide_specs.py without a GPU: every row is what the table says, validate() refuses what lies beyond the limits, and
under the seeds the device file uses the wide columns are part of play - conditions on the inputs, asserted here so that a change of seed
cannot quietly empty a device test.  Everything runs on the CPU oracle and the CPU models."""
import numpy as np
import pytest

import expand_oracle as XO
import mask_oracle as M
import tree_rule_oracle as RM
import wide_specs as W
from gym_novel_gridworlds_amd import search as S
from gym_novel_gridworlds_amd import tree as TR
from gym_novel_gridworlds_amd.spec import ACT_CRAFT, ACT_SELECT

TREE_SIZES = (33, 40, 48)


def test_the_table():
    for name, (K, A, R, E, size, _, kernel) in W.TABLE.items():
        spec = W.spec_of(name)
        cs = spec.compile()
        assert (int(cs.n_items), int(cs.n_actions), int(cs.n_recipes), int(cs.n_entities), int(cs.map_size)) == (K, A, R, E, size), name
        assert len(spec.items_id) == K and len(spec.actions_id) == A and W.step_kernel_of(cs) == kernel, name
        assert spec.max_items == (24 if K > 20 else 20), name
        for alias, of in getattr(spec, 'aliases', {}).items():
            a, b = spec.actions_id[alias], spec.actions_id[of]
            assert a > b and (cs.act_kind[a], cs.act_arg[a]) == (cs.act_kind[b], cs.act_arg[b]), (name, alias)
    rows = list(W.TABLE.values())
    assert {r[0] for r in rows} >= {20, 21, 24} and {r[1] for r in rows} >= {33, 48} and any(28 <= r[1] <= 32 and r[0] == 20 for r in rows)
    assert any(38 <= r[1] <= 40 and r[0] == 24 and r[2] == 8 and r[3] for r in rows) and {r[6] for r in rows} == {'plain', 'general', 'extended'}


@pytest.mark.parametrize('name', [n for n in W.ALL if W.TABLE[n][0] >= 20])
def test_the_added_items_are_in_play(name):
    """Breakable, on the map, in the start inventory, lidar items; two added recipes consume an added item with id >= 12, one gives item K - 1."""
    from gym_novel_gridworlds_amd.lidar import LidarConfig
    spec = W.spec_of(name)
    cs, K = spec.compile(), W.TABLE[name][0]
    base = K - sum(1 for n in spec.items_id if n in W.NAMES or n == W.LAST)
    assert all(cs.breakable[k] for k in range(base, K))
    assert any(int(cs.start_item[j]) >= base for j in range(int(cs.n_start))) and int(cs.n_start) <= 8
    assert sum(int(cs.inv_start_item[j]) >= 12 for j in range(int(cs.n_inv_start))) >= 2 and int(cs.n_inv_start) <= 4
    eats = [r for r in range(int(cs.n_recipes)) if int(cs.recipe_out_item[r]) >= base and any(cs.recipe_in[r][k] for k in range(12, K))]
    assert len(eats) >= 2 and any(int(cs.recipe_out_item[r]) == K - 1 for r in eats)
    assert int(cs.recipe_out_item[int(cs.n_recipes) - 1]) == K - 1, "the recipe named last gives item K - 1"
    lc = LidarConfig(spec).compile(spec)
    assert int(lc.n_chan) == K - 2 and all(lc.chan_of_item[k] for k in range(base, K)) and int(lc.inv_item[int(lc.n_inv) - 1]) == K - 1


def test_validate_refuses_what_lies_beyond():
    import copy
    spec = copy.deepcopy(W.spec_of('w24a48'))
    spec.add_alias('Forward')
    with pytest.raises(ValueError, match='A=49'):
        spec.validate()
    spec = copy.deepcopy(W.spec_of('w24'))
    spec.add_new_item('one_more')
    spec.max_items = 25
    with pytest.raises(ValueError, match='K=25'):
        spec.validate()
    spec = copy.deepcopy(W.spec_of('w24'))
    W.add_recipe(spec, 'amber', {'tree_log': 1}, 1)
    with pytest.raises(ValueError, match='R=9'):
        spec.validate()
    spec = copy.deepcopy(W.spec_of('w21'))
    spec.max_items = 20
    with pytest.raises(AssertionError, match='Cannot have more than 20 items'):
        spec.validate()


@pytest.mark.parametrize('name', W.ALL)
def test_the_warm_up_plays_the_wide_columns(name):
    spec, _, start, acts, o, log = W.oracle_env(name)
    cs = spec.compile()
    K, A, R = W.TABLE[name][:3]
    last = np.asarray(o.st.inv)[:, K - 1] > 0
    assert last.any(), "inventory column K - 1 stays zero"
    assert last[np.arange(W.N_ENVS) % 3 != 2].sum() >= 8, "item K - 1 is crafted from the start tables alone, not only from a rich inventory"
    assert K <= 12 or (np.asarray(o.st.inv)[:, 12:] > 0).sum() > W.N_ENVS, "the columns past 12 are almost empty"
    crafted = {int(cs.act_arg[a]) for step, l in zip(acts, log) for a, ok in zip(step, l[2]) if ok and int(cs.act_kind[a]) == ACT_CRAFT}
    assert R - 1 in crafted, "the recipe named last (index %d) is never crafted: %s" % (R - 1, crafted)
    if A > 32:
        assert any(int(w) >> 32 for l in log for w in l[0]), "no state has a valid action >= 32"
        done = 0
        for step, l in zip(acts, log):
            for i in np.flatnonzero((step >= 32) & l[2]):
                kind = int(cs.act_kind[step[i]])
                done += kind == ACT_CRAFT or (kind == ACT_SELECT and int(l[1]['selected'][i]) != int(cs.act_arg[step[i]]))
        assert done >= 4, "no action >= 32 is executed with an effect"
    if A == 48:
        assert max(bin(int(w)).count('1') for l in log for w in l[0]) > 32, "no state has more than 32 valid actions"
        words = M.oracle_mask_words(spec, o.st)
        assert max(bin(int(w)).count('1') for w in words) > 32, "... nor has one after the warm-up"


@pytest.mark.parametrize('name', [n for n in W.ALL if W.TABLE[n][0] >= 20])
def test_the_recipe_bound_reads_the_wide_columns(name):
    spec = W.spec_of(name)
    K = W.TABLE[name][0]
    program = S.recipe_program(spec, None, 1)
    rows = W.rows_of(name)
    counts = S.map_item_counts(rows['map'], K)
    h = S.recipe_cost_reference(rows['inv'], counts, program)
    assert (h > 0).any() and len(set(h.tolist())) > 2 and any(u.out_item == K - 1 for u in program.rules)
    inv = np.zeros((2, K), np.int32)
    inv[1, K - 1] = 1                                                                # two states that differ in item K - 1 (>= 12) alone
    pair = S.recipe_cost_reference(inv, counts[:2] * 0, program)
    assert pair[0] > pair[1]


@pytest.mark.parametrize('A', TREE_SIZES)
@pytest.mark.parametrize('S_', (1, 2, 17, 64))
def test_the_references_on_the_wide_crafted_rows(S_, A):
    v, r, m, p, names = W.wide_crafted_rows(A)
    for c, q_init, pri in ((1.25, -3.0, None), (1.25, -3.0, p), (0.0, -3.0, None), (1.25, float('nan'), None)):
        got, _ = TR.spread_rows_reference(v, r, m, c, q_init, S_, pri)
        for i in range(len(m)):
            exp, _ = RM.spread_row(v[i], r[i], m[i], c, q_init, S_, None if pri is None else pri[i])
            assert (got[i].view(np.uint32) == exp.view(np.uint32)).all(), (names[i], got[i], exp)
        w = got[len(m) - 10:]
        assert not w[:, A:].any() and (w.sum(1) == S_).all()
        assert not w[5, :32].any() and not w[6, :32].any() and w[7].sum() == S_ and w[8, 33 % A] == S_
        if c == 0.0:                                                                 # no bonus: the best mean takes everything, the lowest id on ties
            assert w[0, 5] == w[1, 21] == w[2, A - 1] == w[3, 0] == w[4, 32] == S_ and w[6, A - 1] == S_
        if q_init != q_init:
            assert w[6, 32] == S_, "NaN at the first valid action (32) keeps the pick"
    if S_ == 64 and A == 48:
        got, _ = TR.spread_rows_reference(v, r, m, 1.25, -3.0, S_, None)
        assert (got[-1] >= 1).all(), "all 48 valid, nothing visited: 64 choices reach every action"


TREE_SEED, TREE_T, TREE_C, TREE_Q = 0x7A11CAFE5EED0003, 6, 6.0, -2.0


def tree_roots(name, count=W.N_ENVS):
    r = np.random.RandomState(len(name)).randint(0, W.N_ENVS, count)
    r[60:65] = r[59]
    return r.astype(np.int32)


def tree_model(name, spread, g, count=W.N_ENVS, buckets=1 << 30):
    spec = W.spec_of(name)
    return RM.RuleModel(spec, W.rows_of(name), count, TREE_T, TREE_C, TREE_Q, None, buckets=buckets, spread=spread, discount_q16=g)


@pytest.mark.parametrize('name', ['w20a33', 'w24a48'])
def test_a_tree_allots_a_wide_action(name):
    """Group h on the model: three iterations at spread 8 - some node's row allots an action >= 32."""
    m = tree_model(name, 8, 58982)
    roots = tree_roots(name)
    m.start(roots)
    m.run(3, TREE_SEED)
    assert any(nd.row[32:].any() for nd in m.node.values()) and sum(r[1] for r in m.report) >= 3
