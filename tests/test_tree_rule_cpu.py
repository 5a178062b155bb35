"""The rule of ngw_tree_set_rule on the CPU: tree.py's spread_rows_reference and the discounted backup_reference against brute-force statements,
the draw of sample.choose_weighted under a spread row, the model of tests/tree_rule_oracle.py against the references, and two properties on the
model - the pairs of one root diverge inside the tree, and the scenario of tests/test_tree_search_cpu.py under spread and discount."""
import functools

import numpy as np
import pytest

import guided_playout_oracle as GO
import snapshot_oracle as SO
import test_tree_search_cpu as X
import tree_rule_oracle as RM
from gym_novel_gridworlds_amd import tree as TR
from gym_novel_gridworlds_amd.sample import choose_weighted

F32 = np.float32
SPREADS, SIZES = (2, 3, 17, 64), (15, 17, 18, 20, 33, 48)


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


def random_rows(rs, n, A):
    visits = (rs.randint(0, 9, (n, A)) * rs.randint(0, 2, (n, A))).astype(np.int32)
    returns = np.where(visits > 0, rs.randint(-400, 100, (n, A)), 0).astype(np.int64)
    masks = rs.randint(0, 1 << A, n, dtype=np.int64).astype(np.uint64)
    masks[0] = 0
    return visits, returns, masks


def crafted_rows(A):
    """-> (visits, returns, masks, priors, what each row is)."""
    n = 12
    v, r, m = np.zeros((n, A), np.int32), np.zeros((n, A), np.int64), np.full(n, (1 << A) - 1, np.uint64)
    p = np.ones((n, A), F32)
    names = ['all scores equal', 'one valid action', 'mask 0', 'visits at 2^31 - 1', 'n_b beyond 2^24', 'large negative returns', 'priors: 0, tiny, 2^64, negative, NaN',
             'equal scores under a sparse mask', 'the highest action alone', 'visited everywhere', 'returns at the int64 ends', 'one visit each']
    m[1] = 1 << (A - 2)
    m[2] = 0
    v[3, :3] = (1 << 31) - 1
    r[3, :3] = (-5, 7, 1 << 40)
    v[4, 0], v[4, 1], v[4, 2] = (1 << 24) + 1, 3, 1                              # n_b + 1 + i crosses float32 steps of 2 above 2^24
    r[4, :3] = (-(1 << 24), -3, -1)
    v[5], r[5] = 2, -(1 << 50)
    r[5, A - 1] = -(1 << 50) + (1 << 28)
    p[6, :5] = (0.0, 2.0 ** -70, 2.0 ** 64, -1.0, np.nan)
    m[7] = 0b101010101010101 & ((1 << A) - 1)
    m[8] = 1 << (A - 1)
    v[9], r[9] = np.arange(1, A + 1), -np.arange(A) * 3
    v[10, :2], r[10, :2] = 1, (np.iinfo(np.int64).max, np.iinfo(np.int64).min)
    v[11], r[11] = 1, np.arange(A) % 3
    return v, r, m, p, names


# ------------------------------------------------------------------ 1. the spread rule
@pytest.mark.parametrize('A', SIZES)
def test_spread_1_is_the_one_hot_rule(A):
    rs = np.random.RandomState(A)
    v, r, m = random_rows(rs, 60, A)
    pri = rs.rand(60, A).astype(F32)
    cv, cr, cm, cp, _ = crafted_rows(A)
    for args in ((v, r, m, 1.25, -3.0, None), (v, r, m, 0.0, 0.5, pri), (cv, cr, cm, 2.0, -1.0, cp), (cv, cr, cm, 2.0, -1.0, None)):
        one, bad1 = TR.puct_rows_reference(*args)
        got, bad = TR.spread_rows_reference(*args[:5], 1, args[5])
        assert (bits(got) == bits(one)).all() and bad == bad1
    assert bad1 is False and TR.spread_rows_reference(cv, cr, cm, 2.0, -1.0, 1, cp)[1] is True


@pytest.mark.parametrize('A', SIZES)
@pytest.mark.parametrize('S', SPREADS)
def test_spread_rows_reference_against_brute_force(S, A):
    rs = np.random.RandomState(100 * S + A)
    v, r, m = random_rows(rs, 12, A)
    pri = rs.rand(12, A).astype(F32)
    for c, q_init, p in ((1.25, -3.0, None), (4.0, 0.0, pri), (0.0, -1.0, None)):
        got, bad = TR.spread_rows_reference(v, r, m, c, q_init, S, p)
        assert not bad
        for i in range(len(m)):
            exp, _ = RM.spread_row(v[i], r[i], m[i], c, q_init, S, None if p is None else p[i])
            assert (bits(got[i]) == bits(exp)).all(), (i, got[i], exp)
        assert (got.sum(1) == np.where(m != 0, S, 0)).all() and (got[0] == 0).all()
        assert all(not got[i, a] or (int(m[i]) >> a) & 1 for i in range(len(m)) for a in range(A)), "nothing is allotted to an invalid action"


@pytest.mark.parametrize('A', (15, 17, 48))
@pytest.mark.parametrize('S', SPREADS)
def test_crafted_rows(S, A):
    v, r, m, p, names = crafted_rows(A)
    for c in (2.0, 0.0):
        got, bad = TR.spread_rows_reference(v, r, m, c, -1.0, S, p)
        assert bad                                                                  # (the negative and the NaN prior of row 6)
        for i in range(len(m)):
            exp, b = RM.spread_row(v[i], r[i], m[i], c, -1.0, S, p[i])
            assert (bits(got[i]) == bits(exp)).all() and b == (i == 6), (names[i], got[i], exp)
        assert got[1, A - 2] == S and got[1].sum() == S and not got[2].any() and got[8, A - 1] == S
        if c == 0.0:                                                                # no bonus: every choice lands on the best mean, the lowest id on ties
            assert got[0, 0] == S and got[7, 0] == S and got[11, 2] == S   # (row 11: the means are a % 3)
    got, bad = TR.spread_rows_reference(v, r, m, 2.0, -1.0, S, None)
    assert not bad
    valid7 = [a for a in range(A) if (int(m[7]) >> a) & 1]
    for i, valid in ((0, list(range(A))), (7, valid7)):                             # all scores equal: the allotment walks the valid actions in id order
        exp = np.zeros(A, F32)
        for s in range(S):
            exp[valid[s % len(valid)]] += 1
        assert (got[i] == exp).all(), (names[i], got[i], exp)


def test_the_draw_under_a_spread_row_is_exact():
    """The entries are small integers: choose_weighted's running float32 sum is exact, its mass is S, and the action drawn is the one whose
    cumulative count first exceeds thr = float32(u * S)."""
    A = 17
    words = np.concatenate([[0, 1, 255, 256, 0xFFFFFFFF, 0xFFFFFF00, 0x80000000], np.random.RandomState(5).randint(0, 1 << 32, 2000, dtype=np.uint64)]).astype(np.uint32)
    rs = np.random.RandomState(9)
    for S in (2, 3, 17, 64):
        v, r, m = random_rows(rs, 6, A)
        rows, _ = TR.spread_rows_reference(v, r, m, 3.0, 0.0, S)
        for row, mask in zip(rows[1:], m[1:]):
            if not mask:
                continue
            got, mass, _ = choose_weighted(np.full(len(words), mask, np.uint64), row, 0, np.arange(len(words)), 0, A, words=words)
            assert (mass == S).all()
            cum = np.cumsum(row.astype(np.int64))
            thr = ((words >> np.uint32(8)).astype(F32) * F32(2.0 ** -24) * F32(S)).astype(F32).astype(np.float64)
            exp = np.array([int(np.argmax(cum > x)) for x in thr], np.int32)
            assert (thr < S).all() and (got == exp).all()
            assert set(got.tolist()) <= set(np.flatnonzero(row).tolist())


# ------------------------------------------------------------------ 2. the discount
def test_discount_65536_is_todays_backup():
    """g = 65536 against the parent's rule, stated here on its own: G_t = rewards[t:, j].sum() + bootstrap[j], added with int64 wrap.  int32 rewards
    keep |G| below (T + 1) * 2^31, so the sums near 2^62 come from preset `returns`, not from G: the wrap of the addition is what they exercise."""
    rs = np.random.RandomState(1)
    x = X.random_case(rs)
    x['rewards'] = np.where(x['rewards'] != 0, rs.randint(-(1 << 31), 1 << 31, x['rewards'].shape), 0).astype(np.int32)
    T_, count = x['actions'].shape
    boot = rs.randint(-(1 << 31), 1 << 31, count).astype(np.int32)
    big = rs.randint(-(1 << 62), 1 << 62, (8, 5)).astype(np.int64)
    big[1, 2] = np.iinfo(np.int64).max - 5                                         # bucket 1, action 2: pair 3's path - the sum wraps here
    n_add, g_add = np.zeros((8, 5), np.int64), np.zeros((8, 5), object)
    for j in range(count):
        d, n = int(x['depth'][j]), int(x['length'][j])
        for t in range(T_):
            if d >= 1 and t < n and t <= d:
                e = x['where'][t, j] if t < d else x['where_leaf'][j]
                if e >= 0:
                    n_add[e, x['actions'][t, j]] += 1
                    g_add[e, x['actions'][t, j]] += int(x['rewards'][t:, j].astype(np.int64).sum()) + int(boot[j])
    exp = np.array([[RM.wrap64(int(big[e, a]) + int(g_add[e, a])) for a in range(5)] for e in range(8)], np.int64)
    for kw in ({}, dict(discount_q16=65536)):
        visits, returns = np.zeros((8, 5), np.int32), big.copy()
        TR.backup_reference(visits, returns, x['actions'], x['rewards'], x['where'], x['depth'], x['length'], x['where_leaf'], boot, **kw)
        assert (visits == n_add).all() and (returns == exp).all()
    assert (np.abs(exp) > 1 << 61).any() and any(abs(int(g)) > 1 << 32 for g in g_add.ravel()) and n_add[1, 2] >= 2
    # D is the identity at 65536 for every x: no multiply, so nothing can wrap
    for g_in in (1 << 62, -(1 << 62), (1 << 63) - 1, -(1 << 63)):
        assert TR.discount_reference(g_in, 65536) == g_in == RM.discounted(g_in, 65536)


@pytest.mark.parametrize('g', [0, 1, 32768, 58982, 65535])
def test_discounted_backup_against_a_python_int_model(g):
    rs = np.random.RandomState(g % 97)
    for seed in range(3):
        x = X.random_case(rs)
        T_, count = x['actions'].shape
        boot = rs.randint(-900, 900, count).astype(np.int32)
        boot[3] = -777                                                              # pair 3: length = T with a leaf; pair 1: depth = length = T
        visits, returns = np.zeros((8, 5), np.int32), np.zeros((8, 5), np.int64)
        touched = TR.backup_reference(visits, returns, x['actions'], x['rewards'], x['where'], x['depth'], x['length'], x['where_leaf'], boot, g)
        n_add, g_add = np.zeros((8, 5), np.int64), np.zeros((8, 5), object)
        for j in range(count):
            d, n = int(x['depth'][j]), int(x['length'][j])
            G = RM.returns_to_go([int(v) for v in x['rewards'][:, j]], n, int(boot[j]), g)
            for t in range(T_):
                e = -1
                if d >= 1 and t < n:
                    e = x['where'][t, j] if t < d else (x['where_leaf'][j] if t == d else -1)
                assert touched[t, j] == e
                if e >= 0:
                    n_add[e, x['actions'][t, j]] += 1
                    g_add[e, x['actions'][t, j]] += G[t]
        assert (visits == n_add).all() and (returns == g_add.astype(np.int64)).all()
        assert (touched[:, 0] == -1).all()                                          # depth = 0: nothing is backed up
    # the cases, on the model itself
    assert RM.discounted(-1, 32768) == -1 and RM.discounted(-3, 32768) == -2 and RM.discounted(3, 32768) == 1, "floor, not truncation"
    assert RM.discounted(-1, 0) == 0 and RM.discounted(5, 1) == 0 and RM.discounted(-5, 1) == -1
    assert RM.returns_to_go([1, 2, 0, 0], 2, 1 << 20, 32768) == [1 + ((2 + (1 << 19)) >> 1), 2 + (1 << 19), 1 << 20], "a bootstrap is discounted len times, not T"
    wrapped = RM.discounted(1 << 50, 65535)
    assert wrapped == RM.wrap64(65535 << 50) >> 16 and wrapped != (65535 << 50) >> 16 and wrapped < 0, "the product wraps as int64 does"
    assert TR.discount_reference(1 << 50, 65535) == wrapped and TR.discount_reference(-3, 32768) == -2


def test_the_largest_rewards_in_the_backup():
    """int32 rewards and a bootstrap at their ends over three steps (a product g * G that wraps needs |G| >= 2^47, which int32 rewards reach only
    beyond 2^16 steps: D itself is held to the wrap in the test above)."""
    T_, g = 3, 65535
    actions, where = np.zeros((T_, 1), np.int32), np.zeros((T_, 1), np.int32)
    rewards = np.full((T_, 1), (1 << 31) - 1, np.int32)
    out = []
    for boot in (0, (1 << 31) - 1):
        visits, returns = np.zeros((1, 1), np.int32), np.zeros((1, 1), np.int64)
        returns[0, 0] = (1 << 62)
        TR.backup_reference(visits, returns, actions, rewards, where, np.array([3], np.int32), np.array([3], np.int32), None, np.array([boot], np.int32), g)
        G = RM.returns_to_go([(1 << 31) - 1] * 3, 3, boot, g)
        assert visits[0, 0] == 3 and int(returns[0, 0]) == RM.wrap64((1 << 62) + sum(G[:3]))
        out.append(int(returns[0, 0]))
    assert out[0] != out[1]


# ------------------------------------------------------------------ 3. the model against the references
@pytest.mark.parametrize('name, spread, g', [('pogo10', 8, 65536), ('pogo10', 1, 58982), ('fire12h', 17, 32768)])
def test_the_model_against_the_references(name, spread, g):
    spec, o, _, _, _ = GO.twin(name)
    _, _, auto, fields, _ = GO.CONFIGS[name]
    rs = np.random.RandomState(3)
    roots = rs.randint(0, GO.N, 40)
    roots[7:20] = roots[6]                                                         # shared roots: the pairs that the spread rule lets diverge
    m = RM.RuleModel(spec, SO.oracle_state(o), 40, 8, 2.0, -1.0, fields=fields, autoreset=auto, horizon=GO.HORIZON if auto else 0, spread=spread, discount_q16=g)
    m.start(roots)
    A = m.A
    boot = rs.randint(-30, 30, 40).astype(np.int32)
    for it in range(3):
        before = {k: (nd.n.copy(), nd.w.copy(), nd.mask, nd.row.copy()) for k, nd in m.node.items()}
        m.iterate(m.playout(77), boot)
        e = m.last
        order = list(m.node)
        bucket = {k: i for i, k in enumerate(order)}
        B = len(order) + 3
        visits, returns, masks, rows = np.zeros((B, A), np.int32), np.zeros((B, A), np.int64), np.zeros(B, np.uint64), np.zeros((B, A), F32)
        for k, (n, w, mk, row) in before.items():
            visits[bucket[k]], returns[bucket[k]], masks[bucket[k]], rows[bucket[k]] = n, w, mk, row
        where = np.array([[bucket[int(k)] if h else -1 for k, h in zip(kr, hr)] for kr, hr in zip(e['before'], e['hit'])], np.int32)
        where_leaf = np.array([bucket[int(k)] if h else -1 for k, h in zip(e['leaf'], e['held'])], np.int32)
        lk, _, _, bad = TR.iteration_reference(visits, returns, masks, rows, e['actions'], e['rewards'], where, e['depth'], e['length'], e['keys'], e['masks'],
                                               where_leaf, m.c, m.q_init, None, boot, spread=spread, discount_q16=g)
        assert (lk == e['leaf']).all() and not bad
        for k, nd in m.node.items():
            b = bucket[k]
            assert (visits[b] == nd.n).all() and (returns[b] == nd.w).all() and masks[b] == nd.mask and (bits(rows[b]) == bits(nd.row)).all(), (it, k)
    assert all(nd.row.sum() in (0, spread) for nd in m.node.values()) and any((nd.w != 0).any() for nd in m.node.values())
    if spread > 1:
        assert max(int((nd.row > 0).sum()) for nd in m.node.values()) >= 2


# ------------------------------------------------------------------ 4. divergence inside the tree
DIVERGE_SEED, DIVERGE_T, DIVERGE_C = 11, 6, 4.0


def diverge_model(spread, iterations=3):
    spec, o, _, _, _ = GO.twin('pogo10')
    m = RM.RuleModel(spec, SO.oracle_state(o), 64, DIVERGE_T, DIVERGE_C, spread=spread)
    m.start(np.full(64, 3, np.int64))                                              # one root state in all 64 roots; the dict has ample room
    m.run(iterations, DIVERGE_SEED)
    return m


def test_the_pairs_of_one_root_diverge_inside_the_tree():
    one, eight = diverge_model(1), diverge_model(8)
    assert all(r[0] == 64 for r in one.report + eight.report)
    assert all(r[1] <= 1 for r in one.report), "one-hot rows: every pair leaves the tree at the same state"
    assert eight.report[0][1] >= 2, "spread = 8: the first iteration grows %d nodes" % eight.report[0][1]
    print("grown per iteration: spread 1 %s, spread 8 %s" % ([r[1] for r in one.report], [r[1] for r in eight.report]))
    assert len(eight) > len(one)


# ------------------------------------------------------------------ 5. the scenario under spread and discount
SCENARIO_T, SCENARIO_I, SCENARIO_SEEDS = 12, 16, (X.CRAFT_SEED, 99)


@functools.lru_cache(maxsize=None)
def scenario_model(spread, g, seed):
    """The late-stage root of tests/test_tree_search_cpu.py in 130 roots, UNIFORM playouts of 12 steps (no default-policy weights)."""
    spec, st, _ = X.craft_scenario()
    m = RM.RuleModel(spec, st, X.CRAFT_ROOTS, SCENARIO_T, X.CRAFT_C, spread=spread, discount_q16=g)
    m.start(np.zeros(X.CRAFT_ROOTS, np.int64))
    m.run(SCENARIO_I, seed)
    return m


@pytest.mark.parametrize('seed', SCENARIO_SEEDS)
@pytest.mark.parametrize('spread, discount', [(1, 1.0), (8, 1.0), (1, 0.9), (8, 0.9)])
def test_the_scenario_under_spread_and_discount(spread, discount, seed):
    """What the model shows for the recorded seeds (DESIGN.md 4.30 holds the counts) - not a promise that discounting finds the plan."""
    spec, _, _ = X.craft_scenario()
    ids = spec.actions_id
    m = scenario_model(spread, int(round(discount * 65536)), seed)
    root = next(iter(m.node))
    nd = m.node[root]
    print("spread %d discount %.1f seed %d: root visits %s, %d nodes, deepest %d" % (
        spread, discount, seed, {a: int(nd.n[i]) for a, i in ids.items() if nd.n[i]}, len(m), max(r[4] for r in m.report)))
    assert int(nd.n.sum()) >= X.CRAFT_ROOTS * SCENARIO_I, "every pair of every iteration passed the root (a walk that returns to it counts again)"
    assert all((int(nd.mask) >> a) & 1 for a in np.flatnonzero(nd.n)), "only valid actions were visited"
    if spread == 1:
        assert len(m) <= 1 + SCENARIO_I, "one-hot rows: at most one node per iteration"
    else:
        assert len(m) > 1 + SCENARIO_I and int((nd.n > 0).sum()) >= 2, "the root's pairs spread over several actions; more than one node per iteration"
    assert m.best_actions([root])[0] == ids['Craft_stick'], "as recorded: under both seeds and all four rules the immediate +10 keeps the lead"
