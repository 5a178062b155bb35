"""Tree-search runs on the CPU: tree.py's numpy references against brute-force statements on random small inputs, the model of
tests/tree_oracle.py against the references, the one-hot row under sample.choose_weighted for a sweep of Philox words, and the scenario "it finds the craft" on the model -
with the constants the GPU test (tests/test_tree_search.py) holds the device to."""
import functools

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import pairs_oracle as PA
import recipe_oracle as RO
import snapshot_oracle as SO
import tree_oracle as TM
from gym_novel_gridworlds_amd import tree as TR
from gym_novel_gridworlds_amd.sample import choose_weighted
from gym_novel_gridworlds_amd.spec import IDX_NONE, make_spec


# ------------------------------------------------------------------ 1. the references against brute force
def random_case(rs, T_=6, count=9, buckets=8, A=5):
    length = rs.randint(0, T_ + 1, count)
    depth = np.array([rs.randint(0, n + 1) for n in length])
    depth[0], length[0] = 0, T_                                    # d = 0
    depth[1] = length[1] = T_                                      # d = length: the whole playout stayed in the tree
    length[2] = depth[2] = 0                                       # a pair that never ran (an IDX_NONE root)
    length[3], depth[3] = T_, T_ - 1                               # a long path in the tree, with a leaf
    actions = np.where(np.arange(T_)[:, None] < length, rs.randint(0, A, (T_, count)), -1).astype(np.int32)
    rewards = np.where(np.arange(T_)[:, None] < length, rs.randint(-50, 20, (T_, count)), 0).astype(np.int32)
    where = np.where(np.arange(T_)[:, None] < depth, rs.randint(0, 3, (T_, count)), -1).astype(np.int32)      # (3 buckets: repeats on one path)
    where[depth.clip(max=T_ - 1), np.arange(count)] = np.where(depth < T_, -1, where[T_ - 1])
    where[:, 3] = np.where(np.arange(T_) < depth[3], 1, -1)        # one (bucket, action) repeated along a path
    actions[:, 3] = np.where(np.arange(T_) < length[3], 2, -1)
    keys = np.where(np.arange(T_)[:, None] < length, rs.randint(1, 1 << 62, (T_, count)), 0).astype(np.uint64)
    masks = np.where(np.arange(T_)[:, None] < length, rs.randint(1, 1 << A, (T_, count)), 0).astype(np.uint64)
    where_leaf = np.where((depth >= 1) & (depth < length), rs.randint(-1, buckets, count), -1).astype(np.int32)
    return dict(actions=actions, rewards=rewards, where=where, depth=depth.astype(np.int32), length=length.astype(np.int32), keys=keys, masks=masks,
                where_leaf=where_leaf)


@pytest.mark.parametrize('seed', range(6))
def test_leaf_and_backup_references_against_brute_force(seed):
    rs = np.random.RandomState(seed)
    x = random_case(rs)
    T_, count = x['actions'].shape
    lk, lm = TR.leaf_reference(x['depth'], x['length'], x['keys'], x['masks'])
    for j in range(count):
        d, n = int(x['depth'][j]), int(x['length'][j])
        if 1 <= d < n:
            assert lk[j] == x['keys'][d - 1, j] and lm[j] == x['masks'][d, j] and lk[j] != 0
        else:
            assert lk[j] == 0 and lm[j] == 0
    boot = rs.randint(-9, 9, count).astype(np.int32) if seed % 2 else None
    visits, returns = rs.randint(0, 4, (8, 5)).astype(np.int32), rs.randint(-99, 99, (8, 5)).astype(np.int64)
    v0, r0 = visits.copy(), returns.copy()
    touched = TR.backup_reference(visits, returns, x['actions'], x['rewards'], x['where'], x['depth'], x['length'], x['where_leaf'], boot)
    # brute force: every (t, j) on its own, as a statement about sets
    n_add, g_add = np.zeros((8, 5), np.int64), np.zeros((8, 5), np.int64)
    for j in range(count):
        d = int(x['depth'][j])
        for t in range(T_):
            e = -1
            if d >= 1 and t < x['length'][j]:
                e = x['where'][t, j] if t < d else (x['where_leaf'][j] if t == d else -1)
            assert touched[t, j] == e
            if e >= 0:
                n_add[e, x['actions'][t, j]] += 1
                g_add[e, x['actions'][t, j]] += int(x['rewards'][t:, j].sum()) + (0 if boot is None else int(boot[j]))
    assert (visits == v0 + n_add).all() and (returns == r0 + g_add).all()
    assert n_add.max() >= 2 and (g_add < 0).any()                                   # repeated destinations and negative returns are in the case
    assert (touched[:, 0] == -1).all() and (touched[:, 2] == -1).all()


def brute_row(n, w, m, c, q_init, p):
    f = np.float32
    total = int(np.asarray(n, np.int64).sum())
    best, pick = None, -1
    for a in range(len(n)):
        if not (int(m) >> a) & 1:
            continue
        q = f(w[a]) / f(n[a]) if n[a] > 0 else f(q_init)
        u = f(f(f(c) * f(p[a])) * np.sqrt(f(total + 1))) / f(1 + int(n[a]))
        s = f(f(q) + f(u))
        if pick < 0 or s > best:
            best, pick = s, a
    row = np.zeros(len(n), f)
    if pick >= 0:
        row[pick] = 1
    return row


@pytest.mark.parametrize('seed', range(4))
def test_puct_rows_reference_against_brute_force(seed):
    rs = np.random.RandomState(100 + seed)
    A, n = 7, 40
    visits = (rs.randint(0, 6, (n, A)) * rs.randint(0, 2, (n, A))).astype(np.int32)
    returns = np.where(visits > 0, rs.randint(-400, 100, (n, A)), 0).astype(np.int64)
    masks = rs.randint(0, 1 << A, n).astype(np.uint64)
    masks[0], masks[1], visits[2], returns[2] = 0, 1 << 3, 0, 0                     # mask 0, one bit, an unvisited row: ties -> the lowest valid id
    masks[2] = 0b1010110
    visits[3], returns[3], masks[3] = 2, -8, (1 << A) - 1                           # equal scores everywhere: a tie
    priors = rs.rand(n, A).astype(np.float32)
    priors[4, 1], priors[5, 2], priors[6, 0], priors[7, 3] = -1.0, np.nan, 2.0 ** 65, 2.0 ** -70      # cleaned: each counts as 0
    for pr in (None, priors):
        rows, bad = TR.puct_rows_reference(visits, returns, masks, 1.25, -3.0, pr)
        assert bad == (pr is not None)
        clean = np.ones((n, A), np.float32) if pr is None else np.where((pr >= 2.0 ** -64) & (pr <= 2.0 ** 64), pr, 0).astype(np.float32)
        for i in range(n):
            assert (rows[i] == brute_row(visits[i], returns[i], masks[i], 1.25, -3.0, clean[i])).all(), i
        assert not rows[0].any() and rows[1, 3] == 1
        assert pr is not None or (rows[2, 1] == 1 and rows[3, 0] == 1)              # (equal priors: equal scores, the lowest valid id)
        assert ((rows == 1).sum(1) == (masks != 0)).all() and (rows[rows != 1] == 0).all()
        assert all((int(masks[i]) >> int(rows[i].argmax())) & 1 for i in range(n) if masks[i])
    rows, bad = TR.puct_rows_reference(visits, returns, masks, 1.25, -3.0, np.abs(np.nan_to_num(priors)).clip(0, 1))
    assert not bad
    assert (TR.best_actions_reference(visits[2:4], masks[2:4]) == [1, 0]).all() and TR.best_actions_reference(visits[:1], masks[:1])[0] == -1


def test_a_one_hot_row_is_chosen_for_every_philox_word():
    """The contract's remark on the thr = 0 corner: w = 0 gives u = 0 and thr = 0, and c[a] = 1 > 0 still holds - strictly."""
    A = 17
    words = np.concatenate([[0, 1, 255, 256, 0xFFFFFFFF, 0xFFFFFF00, 0x80000000], np.random.RandomState(5).randint(0, 1 << 32, 500, dtype=np.uint64)]).astype(np.uint32)
    for a in (0, 5, 16):
        row = np.zeros(A, np.float32)
        row[a] = 1.0
        for m in ((1 << A) - 1, 1 << a, (1 << a) | 1 | (1 << 16)):
            got, mass, _ = choose_weighted(np.full(len(words), m, np.uint64), row, 0, np.arange(len(words)), 0, A, words=words)
            assert (got == a).all() and (mass == 1).all()


# ------------------------------------------------------------------ 2. the model against the references
def model_case(name='pogo10', count=40, steps=8, **kw):
    import guided_playout_oracle as GO
    spec, o, _, _, _ = GO.twin(name)
    rs = np.random.RandomState(3)
    roots = rs.randint(0, GO.N, count)
    roots[5] = IDX_NONE
    roots[7:12] = roots[6]                                                         # shared roots: contention at t = 0
    m = TM.TreeModel(spec, SO.oracle_state(o), count, steps, **kw)
    m.start(roots)
    return spec, m, roots


def test_the_model_against_the_references():
    spec, m, roots = model_case(c=2.0, q_init=-1.0)
    A = m.A
    for it in range(4):
        before = {k: (nd.n.copy(), nd.w.copy(), nd.mask, nd.row.copy()) for k, nd in m.node.items()}
        m.run(1, 77)
        e = m.last
        order = list(m.node)                                                       # a bucket per key: its position in the model's dict
        bucket = {k: i for i, k in enumerate(order)}
        B = len(order) + 3
        visits, returns, masks, rows = np.zeros((B, A), np.int32), np.zeros((B, A), np.int64), np.zeros(B, np.uint64), np.zeros((B, A), np.float32)
        for k, (n, w, mk, row) in before.items():
            visits[bucket[k]], returns[bucket[k]], masks[bucket[k]], rows[bucket[k]] = n, w, mk, row
        where = np.array([[bucket[int(k)] if h else -1 for k, h in zip(kr, hr)] for kr, hr in zip(e['before'], e['hit'])], np.int32)
        where_leaf = np.array([bucket[int(k)] if h else -1 for k, h in zip(e['leaf'], e['held'])], np.int32)
        lk, lm, touched, bad = TR.iteration_reference(visits, returns, masks, rows, e['actions'], e['rewards'], where, e['depth'], e['length'], e['keys'],
                                                      e['masks'], where_leaf, m.c, m.q_init)
        assert (lk == e['leaf']).all() and not bad
        for k, nd in m.node.items():
            b = bucket[k]
            assert (visits[b] == nd.n).all() and (returns[b] == nd.w).all() and masks[b] == nd.mask and (rows[b].view(np.uint32) == nd.row.view(np.uint32)).all(), (it, k)
        assert (e['depth'][roots == IDX_NONE] == 0).all() and (e['actions'][:, roots == IDX_NONE] == -1).all()
    assert m.it == 4 and len(m.report) == 4 and sum(r[1] for r in m.report) == len(m) - len({int(k) for k in e['before'][0] if k})
    assert max(nd.n.sum() for nd in m.node.values()) >= 4 * 6                      # the shared root was visited by every one of its pairs, every iteration
    assert any((nd.w < 0).any() for nd in m.node.values())


def test_run_splits_and_a_full_table_on_the_model():
    _, a, _ = model_case(c=2.0)
    _, b, _ = model_case(c=2.0)
    a.run(3, 9)
    for _ in range(3):
        b.run(1, 9)
    assert list(a.node) == list(b.node) and all((a.node[k].n == b.node[k].n).all() and (a.node[k].w == b.node[k].w).all() for k in a.node)
    spec = model_case(c=2.0)[0]
    import guided_playout_oracle as GO
    _, o, _, _, _ = GO.twin('pogo10')
    m = TM.TreeModel(spec, SO.oracle_state(o), 20, 8, 2.0, buckets=2)
    m.start(np.zeros(20, np.int64))
    m.run(3, 4)
    assert len(m) == 2 and m.full and m.report[0][1] == 1 and m.report[1][2] == 20 and m.report[1][1] == 0     # one leaf grows, then every leaf is refused


# ------------------------------------------------------------------ 3. the scenario
# Chosen on the model: playouts of 24 steps under a heavy default policy (moves, and the goal's craft four times as likely) reach the craft often
# enough from the root's subtrees for their mean returns to separate within 32 iterations; with uniform playouts of 12 steps the +10 of
# Craft_stick - which spends the planks the Pogostick needs - keeps the lead.  The margin holds under a second seed (the test below checks both).
CRAFT_ROOTS, CRAFT_T, CRAFT_C, CRAFT_I, CRAFT_SEED = 130, 24, 8.0, 32, 5
CRAFT_HEAVY = (('Forward', 1.0), ('Left', 1.0), ('Right', 1.0), ('Craft_pogo_stick', 4.0))
CRAFT_PLAN = ('Right', 'Forward', 'Forward', 'Right', 'Forward', 'Craft_pogo_stick')


@functools.lru_cache(maxsize=None)
def craft_scenario(size=9):
    """The late-stage root of tests/test_recipe_heuristic*.py - ingredients held, the crafting table across a small room - in every one of 4 rows
    -> (spec, the rows, the default policy's weights)."""
    from oracle.ngw_oracle import Oracle
    spec = make_spec(T.POGO, size)
    o = Oracle(spec.compile(), 4, seed=XO.good_seed(spec, 4))
    o.reset()
    w = np.zeros(len(spec.actions_id), np.float32)
    for name, x in CRAFT_HEAVY:
        w[spec.actions_id[name]] = x
    return spec, RO.late_stage_state(spec, SO.oracle_state(o)), w


@functools.lru_cache(maxsize=None)
def craft_model(seed=CRAFT_SEED):
    spec, st, w = craft_scenario()
    m = TM.TreeModel(spec, st, CRAFT_ROOTS, CRAFT_T, CRAFT_C, weights=w)
    m.start(np.zeros(CRAFT_ROOTS, np.int64))
    m.run(CRAFT_I, seed)
    return m


@pytest.mark.parametrize('seed', [CRAFT_SEED, 99])
def test_it_finds_the_craft_on_the_model(seed):
    spec, st, _ = craft_scenario()
    ids = spec.actions_id
    plan = np.array([[ids[a]] for a in CRAFT_PLAN], np.int64)
    r = PA.step_pairs(spec, st, np.zeros(1, np.int64), len(plan), plan)
    info = int(r['reports']['info'][0])
    assert r['reports']['ended'][0] and info >> 1 & 1 and (info >> 8 & 255) != 14 and r['reports']['length'][0] == len(plan), "the plan reaches the goal"
    m = craft_model(seed)
    root = next(iter(m.node))
    nd = m.node[root]
    order = np.sort(nd.n)[::-1]
    print("root visits %s of %d" % (nd.n.tolist(), int(nd.n.sum())))
    assert m.best_actions([root])[0] == ids[CRAFT_PLAN[0]]
    assert order[0] >= 3 * order[1], "the margin: the plan's first action has three times the visits of the runner-up"
    assert nd.n[ids['Craft_stick']] < order[1] or nd.n[ids['Craft_stick']] * 3 <= order[0]
