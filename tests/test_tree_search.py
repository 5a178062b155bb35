"""Tree-search runs on the MI355X (csrc/ngw_tree.inc, csrc/ngw_abi_tree.cpp, include/ngw.h ngw_tree_*; tree.py, Snapshot.tree_search).  Every
expectation is the model of tests/tree_oracle.py on the CPU oracle, compared through the keys - never the kernels' own output -, at the smallest
shapes at which the kernels can still go wrong: 130 roots (two full waves and a tail, across a 128 boundary), T = 12, 6 iterations, a table of
4 096 keys; 10 x 10 maps - and 12 x 12 for the Bow and the FireWall configuration, the smallest size at which guided_playout_oracle's and
ngw_testlib's fixtures of those classes exist (S * S = 144 is also the 16-byte map row) -, 9 x 9 for the scenario."""
import functools

import numpy as np
import pytest
import torch

import guided_playout_oracle as GO
import ngw_testlib as T
import snapshot_oracle as SO
import test_tree_search_cpu as X
import tree_oracle as TM
from gym_novel_gridworlds_amd import VecNovelGridworld
from gym_novel_gridworlds_amd.playout import tree_steps
from gym_novel_gridworlds_amd.snapshot import MapsTooLarge
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, IDX_NONE, make_spec
from gym_novel_gridworlds_amd.state_keys import KEY_STATE
from gym_novel_gridworlds_amd.tree import TreeSearch, puct_rows_reference

pytestmark = pytest.mark.gpu
F_TABLE_FULL, F_BAD_WEIGHT = 8, 16
ROOTS, STEPS, ITERATIONS, KEYS, SEED, C_PUCT, Q_INIT = 130, 12, 6, 4096, 0x7A11CAFE5EED0001, 6.0, -2.0
STATE = ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode')
# pogo10, an EXT configuration with FireWall deaths (autoreset, the step count in the key), a compiled LimitActions spec - guided_playout_oracle's -, and a Bow one
CONFIGS = ('pogo10', 'bow12', 'fire12h', 'pogo10lim')


@functools.lru_cache(maxsize=None)
def twin(name):
    """-> (spec, the oracle after a warm-up, seed, env keywords, the warm-up actions, key fields, autoreset)."""
    if name in GO.CONFIGS:
        _, _, auto, fields, _ = GO.CONFIGS[name]
        return GO.twin(name) + (fields, auto)
    from oracle.ngw_oracle import Oracle
    import expand_oracle as XO
    spec = T.build_spec('bow10', map_size=12)
    seed = XO.good_seed(spec, GO.N)
    o = Oracle(spec.compile(), GO.N, seed=seed)
    o.reset()
    rs = np.random.RandomState(12)
    warmup = [rs.randint(0, len(spec.actions_id), GO.N).astype(np.int32) for _ in range(10)]
    for a in warmup:
        o.step(a)
    return spec, o, seed, {}, warmup, KEY_STATE, False


def make(name, keys=KEYS, **kw):
    """The device twin, its states saved into a pool, a table, the tree and the model -> (v, pool, table, t, m)."""
    spec, o, seed, ekw, warmup, fields, auto = twin(name)
    v = VecNovelGridworld(spec=spec, num_envs=GO.N, seed=seed, **ekw)
    v.reset()
    for a in warmup:
        v.step(a)
    if ekw:
        v.set_state(0, step_count=np.asarray(o.st.step_count, np.int32))
    pool, table = v.snapshot(GO.N + 8), v.key_table(keys)
    pool.save()
    kw = dict(dict(c=C_PUCT, q_init=Q_INIT), **kw)
    t = pool.tree_search(table, ROOTS, STEPS, fields=fields, **kw)
    m = TM.TreeModel(spec, SO.oracle_state(o), ROOTS, STEPS, kw['c'], kw['q_init'], kw.get('weights'), fields, table.buckets, autoreset=auto,
                     horizon=GO.HORIZON if auto else 0)
    return v, pool, table, t, m


def roots_of(name):
    rs = np.random.RandomState(len(name))
    r = rs.randint(0, GO.N, ROOTS)
    r[64:70] = r[63]                                                                # a run of equal roots across a wave boundary
    return r.astype(np.int32)


def assert_uncommitted(v, pool, name):
    _, o = twin(name)[:2]
    st, ps = v.get_state(), pool.state(0, GO.N)
    for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode'):
        exp = np.asarray(getattr(o.st, k))
        assert (st[k].reshape(exp.shape) == exp).all() and (ps[k].reshape(exp.shape) == exp).all(), (name, k)


@pytest.mark.parametrize('name', CONFIGS)
def test_against_the_model_iteration_by_iteration(name):
    v, pool, table, t, m = make(name)
    masks_before, look = v.action_masks().copy(), v.lookahead()
    roots = roots_of(name)
    t.start(roots)
    m.start(roots)
    TM.assert_tree(t, table, m, name + ' start', flags=0)
    for i in range(ITERATIONS):
        t.run(1, SEED)
        m.run(1, SEED)
        TM.assert_tree(t, table, m, '%s iteration %d' % (name, i), flags=0)
        e = m.last
        assert (t.last['actions'].cpu().numpy()[:, :ROOTS] == e['actions']).all() and (t.last['depth'].cpu().numpy()[:ROOTS] == e['depth']).all()
        assert (t.last['leaf_keys'].cpu().numpy().view(np.uint64)[:ROOTS] == e['leaf']).all()
    assert sum(r[1] for r in m.report) >= ITERATIONS and max(r[4] for r in m.report) >= 2, "the trees grew and were descended"
    keys = np.array(list(m.node), np.uint64)
    got = t.read(keys)
    assert (got.where == table.lookup(keys)).all() and (got.n == np.stack([nd.n for nd in m.node.values()])).all()
    assert (t.best_actions(torch.from_numpy(keys.view(np.int64)).to(t.visits.device)) == m.best_actions(keys)).all()
    absent = t.read(np.array([12345], np.uint64))
    assert absent.where[0] == -1 and not absent.n.any() and absent.mask[0] == 0 and t.best_actions(np.array([12345], np.uint64))[0] == -1
    # nothing is committed: env state, pool rows, masks, the lookahead table
    assert_uncommitted(v, pool, name)
    assert (v.action_masks() == masks_before).all()
    for a, b in zip(v.lookahead(), look):
        assert (np.asarray(a) == np.asarray(b)).all()
    assert v.error_flags() == 0
    spec, o, seed, ekw = twin(name)[:4]
    if ekw:                                                                         # no prepared episode was consumed: the resets are the oracle's
        from oracle.ngw_oracle import Oracle
        o2 = Oracle(spec.compile(), GO.N, seed=seed, **ekw)
        o2.st = o.st.copy()
        rs, ends = np.random.RandomState(4), 0
        for step in range(30):
            a = rs.randint(0, len(spec.actions_id), GO.N).astype(np.int32)
            o2.step(a)
            _, reward, done, _ = v.step(a, copy=True)
            assert (reward == o2.reward).all() and (done == o2.done.astype(bool)).all(), step
            ends += int(done.sum())
        s = v.get_state()
        assert ends >= GO.N and (s['map'].reshape(GO.N, -1) == np.asarray(o2.st.map).reshape(GO.N, -1)).all() and (s['episode'] == o2.st.episode).all()
    v.close()


def snapshot_of(t):
    """Everything a run leaves, free of bucket numbers - which bucket a key gets is the table's choice and may differ between two tables -: the
    statistics of the occupied buckets as rows (mask word, visits, returns, the row's bits) in sorted order, the recorded arrays that hold no
    bucket as they are, and of `where` / `touched` / `where_leaf` which entries name a bucket."""
    n, w, m, r = [x.cpu().numpy() for x in (t.visits, t.returns, t.mask_words, t.rows)]
    held = m != 0
    table = np.concatenate([m[held, None], n[held].astype(np.int64), w[held], r[held].view(np.uint32).astype(np.int64)], 1)
    table = table[np.lexsort(table.T[::-1])]
    assert not n[~held].any() and not w[~held].any() and not r[~held].any()
    plain = ('actions', 'keys', 'rewards', 'masks', 'depth', 'length', 'leaf_keys', 'leaf_masks', 'fresh')
    return [table] + [t.last[k].cpu().numpy().copy() for k in plain] + [t.last[k].cpu().numpy() >= 0 for k in ('where', 'touched', 'where_leaf')]


def test_one_run_of_six_six_runs_of_one_and_a_second_object():
    out = []
    for split in (False, True, False):
        v, pool, table, t, _ = make('pogo10')
        t.start(roots_of('pogo10'))
        if split:
            for _ in range(ITERATIONS):
                t.run(1, SEED)
        else:
            t.run(ITERATIONS, SEED)
        out.append(snapshot_of(t) + [t.stats()[:6]])
        v.close()
    for other in out[1:]:
        for a, b in zip(out[0][:-1], other[:-1]):
            assert a.tobytes() == b.tobytes()
        assert all((x == y).all() for x, y in zip(out[0][-1][1:], other[-1][1:])) and out[0][-1][0] == other[-1][0] == ITERATIONS
    assert out[0][0][:, 1:18].sum() > ROOTS * ITERATIONS


def test_every_root_the_same_slot():
    """Full contention: at t = 0 every lane of every wave adds to one (bucket, action) - the in-wave combining's case."""
    v, pool, table, t, m = make('pogo10')
    roots = np.full(ROOTS, 3, np.int32)
    t.start(roots)
    m.start(roots)
    t.run(ITERATIONS, SEED)
    m.run(ITERATIONS, SEED)
    TM.assert_tree(t, table, m, 'one root', flags=0)
    root = m.node[next(iter(m.node))]
    assert root.n.sum() >= ROOTS * ITERATIONS and root.n.max() >= 2 * ROOTS
    v.close()


def hand_written(v, pool, table2, roots, rows, first_pair, fields, N, Q, M, c, q_init, bootstrap=None, grow=True):
    """One iteration of the loop TreeSearch.run replaces, on a second table: a guided playout, table.insert of the leaves, tree_steps and two
    INTEGER index_add_ calls, and the rows recomputed on the host under the recorded masks."""
    A = v.n_actions
    r = pool.playout(roots, STEPS, SEED, first_pair=first_pair, record=True, path_keys=True, fields=fields, rewards=True, masks=True, table=table2,
                     table_weights=rows, device=True)
    d, n, j = r.depth.long(), r.length.long(), torch.arange(len(roots), device=r.depth.device)
    has = (d >= 1) & (d < n) & grow
    leaf = torch.where(has, r.keys[(d - 1).clamp(0, STEPS - 1), j], torch.zeros_like(r.keys[0]))
    found = table2.insert(leaf, device=True)
    wl = found.where.long()
    ok = wl >= 0
    M[wl[ok]] = r.masks[d.clamp(0, STEPS - 1), j][ok]
    where = r.where.clone()
    where[d.clamp(0, STEPS - 1)[ok], j[ok]] = found.where[ok]                       # the leaf's step joins the in-table steps
    steps = torch.arange(STEPS, device=where.device)[:, None]
    where[(steps > d[None, :]) | (d[None, :] < 1)] = -1                             # steps beyond the leaf are the default policy's
    G = torch.flip(torch.cumsum(torch.flip(r.rewards.long(), [0]), 0), [0]) + (0 if bootstrap is None else bootstrap.long()[None, :])
    b, a, tt, jj = tree_steps(r._replace(where=where))
    N.view(-1).index_add_(0, b * A + a, torch.ones_like(b, dtype=torch.int32))
    Q.view(-1).index_add_(0, b * A + a, G[tt, jj])
    touched = torch.unique(b).cpu().numpy()
    new_rows, _ = puct_rows_reference(N.cpu().numpy()[touched], Q.cpu().numpy()[touched], M.cpu().numpy()[touched], c, q_init)
    rows[torch.from_numpy(touched).to(rows.device)] = torch.from_numpy(new_rows).to(rows.device)
    return r


@pytest.mark.parametrize('bootstrap', [False, True])
def test_the_stages_against_the_hand_written_loop(bootstrap):
    """run() against grow / backup / reweight on a second object, and both against tree_steps + integer index_add_ on a third table - through
    the keys."""
    v, pool, table, t, m = make('pogo10')
    _, _, _, _, _, fields, _ = twin('pogo10')
    A, roots = v.n_actions, roots_of('pogo10')
    dev = t.visits.device
    table2, table3 = v.key_table(KEYS), v.key_table(KEYS)
    s = pool.tree_search(table2, ROOTS, STEPS, c=C_PUCT, q_init=Q_INIT, fields=fields)
    for x in (t, s):
        x.start(roots)
    m.start(roots)
    N, Q = torch.zeros((table3.buckets, A), dtype=torch.int32, device=dev), torch.zeros((table3.buckets, A), dtype=torch.int64, device=dev)
    M, rows = torch.zeros(table3.buckets, dtype=torch.int64, device=dev), torch.zeros((table3.buckets, A), dtype=torch.float32, device=dev)
    rk = pool.keys(roots, fields, device=True)
    w0 = table3.insert(rk, device=True).where.long()
    M[w0] = pool.sample_actions(roots, np.zeros((ROOTS, A), np.float32), 0, device=True).mask_words
    first, _ = puct_rows_reference(N.cpu().numpy()[w0.cpu().numpy()], Q.cpu().numpy()[w0.cpu().numpy()], M.cpu().numpy()[w0.cpu().numpy()], C_PUCT, Q_INIT)
    rows[w0] = torch.from_numpy(first).to(dev)
    rs = np.random.RandomState(8)
    for i in range(4):
        boot = torch.from_numpy(rs.randint(-20, 20, ROOTS).astype(np.int32)).to(dev) if bootstrap else None
        r = pool.playout(roots, STEPS, SEED, first_pair=i * ROOTS, record=True, path_keys=True, fields=fields, rewards=True, masks=True, table=table2,
                         table_weights=s.rows, device=True)
        s.grow(r)
        s.backup(r, bootstrap=boot)
        s.reweight()
        hand_written(v, pool, table3, roots, rows, i * ROOTS, fields, N, Q, M, C_PUCT, Q_INIT, boot)
        m.iterate(m.playout(SEED), None if boot is None else boot.cpu().numpy())
        m.it = i + 1
        if not bootstrap:
            t.run(1, SEED)
    keys = np.array(list(m.node), np.uint64)
    b2, b3 = table2.lookup(keys), table3.lookup(keys)
    assert (b2 >= 0).all() and (b3 >= 0).all() and len(table2) == len(table3) == len(m)
    exp_n, exp_w = np.stack([nd.n for nd in m.node.values()]), np.stack([nd.w for nd in m.node.values()])
    exp_rows = np.stack([nd.row for nd in m.node.values()])
    assert (s.visits.cpu().numpy()[b2] == exp_n).all() and (s.returns.cpu().numpy()[b2] == exp_w).all() and (s.rows.cpu().numpy()[b2] == exp_rows).all()
    assert (N.cpu().numpy()[b3] == exp_n).all() and (Q.cpu().numpy()[b3] == exp_w).all() and (rows.cpu().numpy()[b3] == exp_rows).all()
    if not bootstrap:
        m.it = 4
        m.report = m.report[-4:]
        TM.assert_tree(t, table, m, 'run against the stages', flags=0)
    else:
        assert (exp_w != 0).any()
    # a backup without a grow: no pair has a leaf
    before = s.visits.sum().item()
    r = pool.playout(roots, STEPS, SEED, first_pair=99 * ROOTS, record=True, path_keys=True, fields=fields, rewards=True, masks=True, table=table2,
                     table_weights=s.rows, device=True)
    s.backup(r)
    assert s.visits.sum().item() - before == int(r.depth.sum().item())
    assert v.error_flags() == 0
    v.close()


def test_priors_and_a_bad_one():
    pri = lambda k: (np.array([((k >> (3 * a)) & 7) for a in range(17)], np.float32) / 4)   # noqa: E731
    v, pool, table, t, m = make('pogo10', priors=True)
    m.priors = pri
    roots = roots_of('pogo10')

    def fill():
        keys = np.array(list(m.node), np.uint64)
        b = torch.from_numpy(table.lookup(keys).astype(np.int64)).to(t.priors.device)
        t.priors[b] = torch.from_numpy(np.stack([pri(int(k)) for k in keys.tolist()])).to(t.priors.device)
        m.fill_priors()
    t.start(roots)
    m.start(roots)
    fill()
    for i in range(4):
        t.run(1, SEED)
        m.run(1, SEED)
        TM.assert_tree(t, table, m, 'priors %d' % i, flags=0)
        fill()
    assert not m.bad
    # a negative prior counts as 0 and raises F_BAD_WEIGHT once its row is recomputed
    root = int(pool.keys(roots[:1])[0])
    good = pri
    bad = lambda k: np.where(np.arange(17) == 1, np.float32(-1.0), good(k)).astype(np.float32) if k == root else good(k)   # noqa: E731
    pri, m.priors = bad, bad
    fill()
    t.run(1, SEED)
    m.run(1, SEED)
    assert m.bad
    TM.assert_tree(t, table, m, 'a bad prior', flags=F_BAD_WEIGHT)
    assert v.error_flags() == F_BAD_WEIGHT
    v.close()


def test_a_table_too_small():
    """Two buckets: the root and the first leaf fill them; every later leaf is refused - F_TABLE_FULL from the insert - and the run goes on."""
    v, pool, table, t, m = make('pogo10', keys=1)
    assert table.buckets == 2
    roots = np.full(ROOTS, 5, np.int32)
    t.start(roots)
    m.start(roots)
    t.run(1, SEED)
    m.run(1, SEED)
    TM.assert_tree(t, table, m, 'filled', flags=0)
    t.run(3, SEED)
    m.run(3, SEED)
    st = TM.assert_tree(t, table, m, 'full', flags=F_TABLE_FULL)
    assert m.full and st.refused[-1] == ROOTS and st.grown[-1] == 0 and st.backed_up[-1] > 0
    assert v.error_flags() == F_TABLE_FULL
    v.close()


def test_roots_that_are_not_there_and_a_second_start():
    v, pool, table, t, m = make('pogo10')
    roots = roots_of('pogo10')[:100]                                                # shorter than `playouts`
    roots[[0, 64, 99]] = IDX_NONE
    t.start(roots)
    m.start(roots)
    t.run(3, SEED)
    m.run(3, SEED)
    TM.assert_tree(t, table, m, 'IDX_NONE roots', flags=0)
    assert (t.last['length'].cpu().numpy()[[0, 64, 99]] == 0).all() and (t.last['touched'].cpu().numpy()[:, 100:] == -1).all()
    # an index out of range in a device list: skipped, F_BAD_INDEX
    far = roots.copy()
    far[7] = 10 ** 6
    t.start(torch.from_numpy(far).to(t.visits.device))
    m.start(far)
    t.run(1, SEED)
    m.run(1, SEED)
    st = TM.assert_tree(t, table, m, 'a root out of range')
    assert st.flags & F_BAD_INDEX and v.error_flags() & F_BAD_INDEX
    with pytest.raises(ValueError, match='outside'):
        t.start(far)
    with pytest.raises(ValueError, match='roots'):
        t.start(np.zeros(ROOTS + 1, np.int32))
    # a committed step, then start() again from the envs: what was learned stays, and the trees go on from the new roots
    held = {k: (nd.n.copy(), nd.w.copy()) for k, nd in m.node.items()}
    spec, o = twin('pogo10')[:2]
    from oracle.ngw_oracle import Oracle
    o2 = Oracle(spec.compile(), GO.N, seed=1)
    o2.st = o.st.copy()
    a = np.full(GO.N, spec.actions_id['Right'], np.int32)
    v.step(a)
    o2.step(a)
    envs = np.arange(GO.N, dtype=np.int32)
    t.start(envs, from_envs=True)
    m.start(envs, rows=SO.oracle_state(o2))
    TM.assert_tree(t, table, m, 'a second start')
    assert all((m.node[k].n == n).all() and (m.node[k].w == w).all() for k, (n, w) in held.items())
    t.run(2, SEED)
    m.run(2, SEED)
    TM.assert_tree(t, table, m, 'after the second start')
    # table.clear() leaves the statistics, clear() zeroes both
    table.clear()
    assert len(table) == 0 and t.visits.sum().item() > 0
    t.clear()
    m.clear()
    assert not t.visits.any() and not t.returns.any() and not t.mask_words.any() and not t.rows.any() and t.stats().iterations == 0
    t.start(envs, from_envs=True)
    m.start(envs)
    t.run(1, SEED)
    m.run(1, SEED)
    TM.assert_tree(t, table, m, 'after clear')
    v.error_flags()
    v.close()


def test_refusals():
    v, pool, table, t, m = make('pogo10')
    other = VecNovelGridworld(spec=make_spec(T.POGO, 10), num_envs=4, seed=3)
    other.reset()
    with pytest.raises(ValueError, match='another env|of this'):
        pool.tree_search(other.key_table(16), 4, 4)
    other.close()
    for kw, msg in ((dict(playouts=1 << 20, steps=1 << 12), 'playouts \\* steps'), (dict(fields=0), 'fields'), (dict(c=float('nan')), 'finite'),
                    (dict(q_init=float('inf')), 'finite'), (dict(playouts=0), 'playouts'), (dict(steps=0), 'steps'), (dict(weights=np.ones(3, np.float32)), 'weights')):
        args = dict(dict(playouts=4, steps=4), **kw)
        with pytest.raises(ValueError, match=msg):
            pool.tree_search(table, **args)
    big = v.key_table(1 << 27)                                                     # 2^28 buckets * 17 actions
    with pytest.raises(ValueError, match='buckets \\* n_actions'):
        pool.tree_search(big, 4, 4)
    big.close()
    with pytest.raises(ValueError, match='iterations'):
        t.run(-1, 0)
    with pytest.raises(ValueError, match='seed'):
        t.run(1, -1)
    r = pool.playout(np.zeros(4, np.int32), STEPS + 1, 1, record=True, path_keys=True, rewards=True, masks=True, table=table, table_weights=t.rows, device=True)
    with pytest.raises(ValueError, match='steps'):
        t.grow(r)
    table.close()
    with pytest.raises(ValueError, match='closed'):
        t.run(1, 0)
    pool.close()
    assert t.closed
    v.close()
    huge = VecNovelGridworld(spec=make_spec(T.POGO, 64), num_envs=4, seed=3)
    huge.reset()
    with pytest.raises(MapsTooLarge):
        huge.snapshot(4).tree_search(huge.key_table(16), 4, 4)
    huge.close()


def test_the_adapter_and_a_wrapper():
    """A tree rooted in the single-env adapter's current state - also through a LidarInFront wrapper -, and re-rooted after a step."""
    from gym_novel_gridworlds_amd import LidarInFront
    env = T.make_adapter_env('pogo10')
    for e in (env, LidarInFront(env, num_beams=8)):
        e.reset()
        table = e.key_table(256)
        t = e.tree_search(table, 64, 8, c=4.0)
        assert isinstance(t, TreeSearch)
        t.run(4, 11)
        st = t.stats()
        root = np.array([e.state_key()], np.uint64)
        best = t.best_actions(root)
        assert st.iterations == 4 and (st.alive == 64).all() and st.grown.sum() == 4 and 0 <= best[0] < t.n_actions and st.flags == 0
        held = t.read(root).n.sum()
        assert held >= 4 * 64
        e.step(int(best[0]))
        t.start(np.zeros(64, np.int32), from_envs=True)
        t.run(2, 11)
        assert t.stats().iterations == 6 and t.read(root).n.sum() >= held and len(table) >= 5
        t.close()
        assert t.closed
        table.close()
    env.close()


def test_it_finds_the_craft():
    """The scenario of tests/test_tree_search_cpu.py: the late-stage root in 130 roots; the device is held to the model bit for bit, so the
    most-visited valid root action - the first action of the plan that reaches the goal - cannot hide behind a threshold."""
    spec, st, w = X.craft_scenario()
    m = X.craft_model()
    v = VecNovelGridworld(spec=spec, num_envs=4, seed=4)
    v.reset()
    v.set_state(0, **{k: st[k] for k in STATE})
    pool, table = v.snapshot(4), v.key_table(KEYS)
    pool.save()
    t = pool.tree_search(table, X.CRAFT_ROOTS, X.CRAFT_T, c=X.CRAFT_C, weights=w)
    roots = np.zeros(X.CRAFT_ROOTS, np.int32)
    t.start(roots)
    t.run(X.CRAFT_I, X.CRAFT_SEED)
    TM.assert_tree(t, table, m, 'the craft', flags=0)
    assert (t.best_actions(roots) == spec.actions_id[X.CRAFT_PLAN[0]]).all()
    v.close()
