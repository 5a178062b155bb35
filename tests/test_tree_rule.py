"""The rule of ngw_tree_set_rule on the MI355X (csrc/ngw_tree.inc: the 16-lane reweight kernel and the backup's discount; tree.py spread=,
discount=).  The stages alone are held to tree.py's numpy references bit for bit on crafted statistics, whole runs to the model of
tests/tree_rule_oracle.py through the keys, at the smallest shapes where the kernels can go wrong: lists of 1, 15, 16, 17 and 257 entries (a
row of 16 lanes, a wave of 4 entries, a work-group of 16), A = 15, 17, 18 and 20 (one slot per lane, and a second slot used by 1, 2 and 4
lanes), 65 and 130 roots, T = 6."""
import ctypes as C

import numpy as np
import pytest
import torch

import guided_playout_oracle as GO
import ngw_testlib as T
import snapshot_oracle as SO
import test_tree_rule_cpu as XR
import test_tree_search as TS
import tree_oracle as TM
import tree_rule_oracle as RM
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.spec import IDX_NONE
from gym_novel_gridworlds_amd.tree import backup_reference, spread_rows_reference

pytestmark = pytest.mark.gpu
F_BAD_WEIGHT = 16
STEPS, ITERATIONS, KEYS, SEED, C_PUCT, Q_INIT = 6, 3, 4096, 0x7A11CAFE5EED0002, 6.0, -2.0
SIZES = {15: 'bow10', 17: 'pogo10', 18: 'axe10', 20: 'stk_fire_axeh10'}
BUCKETS = 64


def small_env(A):
    v = VecNovelGridworld(spec=T.build_spec(SIZES[A]), num_envs=4, seed=3)
    v.reset()
    assert v.n_actions == A
    return v


def fill(t, A, rs, priors):
    """Crafted and random statistics in the tree's 64 buckets -> the numpy copies."""
    v, r, m = XR.random_rows(rs, BUCKETS, A)
    cv, cr, cm, cp, _ = XR.crafted_rows(A)
    n = len(cm)
    v[1:1 + n], r[1:1 + n], m[1:1 + n] = cv, cr, cm
    p = rs.rand(BUCKETS, A).astype(np.float32)
    p[1:1 + n] = cp
    dev = t.visits.device
    t.visits.copy_(torch.from_numpy(v).to(dev))
    t.returns.copy_(torch.from_numpy(r).to(dev))
    t.mask_words.copy_(torch.from_numpy(m.view(np.int64)).to(dev))
    if priors:
        t.priors.copy_(torch.from_numpy(p).to(dev))
    return v, r, m, (p if priors else None)


def lists(rs):
    """Lists of 1, 15, 16, 17 and 257 entries: adjacent and distant duplicates, -1, IDX_NONE, entries out of range."""
    out = [np.array([5], np.int32)]
    for n in (15, 16, 17, 257):
        b = rs.randint(0, BUCKETS - 8, n).astype(np.int32)                           # (the last 8 buckets are never listed: their rows keep their bytes)
        b[n // 2] = b[0]                                                             # a distant duplicate
        if n >= 16:
            b[3:6] = b[2]                                                            # adjacent duplicates
            b[7], b[8], b[9], b[10] = -1, IDX_NONE, BUCKETS, 1 << 30
            b[n - 1] = b[n - 2]                                                      # ... and one at the tail
        if n == 257:
            b[15], b[16], b[63], b[64], b[255], b[256] = 6, 6, 7, 7, 9, 9           # duplicates across a row, a wave and a work-group boundary
        out.append(b)
    return out


@pytest.mark.parametrize('A', sorted(SIZES))
@pytest.mark.parametrize('S, rows16', [(1, 1), (2, 0), (17, 0), (64, 0)])
def test_the_reweight_stage_alone(S, rows16, A):
    v = small_env(A)
    pool, table = v.snapshot(4), v.key_table(BUCKETS // 2)
    assert table.buckets == BUCKETS
    for priors in (False, True):
        t = pool.tree_search(table, 4, 4, c=1.25, q_init=-3.0, priors=priors, spread=S, rows16=rows16)
        assert t.spread == S
        rs = np.random.RandomState(A * 100 + S)
        vis, ret, m, p = fill(t, A, rs, priors)
        for b in lists(rs):
            marker = rs.rand(BUCKETS, A).astype(np.float32) + 100                    # what an untouched row keeps
            t.rows.copy_(torch.from_numpy(marker).to(t.rows.device))
            v.error_flags()
            t.reweight(b)
            got = t.rows.cpu().numpy()
            named = np.unique(b[(b >= 0) & (b < BUCKETS)])
            exp, bad = spread_rows_reference(vis[named], ret[named], m[named], 1.25, -3.0, S, None if p is None else p[named])
            assert (got[named].view(np.uint32) == exp.view(np.uint32)).all(), (len(b), np.argwhere(got[named] != exp)[:4])
            rest = np.ones(BUCKETS, bool)
            rest[named] = False
            assert (got[rest].view(np.uint32) == marker[rest].view(np.uint32)).all(), "a row that was not listed changed"
            assert v.error_flags() == (F_BAD_WEIGHT if bad else 0), (len(b), bad)
        if priors:
            assert bad and not spread_rows_reference(vis[:1], ret[:1], m[:1], 1.25, -3.0, S, p[:1])[1]
            t.reweight(np.array([0], np.int32))                                      # a row of good priors raises nothing
            assert v.error_flags() == 0
        t.close()
    v.close()


@pytest.mark.parametrize('A', sorted(SIZES))
def test_one_lane_and_sixteen_lanes_at_spread_1(A):
    v = small_env(A)
    pool, table = v.snapshot(4), v.key_table(BUCKETS // 2)
    out = []
    for rows16 in (2, 1, 0):
        t = pool.tree_search(table, 4, 4, c=1.25, q_init=-3.0, priors=True, rows16=rows16)
        fill(t, A, np.random.RandomState(A), True)
        t.reweight(np.arange(BUCKETS, dtype=np.int32))
        out.append(t.rows.cpu().numpy().tobytes())
        t.close()
    assert out[0] == out[1] == out[2] and any(out[0])
    v.error_flags()
    v.close()


@pytest.mark.parametrize('g', [65536, 58982, 0])
def test_the_backup_stage_alone(g):
    """A recorded guided playout of 130 pairs, T = 6, per-pair limits and a bootstrap, against backup_reference - with and without plain_backup."""
    v, pool, table, t0, m = TS.make('pogo10')
    roots = TS.roots_of('pogo10')
    t0.start(roots)
    t0.run(2, SEED)                                                                  # a table with a few nodes in it
    rs = np.random.RandomState(6)
    limits = rs.randint(0, STEPS + 1, TS.ROOTS).astype(np.int32)
    boot = rs.randint(-(1 << 30), 1 << 30, TS.ROOTS).astype(np.int32)
    r = pool.playout(roots, STEPS, SEED, first_pair=7 * TS.ROOTS, limits=limits, record=True, path_keys=True, rewards=True, masks=True, table=table,
                     table_weights=t0.rows, device=True)
    rec = {k: getattr(r, k).cpu().numpy() for k in ('actions', 'rewards', 'where', 'depth', 'length')}
    assert (rec['length'] < STEPS).any() and (rec['depth'] >= 1).any()
    out = []
    for plain in (False, True):
        t = pool.tree_search(table, TS.ROOTS, STEPS, c=C_PUCT, plain_backup=plain, discount=g / 65536)
        assert t.discount_q16 == g
        t.backup(r, bootstrap=boot)
        vis, ret = np.zeros((table.buckets, v.n_actions), np.int32), np.zeros((table.buckets, v.n_actions), np.int64)
        touched = backup_reference(vis, ret, rec['actions'], rec['rewards'], rec['where'], rec['depth'], rec['length'], None, boot, g)
        assert (t.visits.cpu().numpy() == vis).all() and (t.returns.cpu().numpy() == ret).all()
        assert vis.sum() == (touched >= 0).sum() > 0 and (ret != 0).any(), "every add is recorded in touched, and the case backs something up"
        assert (t.last['touched'].cpu().numpy()[:STEPS] == touched).all()
        out.append(ret)
        t.close()
    assert (out[0] == out[1]).all()
    v.close()


def make(name, count, spread, discount, **kw):
    spec, o, seed, ekw, warmup, fields, auto = TS.twin(name)
    v = VecNovelGridworld(spec=spec, num_envs=GO.N, seed=seed, **ekw)
    v.reset()
    for a in warmup:
        v.step(a)
    if ekw:
        v.set_state(0, step_count=np.asarray(o.st.step_count, np.int32))
    pool, table = v.snapshot(GO.N + 8), v.key_table(KEYS)
    pool.save()
    t = pool.tree_search(table, count, STEPS, c=C_PUCT, q_init=Q_INIT, fields=fields, spread=spread, discount=discount, **kw)
    m = RM.RuleModel(spec, SO.oracle_state(o), count, STEPS, C_PUCT, Q_INIT, None, fields, table.buckets, autoreset=auto, horizon=GO.HORIZON if auto else 0,
                     spread=spread, discount_q16=int(round(discount * 65536)))
    return v, pool, table, t, m, o


def roots_of(name, count):
    r = np.random.RandomState(len(name)).randint(0, GO.N, count)
    r[60:70 if count > 70 else 65] = r[59]                                           # a run of equal roots across a wave boundary
    return r.astype(np.int32)


@pytest.mark.parametrize('spread, discount', [(8, 1.0), (1, 0.9), (64, 0.5)])
@pytest.mark.parametrize('name, count', [('pogo10', 130), ('bow12', 65), ('fire12h', 130), ('pogo10lim', 65)])
def test_whole_runs_against_the_model(name, count, spread, discount):
    v, pool, table, t, m, _ = make(name, count, spread, discount)
    roots = roots_of(name, count)
    t.start(roots)
    m.start(roots)
    TM.assert_tree(t, table, m, '%s start' % name, flags=0)
    for i in range(ITERATIONS):
        t.run(1, SEED)
        m.run(1, SEED)
        TM.assert_tree(t, table, m, '%s spread %d discount %s iteration %d' % (name, spread, discount, i), flags=0)
        assert (t.last['actions'].cpu().numpy()[:, :count] == m.last['actions']).all()
    if spread > 1:
        assert max(int((nd.row > 0).sum()) for nd in m.node.values()) >= 2, "a row allots more than one action"
    assert v.error_flags() == 0
    v.close()


def test_one_run_of_three_and_three_runs_of_one():
    out = []
    for split in (False, True):
        v, pool, table, t, m, _ = make('pogo10', 130, 8, 0.9)
        t.start(roots_of('pogo10', 130))
        if split:
            for _ in range(ITERATIONS):
                t.run(1, SEED)
        else:
            t.run(ITERATIONS, SEED)
        out.append(TS.snapshot_of(t) + [np.stack(t.stats()[1:6])])
        if split:
            m.start(roots_of('pogo10', 130))
            m.run(ITERATIONS, SEED)
            TM.assert_tree(t, table, m, 'three runs of one', flags=0)
        v.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


def test_roots_in_the_envs_and_the_adapter():
    v, pool, table, t, m, o = make('pogo10', 65, 8, 0.9)
    envs = (np.arange(65) % GO.N).astype(np.int32)
    t.start(envs, from_envs=True)
    m.start(envs)
    t.run(ITERATIONS, SEED)
    m.run(ITERATIONS, SEED)
    TM.assert_tree(t, table, m, 'from_envs', flags=0)
    v.close()
    from gym_novel_gridworlds_amd import LidarInFront
    env = T.make_adapter_env('pogo10')
    grown = {}
    for e, S in ((env, 1), (env, 8), (LidarInFront(env, num_beams=8), 8)):
        e.reset()
        table = e.key_table(1024)
        t = e.tree_search(table, 64, STEPS, c=4.0, spread=S, discount=0.9)
        assert (t.spread, t.discount_q16) == (S, 58982)
        t.run(2, 11)
        st = t.stats()
        assert st.iterations == 2 and (st.alive == 64).all() and st.flags == 0
        grown[S] = int(st.grown[0])
        t.close()
        table.close()
    assert grown[1] <= 1 < grown[8], "64 playouts from one state: one node with one-hot rows, several with spread = 8 (%s)" % grown
    env.close()


def test_a_default_tree_is_unchanged():
    out = []
    for kw in ({}, dict(spread=1, discount=1.0), dict(rows16=2), dict(rows16=1)):
        v, pool, table, t, _ = TS.make('pogo10', **kw)
        t.start(TS.roots_of('pogo10'))
        t.run(ITERATIONS, SEED)
        out.append(TS.snapshot_of(t) + [np.stack(t.stats()[1:6])])
        v.close()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()


def test_set_rule_forgets_the_last_backups_list():
    """include/ngw.h: ngw_tree_set_rule enqueues one fill of `touched` with -1, so reweight() with no list right after it rewrites no row - and the
    rows written after the next backup are the new rule's."""
    v, pool, table, t, m = TS.make('pogo10')
    roots = TS.roots_of('pogo10')
    t.start(roots)
    t.run(2, SEED)
    assert (t.last['touched'] >= 0).any()
    marker = torch.rand_like(t.rows) + 100
    t.rows.copy_(marker)
    t.reweight()                                                                    # the list of the last backup: its rows are rewritten
    changed = (t.rows != marker).any(dim=1)
    assert changed.any() and set(torch.unique(t.last['touched'][t.last['touched'] >= 0]).tolist()) == set(torch.nonzero(changed).flatten().tolist())
    t.rows.copy_(marker)
    assert _cabi.lib().ngw_tree_set_rule(v._h, t._t, C.byref(_cabi.TreeRule(8, 65536, 0, 0))) == 0
    assert (t.last['touched'] == -1).all()
    t.reweight()
    assert (t.rows == marker).all(), "reweight(NULL) right after set_rule rewrote a row"
    t.reweight(np.arange(table.buckets, dtype=np.int32))                            # named buckets: rewritten, under the new rule
    exp, _ = spread_rows_reference(t.visits.cpu().numpy(), t.returns.cpu().numpy(), t.mask_words.cpu().numpy().view(np.uint64), TS.C_PUCT, TS.Q_INIT, 8)
    assert (t.rows.cpu().numpy().view(np.uint32) == exp.view(np.uint32)).all() and exp.max() > 1
    v.error_flags()
    v.close()


def test_refusals():
    v, pool, table, t, _ = TS.make('pogo10')
    L = _cabi.lib()
    rule = lambda *a: C.byref(_cabi.TreeRule(*a))                                    # noqa: E731
    for args, msg in (((0, 65536, 0, 0), b'spread'), ((65, 65536, 0, 0), b'spread'), ((1, -1, 0, 0), b'discount_q16'), ((1, 65537, 0, 0), b'discount_q16'),
                      ((1, 65536, -1, 0), b'rows16'), ((1, 65536, 3, 0), b'rows16'), ((2, 65536, 2, 0), b'one-lane'), ((1, 65536, 0, 1), b'reserved')):
        assert L.ngw_tree_set_rule(v._h, t._t, rule(*args)) == _cabi.E_INVALID_ARG and msg in L.ngw_last_error(), args
    for args in ((None, t._t, rule(1, 65536, 0, 0)), (v._h, None, rule(1, 65536, 0, 0)), (v._h, t._t, None)):
        assert L.ngw_tree_set_rule(*args) == _cabi.E_INVALID_ARG and b'NULL' in L.ngw_last_error()
    assert L.ngw_tree_set_rule(v._h, t._t, rule(64, 0, 1, 0)) == 0 == L.ngw_tree_set_rule(v._h, t._t, rule(1, 65536, 2, 0))
    for kw, msg in ((dict(spread=0), 'spread'), (dict(spread=65), 'spread'), (dict(spread=2.0), 'spread'), (dict(spread=True), 'spread'), (dict(discount=-0.1), 'discount'),
                    (dict(discount=1.5), 'discount'), (dict(discount=float('nan')), 'discount'), (dict(discount='x'), 'discount'), (dict(rows16=3), 'rows16'),
                    (dict(rows16=2, spread=2), 'rows16')):
        with pytest.raises(ValueError, match=msg):
            pool.tree_search(table, 4, 4, **kw)
    t.close()
    assert L.ngw_tree_set_rule(v._h, t._t, rule(1, 65536, 0, 0)) == _cabi.E_INVALID_ARG
    v.close()
