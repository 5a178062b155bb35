"""Snapshot rollout, host side (no GPU): the C-ABI and Python surface, the host checks of Snapshot.rollout (snapshot.check_plan_ids,
check_rollout), and the whole call - sharded form included - on the oracle-backed stand-in (tests/slot_rollout_oracle.py), which is
itself held to T chained oracle expands."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import slot_rollout_oracle as RO
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.snapshot import check_plan_ids, check_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_rollout():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+ngw_snapshot_rollout\s*\(', text)
    assert re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', open(os.path.join(ROOT, 'include', 'ngw.h')).read())
    L = _cabi.lib()
    assert hasattr(L, 'ngw_snapshot_rollout') and 'ngw_snapshot_rollout' in _cabi.SYMBOLS
    assert L.ngw_snapshot_rollout(None, None, None, None, 0, 0, None, None, 0, None, None, None, None) == _cabi.E_INVALID_ARG
    assert 'NULL' in _cabi.last_error()


def test_python_surface():
    from gym_novel_gridworlds_amd.snapshot import Snapshot
    from gym_novel_gridworlds_amd.vec_env import PlanEval
    assert callable(Snapshot.rollout)
    e = PlanEval(np.array([1, 2], np.int32), np.array([3, 1], np.int32), np.array([True, True]), np.array([1 | 2, 14 << 8], np.uint32))
    assert e['ret'] is e.ret and e.goal.tolist() == [True, False] and e.died.tolist() == [False, True]


def test_host_checks_of_the_plans():
    a = check_plan_ids([[0, 1, 2], [3, 3, 3]], 4)
    assert a.dtype == np.int32 and a.shape == (2, 3) and a.flags.c_contiguous
    assert check_plan_ids(np.zeros((0, 5)), 4).shape == (0, 5)
    for bad in ([[0.5, 1.0]], [['a', 'b']], [[True, False]]):
        with pytest.raises(ValueError, match='integer'):
            check_plan_ids(bad, 4)
    for bad in ([0, 1], np.zeros((2, 2, 2), np.int32), np.zeros((2, 0), np.int32)):
        with pytest.raises(ValueError, match=r'shaped \[count, T\]'):
            check_plan_ids(bad, 4)
    with pytest.raises(ValueError, match='one action sequence per pair'):
        check_plan_ids(None, 4)
    with pytest.raises(ValueError, match='^4 is not in list$'):
        check_plan_ids([[0, 1], [4, 0]], 4)
    with pytest.raises(ValueError, match='^-1 is not in list$'):
        check_plan_ids([[0, -1]], 4)


def test_host_checks_of_the_index_lists():
    p, c, count = check_rollout([0, 0, 2], 3, [5, 4, 3], 3, 6, True)
    assert p.dtype == c.dtype == np.int32 and count == 3 and p.tolist() == [0, 0, 2]                  # parents may repeat
    assert check_rollout(None, 2, None, 4, 4, True) == (None, None, 2)                                  # nothing kept: no child to collide
    assert check_rollout([3, 3], 2, None, 4, 1, True)[2] == 2                                           # ... and no capacity to exceed
    assert check_rollout(None, 2, [2, 3], 4, 4, True)[2] == 2                                           # parents 0, 1 -> slots 2, 3
    assert check_rollout(None, 2, [0, 1], 4, 4, False)[2] == 2                                          # another buffer: the same indices are fine
    assert check_rollout([], 0, [], 3, 3, True)[2] == 0
    for bad in ([0.5, 1.0], ['a', 'b'], [True, False]):
        with pytest.raises(ValueError, match='integer'):
            check_rollout(bad, 2, [1, 2], 3, 6, False)
        with pytest.raises(ValueError, match='integer'):
            check_rollout([0, 0], 2, bad, 3, 6, False)
    with pytest.raises(ValueError, match='one-dimensional'):
        check_rollout(np.zeros((2, 1), np.int32), 2, [1, 2], 3, 6, False)
    with pytest.raises(ValueError, match='one-dimensional'):
        check_rollout([0, 0], 2, np.zeros((2, 1), np.int32), 3, 6, False)
    with pytest.raises(ValueError, match=r'parents: 3 outside \[0, 3\)'):
        check_rollout([0, 3], 2, [1, 2], 3, 6, False)
    with pytest.raises(ValueError, match=r'parents: -1 outside'):
        check_rollout([-1, 0], 2, None, 3, 6, False)
    with pytest.raises(ValueError, match=r'children: 6 outside \[0, 6\)'):
        check_rollout([0, 1], 2, [1, 6], 3, 6, False)
    # duplicate children; a child that is also a parent in the same buffer (and not in another)
    with pytest.raises(ValueError, match='children: the same index twice'):
        check_rollout([0, 1], 2, [2, 2], 3, 6, False)
    with pytest.raises(ValueError, match='slot 1 is also a parent'):
        check_rollout([0, 1], 2, [2, 1], 3, 6, True)
    assert check_rollout([0, 1], 2, [2, 1], 3, 6, False)[2] == 2
    with pytest.raises(ValueError, match='slot 1 is also a parent'):
        check_rollout(None, 2, [1, 4], 3, 6, True)
    # mismatched lengths; no list and more pairs than rows; more pairs than slots
    for args in (([0, 1, 2], 2, [3, 4]), ([0, 1], 3, [3, 4]), ([0, 1], 2, [3, 4, 5]), (None, 2, [3]), ([0], 2, None)):
        with pytest.raises(ValueError, match='different lengths'):
            check_rollout(*args, 3, 6, False)
    with pytest.raises(ValueError, match='4 pairs for 3 rows'):
        check_rollout(None, 4, [2, 3, 4, 5], 3, 6, False)

    class Dev:                                                  # a device tensor's values are not looked at, its length is
        def __init__(self, n):
            self.n = n
    dl = lambda x: x.n if isinstance(x, Dev) else None   # noqa: E731
    d = Dev(2)
    assert check_rollout(d, 2, [0, 1], 3, 6, True, dl)[0] is d                       # (children disjoint from parents: not checkable)
    with pytest.raises(ValueError, match='different lengths'):
        check_rollout(Dev(3), 2, [0, 1], 3, 6, True, dl)
    with pytest.raises(ValueError, match='7 pairs for a snapshot of 6 slots'):      # children with count above the capacity
        check_rollout([0] * 7, 7, Dev(7), 3, 6, False, dl)


def _env(n=12, cfg='pogo10', **kw):
    spec = T.build_spec(cfg)
    env = RO.OracleVecRollout(spec, n, seed=XO.good_seed(spec, n), **kw)
    env.reset()
    return spec, env


@pytest.mark.parametrize('cfg,auto', [('pogo10', True), ('fire10h', False), ('fire10h', True)])
def test_stand_in_equals_chained_oracle_expands(cfg, auto):
    """The rollout oracle against T chained oracle_expand calls that stop expanding a pair at its first done: the same end states, the
    same sums, lengths, ends and last info words; a pure evaluation leaves every slot as it was."""
    kw = dict(autoreset=True, horizon=14) if auto else {}
    spec, env = _env(n=24, cfg=cfg, **kw)
    A, n, steps = len(spec.actions_id), env.num_envs, 6
    rs = np.random.RandomState(1)
    for _ in range(9):
        env.step(rs.randint(0, A, n).astype(np.int32))
    count = 40
    parents, plans = rs.randint(0, n, count), rs.randint(0, A, (count, steps))
    pool = env.snapshot(count + n)
    pool.save(slots=count + np.arange(n))
    before = pool.state()
    e = pool.rollout(parents, plans, from_envs=True)
    after = pool.state()
    assert all((before[k] == after[k]).all() for k in RO.STATE_KEYS)
    e2 = pool.rollout(count + parents, plans, np.arange(count))                        # slot to slot in one buffer, kept
    for k in ('ret', 'length', 'ended', 'info'):
        assert (e[k] == e2[k]).all(), k
    # the chain
    rows = {k: getattr(env.o.st, k)[parents].copy() for k in RO.STATE_KEYS}
    ret, length = np.zeros(count, np.int64), np.zeros(count, np.int64)
    ended, info = np.zeros(count, bool), np.zeros(count, np.uint32)
    alive = np.ones(count, bool)
    for t in range(steps):
        idx = np.nonzero(alive)[0]
        if not idx.size:
            break
        kids, rep = XO.oracle_expand(spec, rows, idx, plans[idx, t], env.o.autoreset, env.o.horizon)
        for k in RO.STATE_KEYS:
            rows[k][idx] = kids[k]
        ret[idx] += rep['reward']; length[idx] += 1; info[idx] = rep['info']
        ended[idx] = rep['done']
        alive[idx[rep['done']]] = False
    assert (e.ret == ret).all() and (e.length == length).all() and (e.ended == ended).all() and (e.info == info).all()
    RO.assert_rows(pool.state(0, count), rows, '%s auto=%d' % (cfg, auto))
    if auto:
        assert (length[ended] < steps).any()                                           # (the horizon cuts pairs mid-plan)


def test_stand_in_invalid_ids_are_no_op_steps_that_count():
    spec, env = _env()
    A = len(spec.actions_id)
    rows = env.get_state()
    plans = np.array([[A, 1, 1], [1, -1, 1], [1, 1, 1]])
    ends, rep, alive = RO.oracle_slot_rollout(spec, rows, [0, 0, 0], plans)
    two, rep2, _ = RO.oracle_slot_rollout(spec, rows, [0], [[1, 1]])
    assert rep['length'].tolist() == [3, 3, 3] and alive.all()
    assert rep['ret'][0] == rep['ret'][1] == rep2['ret'][0] and rep['info'][0] == rep['info'][2]
    for k in RO.STATE_KEYS:
        assert (ends[k][0] == two[k][0]).all() and (ends[k][1] == two[k][0]).all(), k
    _, rep3, _ = RO.oracle_slot_rollout(spec, rows, [0], [[1, A]])
    assert rep3['info'][0] == 0 and rep3['length'][0] == 2


def test_stand_in_refuses_what_the_product_refuses():
    spec, env = _env()
    _, other = _env()
    s, t, foreign = env.snapshot(8), env.snapshot(8), other.snapshot(8)
    s.save(envs=[0, 1], slots=[0, 1])
    with pytest.raises(ValueError, match='also a parent'):
        s.rollout([0, 1], [[0, 0]] * 2, [1, 2])
    s.rollout([0, 1], [[0, 0]] * 2, [1, 2], source=t)                                  # another buffer of the same env
    s.rollout([0, 1], [[0, 0]] * 2)                                                    # nothing kept
    with pytest.raises(ValueError, match='another env'):
        s.rollout([0], [[0]], [1], source=foreign)
    with pytest.raises(ValueError, match='either source or from_envs'):
        s.rollout([0], [[0]], [1], source=t, from_envs=True)
    with pytest.raises(ValueError, match=r'outside \[0, 12\)'):
        s.rollout([12], [[0]], [1], from_envs=True)
    with pytest.raises(ValueError, match='is not in list'):
        s.rollout([0], [[0, len(spec.actions_id)]], [1])
    with pytest.raises(ValueError, match='the same index twice'):
        s.rollout([0, 1], [[0]] * 2, [3, 3])
    t.close()
    with pytest.raises(ValueError, match='closed'):
        s.rollout([0], [[0]], [1], source=t)
    with pytest.raises(ValueError, match='closed'):
        t.rollout([0], [[0]], [1], source=s)


def test_product_snapshot_refuses_closed_and_foreign_snapshots_before_any_device_call():
    """Snapshot.rollout's own guards run before it touches the device: checked on Snapshot objects that never had a handle."""
    from gym_novel_gridworlds_amd.snapshot import Snapshot

    class Env:
        _h, num_envs, n_actions, device = None, 4, 5, 0

    def bare(env, handle):
        s = Snapshot.__new__(Snapshot)
        s.env, s.capacity, s._s, s._keep = env, 8, C.c_void_p(handle), None
        return s
    env = Env()
    with pytest.raises(ValueError, match='closed'):
        bare(env, 0).rollout([0], [[0]], [1])
    live, other = Env(), Env()
    live._h = other._h = 1
    with pytest.raises(ValueError, match='closed'):
        bare(live, 1).rollout([0], [[0]], [1], source=bare(live, 0))
    with pytest.raises(ValueError, match='another env'):
        bare(live, 1).rollout([0], [[0]], [1], source=bare(other, 1))
    with pytest.raises(ValueError, match='either source or from_envs'):
        bare(live, 1).rollout([0], [[0]], [1], source=bare(live, 1), from_envs=True)
    with pytest.raises(ValueError, match='a Snapshot expected'):
        bare(live, 1).rollout([0], [[0]], [1], source=object())
    # the host checks of the arguments come before any device call too
    with pytest.raises(ValueError, match='^5 is not in list$'):
        bare(live, 1).rollout([0], [[0, 5]], [1])
    with pytest.raises(ValueError, match=r'shaped \[count, T\]'):
        bare(live, 1).rollout([0], [0], [1])
    with pytest.raises(ValueError, match='integer'):
        bare(live, 1).rollout([0], [[0.5]], [1])
    with pytest.raises(ValueError, match='the same index twice'):
        bare(live, 1).rollout([0, 1], [[0]] * 2, [3, 3])
    with pytest.raises(ValueError, match='slot 1 is also a parent'):
        bare(live, 1).rollout([0, 1], [[0]] * 2, [2, 1])
    with pytest.raises(ValueError, match=r'children: 8 outside \[0, 8\)'):
        bare(live, 1).rollout([0], [[0]], [8])
    with pytest.raises(ValueError, match=r'parents: 4 outside \[0, 4\)'):
        bare(live, 1).rollout([4], [[0]], from_envs=True)
    with pytest.raises(ValueError, match='different lengths'):
        bare(live, 1).rollout([0, 1], [[0]], [2, 3])


def test_sharded_env_rolls_out_rank_locally():
    """World 2 on the stand-in: each rank's snapshot() is its local env's, rollout takes the shard's own env indices, and the two shards
    together give what one env over all the envs gives."""
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld, shard_range
    spec = T.build_spec('pogo10')
    n, A, steps = 16, len(spec.actions_id), 5
    seed = XO.good_seed(spec, n)

    class Rank(ShardedVecNovelGridworld):
        def __init__(self, rank, world):                              # (a rank without a process group: what __init__ derives from it)
            self.rank, self.world, self.global_num_envs = rank, world, n
            self.first, self.num_envs = shard_range(n, world, rank)
            self.local = RO.OracleVecRollout(spec, self.num_envs, seed=seed, env_index_base=self.first, autoreset=True, horizon=4)
            self.spec = spec

    whole = RO.OracleVecRollout(spec, n, seed=seed, autoreset=True, horizon=4)
    whole.reset()
    rs = np.random.RandomState(2)
    plans = rs.randint(0, A, (n, steps))
    ws = whole.snapshot(n)
    we = ws.rollout(None, plans, np.arange(n), from_envs=True)
    assert (we.length == 4).all() and we.ended.all() and not we.goal.any()       # the horizon cuts every pair mid-plan
    for rank in range(2):
        env = Rank(rank, 2)
        env.reset()
        s = env.snapshot()
        assert s.env is env.local and s.capacity == n // 2 and callable(s.rollout)
        local = slice(env.first, env.first + env.num_envs)
        e = s.rollout(np.arange(env.num_envs), plans[local], np.arange(env.num_envs), from_envs=True)
        for k in ('ret', 'length', 'ended', 'info'):
            assert (e[k] == we[k][local]).all(), (rank, k)
        got, exp = s.state(), ws.state(env.first, env.num_envs)
        assert all((got[k] == exp[k]).all() for k in RO.STATE_KEYS), rank
        with pytest.raises(ValueError, match=r'outside \[0, 8\)'):                   # a GLOBAL env index is out of the shard's range
            s.rollout([n - 1], [[0]], from_envs=True)
        env.close()
