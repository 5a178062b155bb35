"""Snapshot expand, host side (no GPU): the host checks of Snapshot.expand (snapshot.check_expand), expand_all's pairing, the C-ABI and
Python surface, and the whole call - sharded form included - on the oracle-backed stand-in (tests/expand_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.snapshot import Expansion, all_actions_pairs, check_action_ids, check_expand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_expand():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+ngw_snapshot_expand\s*\(', text)
    L = _cabi.lib()
    assert hasattr(L, 'ngw_snapshot_expand') and 'ngw_snapshot_expand' in _cabi.SYMBOLS
    assert L.ngw_snapshot_expand(None, None, None, None, None, None, 1, None, None, None) == _cabi.E_INVALID_ARG
    assert 'NULL' in _cabi.last_error()


def test_python_surface():
    from gym_novel_gridworlds_amd.snapshot import Snapshot
    assert callable(Snapshot.expand) and callable(Snapshot.expand_all)
    e = Expansion(np.array([1, 2], np.int32), np.array([True, True]), np.array([True, False]),
                  np.array([1 | 2, 14 << 8], np.uint32))
    assert e['reward'] is e.reward and e.goal.tolist() == [True, False] and e.died.tolist() == [False, True]
    assert e.reshape(2, 1).info.shape == (2, 1)
    from gym_novel_gridworlds_amd.vec_env import decode_info_words
    assert decode_info_words(e.info)['message_code'].tolist() == [0, 14]


def test_host_checks_of_the_arguments():
    ok = check_expand([0, 0, 2], [1, 0, 3], [5, 4, 3], 3, 6, 4, True)
    assert [x.dtype for x in ok[:3]] == [np.int32] * 3 and ok[3] == 3 and ok[0].tolist() == [0, 0, 2]     # parents may repeat
    assert check_expand(None, [0, 1], [2, 3], 4, 4, 2, True)[3] == 2                                       # parents 0, 1 -> slots 2, 3
    assert check_expand(None, [0, 1], None, 4, 4, 2, False)[3] == 2                                        # another buffer: the same indices are fine
    assert check_expand([], [], [], 3, 3, 2, True)[3] == 0
    # bad dtype or shape
    for bad in ([0.5, 1.0], ['a', 'b'], [True, False]):
        with pytest.raises(ValueError, match='integer'):
            check_expand(bad, [0, 0], [1, 2], 3, 6, 4, False)
        with pytest.raises(ValueError, match='integer'):
            check_expand([0, 0], bad, [1, 2], 3, 6, 4, False)
        with pytest.raises(ValueError, match='integer'):
            check_expand([0, 0], [0, 0], bad, 3, 6, 4, False)
    for k in range(3):
        args = [[0, 0], [0, 0], [1, 2]]
        args[k] = np.zeros((2, 1), np.int32)
        with pytest.raises(ValueError, match='one-dimensional'):
            check_expand(*args, 3, 6, 4, False)
    with pytest.raises(ValueError, match='one action id per pair'):
        check_expand([0], None, [1], 3, 6, 4, False)
    # out of range: parent, child, action
    with pytest.raises(ValueError, match=r'parents: 3 outside \[0, 3\)'):
        check_expand([0, 3], [0, 0], [1, 2], 3, 6, 4, False)
    with pytest.raises(ValueError, match=r'parents: -1 outside'):
        check_expand([-1, 0], [0, 0], [1, 2], 3, 6, 4, False)
    with pytest.raises(ValueError, match=r'children: 6 outside \[0, 6\)'):
        check_expand([0, 1], [0, 0], [1, 6], 3, 6, 4, False)
    with pytest.raises(ValueError, match='^4 is not in list$'):
        check_expand([0, 1], [0, 4], [1, 2], 3, 6, 4, False)
    with pytest.raises(ValueError, match='^-1 is not in list$'):
        check_action_ids([2, -1], 4)
    # repeated child; child equal to a parent in the same buffer (and not in another)
    with pytest.raises(ValueError, match='children: the same index twice'):
        check_expand([0, 1], [0, 0], [2, 2], 3, 6, 4, False)
    with pytest.raises(ValueError, match='slot 1 is also a parent'):
        check_expand([0, 1], [0, 0], [2, 1], 3, 6, 4, True)
    assert check_expand([0, 1], [0, 0], [2, 1], 3, 6, 4, False)[3] == 2
    with pytest.raises(ValueError, match='slot 0 is also a parent'):
        check_expand(None, [0, 0], None, 3, 6, 4, True)
    with pytest.raises(ValueError, match='slot 1 is also a parent'):
        check_expand(None, [0, 0], [1, 4], 3, 6, 4, True)
    # mismatched lengths; no list and more pairs than rows
    for args in (([0, 1, 2], [0, 0], [3, 4]), ([0, 1], [0, 0, 0], [3, 4]), ([0, 1], [0, 0], [3, 4, 5]), (None, [0, 0], [3]), ([0], [0, 0], None)):
        with pytest.raises(ValueError, match='different lengths'):
            check_expand(*args, 3, 6, 4, False)
    with pytest.raises(ValueError, match='4 pairs for 3 rows'):
        check_expand(None, [0] * 4, [2, 3, 4, 5], 3, 6, 4, False)
    with pytest.raises(ValueError, match='7 pairs for a snapshot of 6 slots'):
        check_expand([0] * 7, [0] * 7, None, 3, 6, 4, False)
    # a device tensor's values are not looked at, its length is
    class Dev:
        def __init__(self, n):
            self.n = n
    dl = lambda x: x.n if isinstance(x, Dev) else None   # noqa: E731
    d = Dev(2)
    assert check_expand(d, [0, 0], [0, 1], 3, 6, 4, True, dl)[0] is d                # (children disjoint from parents: not checkable)
    with pytest.raises(ValueError, match='different lengths'):
        check_expand(Dev(3), [0, 0], [0, 1], 3, 6, 4, True, dl)
    assert check_expand([0, 1], Dev(2), Dev(2), 3, 6, 4, True, dl)[3] == 2


def test_expand_all_pairs_every_parent_with_every_action():
    p, a, c, shape = all_actions_pairs([7, 2, 7], 10, 4)
    assert shape == (3, 4)
    assert p.tolist() == [7] * 4 + [2] * 4 + [7] * 4 and a.tolist() == [0, 1, 2, 3] * 3 and c.tolist() == list(range(10, 22))
    p, a, c, shape = all_actions_pairs(np.zeros(0, np.int64), 3, 5)
    assert shape == (0, 5) and p.size == a.size == c.size == 0
    import torch
    tp, ta, tc, shape = all_actions_pairs(torch.tensor([7, 2], dtype=torch.int32), 10, 3)
    assert shape == (2, 3) and tp.dtype == ta.dtype == tc.dtype == torch.int32
    assert tp.tolist() == [7, 7, 7, 2, 2, 2] and ta.tolist() == [0, 1, 2, 0, 1, 2] and tc.tolist() == list(range(10, 16))


def _env(n=12, cfg='pogo10', **kw):
    spec = T.build_spec(cfg)
    env = XO.OracleVecExpand(spec, n, seed=XO.good_seed(spec, n), **kw)
    env.reset()
    return spec, env


def test_stand_in_children_and_reports_are_the_stepped_rows():
    """The stand-in end to end: children are what stepping the parent gives, reports what the step reports, nothing else changes; a second
    generation grows slot to slot; expand_all's table is the lookahead table of the parents."""
    import lookahead_oracle as LO
    spec, env = _env(autoreset=True, horizon=25)
    A, n = len(spec.actions_id), env.num_envs
    rs = np.random.RandomState(0)
    for _ in range(10):
        env.step(rs.randint(0, A, n).astype(np.int32))
    before = env.get_state()
    pool = env.snapshot(n * (A + 2))
    acts = rs.randint(0, A, n)
    e = pool.expand(None, acts, np.arange(n), from_envs=True)
    twin = XO.OracleVecExpand(spec, n, seed=0, autoreset=True, horizon=25)
    twin.set_state(0, **before)
    _, reward, done, info = twin.step(acts.astype(np.int32))
    assert (e.reward == reward).all() and (e.done == done).all() and (e.result == info['result']).all()
    after = env.get_state()
    assert all((before[k] == after[k]).all() for k in XO.STATE_KEYS)
    kids = pool.state(0, n)
    ended = e.done
    for k in ('map', 'loc', 'facing', 'inv', 'selected'):                              # where no reset ran the twin holds the child
        assert (kids[k][~ended] == twin.get_state()[k][~ended]).all(), k
    assert (kids['step_count'] == before['step_count'] + 1).all() and (kids['episode'] == before['episode']).all()
    # second generation, slot to slot in the same buffer, through expand_all
    t = pool.expand_all([0, 3], n)
    assert t.reward.shape == (2, A)
    look = LO.oracle_lookahead(spec, XO.rows_state(spec, kids, [0, 3]), True, 25)
    LO.assert_table(t, look, 'expand_all against the lookahead of the parents')
    assert (pool.state(0, n)['map'] == kids['map']).all()                              # the parents are untouched


def test_stand_in_refuses_what_the_product_refuses():
    spec, env = _env()
    _, other = _env()
    s, t, foreign = env.snapshot(8), env.snapshot(8), other.snapshot(8)
    s.save(envs=[0, 1], slots=[0, 1])
    with pytest.raises(ValueError, match='also a parent'):
        s.expand([0, 1], [0, 0], [1, 2])
    s.expand([0, 1], [0, 0], [1, 2], source=t)                                          # another buffer of the same env
    with pytest.raises(ValueError, match='another env'):
        s.expand([0], [0], [1], source=foreign)
    with pytest.raises(ValueError, match='either source or from_envs'):
        s.expand([0], [0], [1], source=t, from_envs=True)
    with pytest.raises(ValueError, match=r'outside \[0, 12\)'):
        s.expand([12], [0], [1], from_envs=True)
    with pytest.raises(ValueError, match='is not in list'):
        s.expand([0], [len(spec.actions_id)], [1])
    t.close()
    with pytest.raises(ValueError, match='closed'):
        s.expand([0], [0], [1], source=t)
    with pytest.raises(ValueError, match='closed'):
        t.expand([0], [0], [1], source=s)


def test_product_snapshot_refuses_closed_and_foreign_snapshots_before_any_device_call():
    """Snapshot.expand's own guards run before it touches the device: checked on Snapshot objects that never had a handle."""
    from gym_novel_gridworlds_amd.snapshot import Snapshot

    class Env:
        _h, num_envs, n_actions, device = None, 4, 5, 0

    def bare(env, handle):
        s = Snapshot.__new__(Snapshot)
        s.env, s.capacity, s._s, s._keep = env, 8, C.c_void_p(handle), None
        return s
    env = Env()
    with pytest.raises(ValueError, match='closed'):
        bare(env, 0).expand([0], [0], [1])
    live, other = Env(), Env()
    live._h = other._h = 1
    with pytest.raises(ValueError, match='closed'):
        bare(live, 1).expand([0], [0], [1], source=bare(live, 0))
    with pytest.raises(ValueError, match='another env'):
        bare(live, 1).expand([0], [0], [1], source=bare(other, 1))
    with pytest.raises(ValueError, match='either source or from_envs'):
        bare(live, 1).expand([0], [0], [1], source=bare(live, 1), from_envs=True)
    with pytest.raises(ValueError, match='a Snapshot expected'):
        bare(live, 1).expand([0], [0], [1], source=object())


def test_sharded_env_expands_rank_locally():
    """World 2 on the stand-in: each rank's snapshot() is its local env's, expand takes the shard's own env indices, and the two shards
    together give what one env over all the envs gives."""
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld, shard_range
    spec = T.build_spec('pogo10')
    n, A = 16, len(spec.actions_id)
    seed = XO.good_seed(spec, n)

    class Rank(ShardedVecNovelGridworld):
        def __init__(self, rank, world):                              # (a rank without a process group: what __init__ derives from it)
            self.rank, self.world, self.global_num_envs = rank, world, n
            self.first, self.num_envs = shard_range(n, world, rank)
            self.local = XO.OracleVecExpand(spec, self.num_envs, seed=seed, env_index_base=self.first, autoreset=True, horizon=9)
            self.spec = spec

    whole = XO.OracleVecExpand(spec, n, seed=seed, autoreset=True, horizon=9)
    whole.reset()
    rs = np.random.RandomState(2)
    acts = rs.randint(0, A, n)
    ws = whole.snapshot(n)
    we = ws.expand(None, acts, None, from_envs=True)
    for rank in range(2):
        env = Rank(rank, 2)
        env.reset()
        s = env.snapshot()
        assert s.env is env.local and s.capacity == n // 2 and callable(s.expand) and callable(s.expand_all)
        local = slice(env.first, env.first + env.num_envs)
        e = s.expand(np.arange(env.num_envs), acts[local], np.arange(env.num_envs), from_envs=True)
        for k in ('reward', 'done', 'result', 'info'):
            assert (e[k] == we[k][local]).all(), (rank, k)
        got, exp = s.state(), ws.state(env.first, env.num_envs)
        assert all((got[k] == exp[k]).all() for k in XO.STATE_KEYS), rank
        with pytest.raises(ValueError, match=r'outside \[0, 8\)'):                   # a GLOBAL env index is out of the shard's range
            s.expand([n - 1], [0], [0], from_envs=True)
        pool = env.snapshot(2 * A)
        t = pool.expand_all([0, 5], 0, from_envs=True)
        assert t.reward.shape == (2, A) and (t.reward[0, acts[env.first]] == e.reward[0]) and (t.info[1, acts[env.first + 5]] == e.info[5])
        env.close()
