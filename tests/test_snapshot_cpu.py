"""Device-side snapshots, host side (no GPU): the index checks of Snapshot.save / restore, the C-ABI surface, the Python surface, and the
sharded env's delegation on the oracle-backed stand-in with the numpy snapshot model (tests/snapshot_oracle.py)."""
import os
import re

import numpy as np
import pytest

import ngw_testlib as T
import snapshot_oracle as SO
from gym_novel_gridworlds_amd import _cabi
from gym_novel_gridworlds_amd.snapshot import check_indices, pair_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAP_API = ['ngw_snapshot_create', 'ngw_snapshot_destroy', 'ngw_snapshot_save', 'ngw_snapshot_restore', 'ngw_snapshot_get']


def test_header_declares_and_library_exports_the_snapshot_api():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    L = _cabi.lib()
    for name in SNAP_API:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert hasattr(L, name), name
        assert name in _cabi.SYMBOLS
    assert re.search(r'#define\s+NGW_F_BAD_INDEX\s+4u', text) and re.search(r'#define\s+NGW_SNAP_KEEP_EPISODE\s+1\b', text)
    from gym_novel_gridworlds_amd.snapshot import KEEP_EPISODE
    from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, F_INVALID_ACTION, F_PLACEMENT
    assert (F_INVALID_ACTION, F_PLACEMENT, F_BAD_INDEX, KEEP_EPISODE) == (1, 2, 4, 1)
    assert L.ngw_abi_version() == 3                                   # (ngw_spec did not change)


def test_null_arguments_are_refused_without_a_device():
    L = _cabi.lib()
    import ctypes as C
    out = C.c_void_p()
    assert L.ngw_snapshot_create(None, 4, C.byref(out)) == -1
    assert L.ngw_snapshot_destroy(None, None) == -1
    assert L.ngw_snapshot_save(None, None, None, None, 1) == -1
    assert L.ngw_snapshot_restore(None, None, None, None, 1, 0) == -1
    assert L.ngw_snapshot_get(None, None, 0, 1, *([None] * 7)) == -1


def test_python_surface():
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.snapshot import Snapshot
    for cls, names in ((VecNovelGridworld, ('snapshot', 'fork')), (ShardedVecNovelGridworld, ('snapshot', 'fork')),
                       (Snapshot, ('save', 'restore', 'state', 'close'))):
        for name in names:
            assert callable(getattr(cls, name, None)), (cls.__name__, name)


def test_index_checks():
    assert check_indices(None, 10) is None
    a = check_indices([3, 1, 2], 4, distinct=True)
    assert a.dtype == np.int32 and a.flags['C_CONTIGUOUS'] and a.tolist() == [3, 1, 2]
    assert check_indices(np.array([5, 5, 0], np.int64), 6).tolist() == [5, 5, 0]          # repeats are fine where not required distinct
    assert check_indices(np.arange(10, dtype=np.uint8)[::2], 9).tolist() == [0, 2, 4, 6, 8]   # (a strided view is made contiguous)
    assert check_indices([], 3, distinct=True).size == 0
    for bad in ([0.0, 1.0], np.array([1.5]), [True, False], ['a'], np.zeros(3, np.float32)):
        with pytest.raises(ValueError, match='integer'):
            check_indices(bad, 10)
    with pytest.raises(ValueError, match='one-dimensional'):
        check_indices(np.zeros((2, 2), np.int32), 10)
    with pytest.raises(ValueError, match='one-dimensional'):
        check_indices(3, 10)
    for bad in ([0, 10], [-1], np.array([2 ** 40]), [3, 4, 11, 2]):
        with pytest.raises(ValueError, match='outside'):
            check_indices(bad, 10)
    with pytest.raises(ValueError, match='twice'):
        check_indices([1, 2, 1], 10, distinct=True)
    assert check_indices([9], 10).tolist() == [9] and check_indices([0], 1).tolist() == [0]


def test_pair_count():
    assert pair_count(None, None, 7) == 7
    assert pair_count(3, None, 7) == 3 and pair_count(None, 4, 7) == 4 and pair_count(5, 5, 7) == 5
    with pytest.raises(ValueError, match='different lengths'):
        pair_count(3, 4, 7)


def test_numpy_model_semantics():
    """The model itself: a fork shares the slot's state, the episode rule, the zero row."""
    m = SO.NumpySnapshot(5, 3, 4)
    z = m.state()
    assert (z['loc'] == 1).all() and all((z[k] == 0).all() for k in SO.STATE_KEYS if k != 'loc')
    from oracle.ngw_oracle import State
    st = State(6, 5, 3)
    rs = np.random.RandomState(0)
    st.map[...] = rs.randint(0, 3, st.map.shape); st.loc[...] = rs.randint(1, 4, st.loc.shape); st.episode[...] = np.arange(6) + 10
    before = st.copy()
    m.save(st, envs=[4, 2], slots=[3, 0])
    m.restore(st, slots=[3, 3, 0], envs=[0, 1, 5])
    assert (st.map[0] == before.map[4]).all() and (st.map[1] == before.map[4]).all() and (st.map[5] == before.map[2]).all()
    assert st.episode.tolist() == [14, 14, 12, 13, 14, 12]
    assert (st.map[2:5] == before.map[2:5]).all()
    m.restore(st, slots=[0], envs=[3], keep_episode=True)
    assert (st.map[3] == before.map[2]).all() and st.episode[3] == 13


def test_sharded_env_delegates_to_its_local_env():
    """ShardedVecNovelGridworld.snapshot / fork are the local env's: rank-local slots, the shard's own env indices."""
    spec = T.build_spec('pogo10')
    n, A = 24, len(spec.actions_id)
    env = SO.sharded_on_oracle(global_num_envs=n, spec=spec, seed=3, autoreset=True, horizon=9)
    ref = SO.OracleVecSnap(spec, n, seed=3, autoreset=True, horizon=9)
    env.reset(); ref.reset()
    rs = np.random.RandomState(1)

    def steps(k):
        for _ in range(k):
            a = rs.randint(0, A, n).astype(np.int32)
            env.step(a); ref.step(a)

    def same():
        a, b = env.local.get_state(), ref.get_state()
        return all((a[k] == b[k]).all() for k in SO.STATE_KEYS)
    steps(5)
    s = env.snapshot(8)
    assert s.capacity == 8 and s.env is env.local
    model = SO.NumpySnapshot(spec.map_size, len(spec.items_id), 8)
    s.save(envs=[3, 17, 9], slots=[7, 0, 2]); model.save(ref.o.st, [3, 17, 9], [7, 0, 2])
    steps(6)
    s.restore(slots=[7, 7, 2, 0], envs=[1, 2, 23, 9]); model.restore(ref.o.st, [7, 7, 2, 0], [1, 2, 23, 9])
    assert same()
    st = s.state()
    assert all((st[k] == model.state()[k]).all() for k in SO.STATE_KEYS)
    steps(20)
    assert same()
    src = rs.randint(0, n, n)
    env.fork(src); ref.fork(src)
    steps(20)
    assert same()
    # forks of one env share the rest of the episode and differ from the next reset on
    env.fork(np.zeros(n, np.int64))
    st = env.local.get_state()
    assert (st['map'] == st['map'][0]).all() and (st['episode'] == st['episode'][0]).all()
    a = np.full(n, spec.actions_id['Left'], np.int32)
    left = 9 - int(st['step_count'][0])
    for _ in range(left - 1):
        env.step(a)
    st = env.local.get_state()
    assert (st['map'] == st['map'][0]).all() and (st['facing'] == st['facing'][0]).all()
    env.step(a)                                                       # the horizon: every env resets from its OWN stream
    st = env.local.get_state()
    assert (st['episode'] == st['episode'][0]).all() and len({st['map'][i].tobytes() + st['loc'][i].tobytes() for i in range(n)}) > n // 2
    # inject_novelty closes the shard's snapshots
    from gym_novel_gridworlds_amd import inject_novelty
    inject_novelty(env, 'axe', 'medium', 'wooden', '')
    with pytest.raises(ValueError, match='closed'):
        s.save()
    env.close()
