"""The AgentMap window kept current, host side (no GPU): the export and its argument checks that need no device, the Python surface and its
argument checking, the pass-through of the sharded env and of LimitActions, and the contract itself - which calls leave the kept buffer
current, which make it stale - stated once on an oracle-backed stand-in (ngw_testlib.OracleVec plus the switch) whose windows come from the
numpy builder of tests/slot_observe_oracle.py.  tests/test_agent_view_fused.py holds the device to the same contract."""
import os
import re

import numpy as np
import pytest

import ngw_testlib as T
import slot_observe_oracle as OO
from gym_novel_gridworlds_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym_novel_gridworlds_amd', 'csrc')


def test_header_declares_and_library_exports_the_entry_point():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+ngw_agent_view_fuse\s*\(\s*ngw_handle\s*\*\s*h\s*,\s*int\s+view_size\s*,\s*int\s+on\s*\)', text)
    L = _cabi.lib()
    assert hasattr(L, 'ngw_agent_view_fuse') and 'ngw_agent_view_fuse' in _cabi.SYMBOLS
    assert L.ngw_abi_version() == 3                              # (an added export: the version stays)
    assert 'ngw_agent_view_fuse' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_null_handle_is_refused_without_a_gpu():
    L = _cabi.lib()
    for on in (0, 1, 2):
        assert L.ngw_agent_view_fuse(None, 5, on) == _cabi.E_INVALID_ARG
        assert 'NULL' in _cabi.last_error()


def test_python_argument_checking_happens_before_the_library_is_called():
    from gym_novel_gridworlds_amd.vec_env import VecNovelGridworld, check_view_size
    v = VecNovelGridworld.__new__(VecNovelGridworld)             # (no handle: a call that reached the library would fail differently)
    for bad in (0, 128, -3, True, 2.0, '5', [5]):
        with pytest.raises(ValueError, match='view_size'):
            v.set_agent_view(bad)
        with pytest.raises(ValueError):
            check_view_size(bad)
    assert check_view_size(np.int64(127)) == 127 and check_view_size(1) == 1


def test_python_surface_has_the_methods():
    from gym_novel_gridworlds_amd import LimitActions, VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    for cls in (VecNovelGridworld, ShardedVecNovelGridworld, LimitActions):
        for name in ('set_agent_view', 'agent_view'):
            assert callable(cls.__dict__.get(name)), (cls.__name__, name)       # (defined there, not reached through __getattr__)
    assert callable(VecNovelGridworld.agent_view_observation) and callable(ShardedVecNovelGridworld.agent_view_observation)


def test_every_writer_of_the_state_ends_the_buffers_freshness_in_one_place():
    """The library's rule (ngw_abi_launch.cpp state_written): whatever writes the state clears view_fresh there, and only a launch that has left
    the windows behind it sets it."""
    text = open(os.path.join(CSRC, 'ngw_abi_launch.cpp')).read()
    body = text[text.index('void state_written('):]
    body = body[:body.index('\n}\n')]
    assert 'h->view_fresh = false;' in body
    sets = [f for f in sorted(os.listdir(CSRC)) if f.startswith('ngw_abi_') and 'view_fresh = true' in open(os.path.join(CSRC, f)).read()]
    assert sets == ['ngw_abi_launch.cpp', 'ngw_abi_obs.cpp'], sets


class ViewVec(T.OracleVec):
    """OracleVec with the switch: `buf` is the kept buffer, written by the calls the contract names and by nothing else; `gathers` counts
    the stand-alone gathers agent_view() had to run."""

    def __init__(self, *a, **kw):
        T.OracleVec.__init__(self, *a, **kw)
        self.cfg, self.buf, self.fresh, self.gathers, self.calls = None, None, False, 0, []

    def _window(self, V):
        st = self.o.st
        rows = dict(map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, selected=st.selected, step_count=st.step_count)
        return OO.expect_view(rows, np.arange(self.num_envs), V)['agent_map']

    def _committed(self):
        if self.cfg:
            self.buf[...] = self._window(self.cfg[0])
            self.fresh = True

    def set_agent_view(self, view_size=5, fused=True):
        from gym_novel_gridworlds_amd.vec_env import check_view_size
        self.calls.append(('set_agent_view', view_size, fused))
        if view_size is None:
            self.cfg, self.fresh = None, False
            return
        V = check_view_size(view_size)
        self.cfg = (V, bool(fused))
        self.buf = np.zeros((self.num_envs, 2 * V + 1, 2 * V + 1), np.int8)
        self._committed()

    def agent_view(self, view_size=5, device=False, copy=False):
        self.calls.append(('agent_view', view_size, device, copy))
        if not self.cfg or view_size != self.cfg[0]:
            self.gathers += 1
            return self._window(view_size)
        if not self.fresh:
            self.gathers += 1
            self._committed()
        return self.buf.copy() if copy else self.buf

    def step(self, actions, copy=False):
        out = T.OracleVec.step(self, actions, copy)
        self._committed()
        return out

    def reset(self, mask=None, copy=False):
        T.OracleVec.reset(self, mask, copy)
        self._committed()

    def set_state(self, *a, **kw):
        T.OracleVec.set_state(self, *a, **kw)
        self.fresh = False


def test_which_calls_keep_the_buffer_current_and_which_make_it_stale():
    spec = T.build_spec('pogo10')
    n, V = 70, 2
    v = ViewVec(spec, n, seed=5)
    v.reset()
    v.set_agent_view(V)
    rs = np.random.RandomState(2)
    A = len(spec.actions_id)
    for t in range(6):
        v.step(rs.randint(0, A, n).astype(np.int32))
        assert (v.buf == v._window(V)).all() and v.fresh, t          # current without a call
    got = v.agent_view(V)
    assert got is v.buf and v.gathers == 0                           # ... and agent_view() launches nothing
    v.agent_view(V)
    assert v.gathers == 0
    v.reset((np.arange(n) % 3 == 0).astype(np.uint8))
    assert (v.buf == v._window(V)).all() and v.gathers == 0
    st = v.get_state()
    st['loc'][:] = np.roll(st['loc'], 1, axis=0)
    v.set_state(0, loc=st['loc'])                                    # written outside a step: stale until asked for
    assert not v.fresh
    assert (v.agent_view(V) == v._window(V)).all() and v.gathers == 1
    v.agent_view(V)
    assert v.gathers == 1
    other = v.agent_view(5)                                          # another size: its own result, the kept buffer untouched
    assert other.shape == (n, 11, 11) and v.gathers == 2 and v.fresh and (v.buf == v._window(V)).all()
    v.set_agent_view(None)
    v.step(rs.randint(0, A, n).astype(np.int32))
    assert not v.fresh and (v.agent_view(V) == v._window(V)).all() and v.gathers == 3
    for bad in (0, 128, True):
        with pytest.raises(ValueError):
            v.set_agent_view(bad)


def test_sharded_env_and_limit_actions_pass_the_calls_through():
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    spec = T.build_spec('pogo10')
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    sh = ShardedVecNovelGridworld.__new__(ShardedVecNovelGridworld)  # (no process group here: the methods under test touch `local` alone)
    sh.local = ViewVec(spec, 70, seed=5)
    sh.local.reset()
    sh.set_agent_view(2, fused=False)
    assert sh.local.calls[-1] == ('set_agent_view', 2, False) and sh.local.cfg == (2, False)
    assert sh.agent_view(2) is sh.local.buf and sh.local.calls[-1] == ('agent_view', 2, False, False)
    sh.agent_view(3, device=False, copy=True)
    assert sh.local.calls[-1] == ('agent_view', 3, False, True)
    sh.set_agent_view(None)
    assert sh.local.cfg is None

    class Inner:                                                     # what LimitActions wraps: anything with the two methods
        action_space = observation_space = None

        def __init__(self):
            self.vec = ViewVec(spec, 1, seed=5)
            self.vec.reset()

        def set_agent_view(self, view_size=5, fused=True):
            return self.vec.set_agent_view(view_size, fused=fused)

        def agent_view(self, view_size=5, device=False, copy=False):
            return self.vec.agent_view(view_size, device=device, copy=copy)
    inner = Inner()
    w = LimitActions(inner, {'Forward', 'Left', 'Right', 'Break'})
    w.set_agent_view(2)
    assert inner.vec.calls[-1] == ('set_agent_view', 2, True)
    assert (w.agent_view(2) == inner.vec._window(2)).all() and inner.vec.calls[-1] == ('agent_view', 2, False, False)
    w.set_agent_view(None)
    assert inner.vec.cfg is None
