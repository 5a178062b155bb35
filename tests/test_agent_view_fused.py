"""The AgentMap window kept current by the batched step (set_agent_view, include/ngw.h ngw_agent_view_fuse; the step kernel's VIEW form in
csrc/ngw_lean_step.inc), held to the CPU oracle: after every committed step and reset the handle's view buffer - read where it lies, without
another call - is the window the numpy builder of tests/slot_observe_oracle.py cuts out of the unmodified oracle's state, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import ngw_testlib as T
import slot_observe_oracle as OO
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu


def rows_of(o):
    st = o.st
    return dict(map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, selected=st.selected, step_count=st.step_count)


def expect(o, V):
    return OO.expect_view(rows_of(o), np.arange(o.st.map.shape[0]), V)['agent_map']


def good_seed(spec, n, lo=4, **kw):
    return next(sd for sd in range(lo, lo + 40) if not Oracle(spec.compile(), n, seed=sd, **kw).reset() & 2)   # (tight maps can exhaust the placement)


class Pair:
    """A batched env with the switch on and the oracle beside it; `buf` is the handle's view buffer, fetched ONCE."""

    def __init__(self, cfg, n, V, fused=True, map_size=None, autoreset=False, horizon=0, prefetch=None, before=None):
        self.spec = spec = T.build_spec(cfg, map_size)
        seed = good_seed(spec, n)
        self.n, self.V, self.A = n, V, len(spec.actions_id)
        self.v = v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=autoreset, horizon=horizon)
        self.o = Oracle(spec.compile(), n, seed=seed, autoreset=autoreset, horizon=horizon)
        if prefetch is not None:
            v.set_reset_prefetch(prefetch)
        if before is not None:
            before(v)
        v.reset()
        self.o.reset()
        v.set_agent_view(V, fused=fused)
        self.buf = v.agent_view(V, device=True)
        self.rs = np.random.RandomState(11)

    def check(self, where):
        self.v.sync()
        got, exp = self.buf.cpu().numpy(), expect(self.o, self.V)
        assert got.dtype == np.int8 and got.shape == exp.shape, (where, got.dtype, got.shape, exp.shape)
        bad = np.nonzero((got != exp).reshape(self.n, -1).any(1))[0]
        assert bad.size == 0, (where, 'envs', bad[:6], got[bad[0]], exp[bad[0]])

    def actions(self, T_=1):
        return self.rs.randint(0, self.A, (T_, self.n)).astype(np.int32)

    def step(self, act):
        import torch
        ad = torch.as_tensor(act, device=self.buf.device)
        self.v.step_device(ad.data_ptr())
        self.v.sync()                                            # (`ad` goes away with this frame)
        self.o.step(act)

    def close(self):
        assert self.v.error_flags() == 0
        self.v.close()


SHAPES = [('pogo10', None, 5, 70), ('pogo10', None, 1, 130), ('add11e', None, 5, 70), ('bow10', 12, 5, 130), ('pogo10', 32, 16, 70),
          ('fire10h', None, 5, 130), ('fire10h', None, 2, 70), ('axe10', None, 5, 70), ('jump12', None, 5, 70),
          ('add11e', None, 2, 130), ('axe10', None, 2, 70), ('jump12', None, 2, 130), ('pogo10', 32, 2, 70)]


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('cfg,S,V,n', SHAPES)
def test_buffer_is_current_after_every_step(cfg, S, V, n, fused):
    """Random actions, no autoreset: windows that hang over every edge (view_size 5 on 10 x 10), view_size 1, odd S * S (11 x 11: rows start at any
    byte), 12 x 12 Bow, a 33 x 33 window on a 32 x 32 map, a FireWall configuration (the EXT instantiation), the axe configuration (an entity
    pick-up changes cells near the agent) and Jump (outside the plain class); 70 and 130 envs end in a partial wave.  fused=False: the gather.
    view_size 1 and 2 are built by the step kernel itself (its plain, general and EXT instantiations), the larger ones by the gather behind it."""
    p = Pair(cfg, n, V, fused, S)
    p.check('after the switch-on')
    for t in range(12):
        p.step(p.actions()[0])
        p.check('%s step %d' % (cfg, t))
    p.close()


def test_window_wider_than_the_map_at_the_top_of_the_range():
    """view_size 127 (a 255 x 255 window on a 10 x 10 map): beyond what the step kernel builds itself, so the gather follows the step."""
    p = Pair('pogo10', 70, 127)
    for t in range(2):
        p.step(p.actions()[0])
        p.check('step %d' % t)
    p.close()


@pytest.mark.parametrize('fused', [True, False])
def test_agents_on_edges_and_in_corners(fused):
    """A scripted prefix drives the agents along each edge and into the corners: with view_size 2 on 10 x 10 zeros appear on one side, then on two."""
    p = Pair('pogo10', 70, 2, fused)
    ids = p.spec.actions_id
    script = []
    for _ in range(4):
        script += [ids['Forward']] * 9 + [ids['Left']]
    seen = set()
    for t, a in enumerate(script):
        p.step(np.full(p.n, a, np.int32))
        p.check('script step %d' % t)
        loc = p.o.st.loc
        seen |= {(int(r <= 1), int(c <= 1), int(r >= 8), int(c >= 8)) for r, c in loc}
    for side in range(4):
        assert any(s[side] for s in seen), side                  # an agent stood beside every wall
    assert any(sum(s) == 2 for s in seen)                        # ... and in a corner
    p.close()


@pytest.mark.parametrize('cfg,V', [('pogo10', 2), ('fire10h', 2), ('pogo10', 5)])
@pytest.mark.parametrize('prefetch', [2, 0])
@pytest.mark.parametrize('fused', [True, False])
def test_autoreset_with_prepared_and_inline_episodes(cfg, V, prefetch, fused):
    """horizon 3, the envs' step counts staggered by a masked reset: episodes end on different steps inside one wave, the new episode swapped in
    from a prepared row (refills every 2 steps) or drawn inline (prepared episodes off).  The window is the new episode's first state.
    view_size 2: the step kernel's own epilogue behind its cold path; 5: the gather behind the step."""
    p = Pair(cfg, 130, V, fused, autoreset=True, horizon=3, prefetch=prefetch)
    p.step(p.actions()[0])
    mask = (np.arange(p.n) % 3 == 0).astype(np.uint8)
    p.v.reset(mask)
    p.o.reset(mask)
    p.check('after reset(mask)')
    partial = 0
    for t in range(9):
        p.step(p.actions()[0])
        p.check('%s step %d' % (cfg, t))
        ended = np.asarray(p.o.done[:64]).astype(bool)
        partial += int(0 < ended.sum() < 64)
    assert partial >= 3, "no step reset only some lanes of a wave"
    p.close()


def test_coexists_with_fused_masks_and_fused_lidar():
    """With set_action_masks(True), and with lidar_configure(fused=True), the step kernel has no VIEW form: the gather follows, and all three
    observations describe the state the step left."""
    lc = OO.lidar_config('pogo10')
    for what in ('masks', 'lidar', 'both'):
        def before(v):
            if what != 'masks':
                v.lidar_configure(lc, fused=True)
            if what != 'lidar':
                v.set_action_masks(True)
        p = Pair('pogo10', 130, 5, True, autoreset=True, horizon=5, before=before)
        idx = np.arange(p.n)
        for t in range(7):
            p.step(p.actions()[0])
            p.check('%s step %d' % (what, t))
            if what != 'lidar':
                OO.assert_masks(p.v.action_masks(), p.spec, rows_of(p.o), idx, '%s step %d' % (what, t))
            if what != 'masks':
                OO.assert_lidar(p.v, p.v.lidar_observation(copy=True), p.spec, lc, rows_of(p.o), idx, '%s step %d' % (what, t))
        p.close()


@pytest.mark.parametrize('cfg,V', [('pogo10', 2), ('fire10h', 2), ('axe10', 2), ('pogo10', 5)])
def test_multi_step_calls_graphs_host_steps_and_resets(cfg, V):
    import torch
    p = Pair(cfg, 130, V, True, autoreset=True, horizon=4)
    v, o, n = p.v, p.o, p.n
    act = p.actions(5)
    ad = torch.as_tensor(act, device=p.buf.device)
    v.step_device_many(ad.data_ptr(), n, 5)
    for t in range(5):
        o.step(act[t])
    p.check('step_device_many')
    v.graph_build(ad.data_ptr(), n, 5)
    v.graph_launch(2)
    for rep in range(2):
        for t in range(5):
            o.step(act[t])
    p.check('graph replayed twice')
    a = p.actions()[0]
    v.step(a)
    o.step(a)
    p.check('host step')
    got = v.agent_view(V, device=False)
    assert (got == expect(o, V)).all(), 'agent_view(device=False) after a host step'
    mask = (np.arange(n) % 7 == 2).astype(np.uint8)
    v.reset(mask)
    o.reset(mask)
    p.check('reset(mask)')
    v.reset()
    o.reset()
    p.check('reset')
    w = torch.ones((p.A, n), dtype=torch.float32, device=p.buf.device)
    s = v.step_sampled(w, 77)
    v.sync()
    o.step(s.action.cpu().numpy().astype(np.int32))
    p.check('step_sampled')
    p.close()


def test_state_written_outside_a_step_is_refreshed_not_served_stale():
    """fork() and snap.restore() change the state without a step: agent_view() gathers again; a second call launches nothing - the buffer,
    overwritten through its zero-copy view in between, comes back as it was left (the hook of tests/test_lookahead.py)."""
    import torch
    p = Pair('pogo10', 130, 5, True)
    v, o, n = p.v, p.o, p.n
    for t in range(4):
        p.step(p.actions()[0])

    def poisoned():
        p.buf.fill_(-77)
        torch.cuda.synchronize()
        return bool((v.agent_view(5, copy=True) == -77).all())

    assert v.agent_view(5, device=True).data_ptr() == p.buf.data_ptr()
    assert poisoned(), "agent_view() on a current buffer launched the gather"
    assert poisoned()
    snap = v.snapshot()
    snap.save()
    saved = o.st.copy()
    p.step(p.actions()[0])
    p.check('step after the poison')
    snap.restore()
    o.st = saved.copy()
    assert not poisoned(), "a restored state was served from the stale buffer"
    assert (v.agent_view(5, copy=True) == expect(o, 5)).all(), 'after snap.restore()'
    assert poisoned()
    src = (np.arange(n)[::-1]).astype(np.int32)
    v.fork(src)
    for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode'):
        getattr(o.st, k)[...] = getattr(o.st, k)[src]
    assert (v.agent_view(5, copy=True) == expect(o, 5)).all(), 'after fork()'
    # another size: its own result, and the kept buffer keeps its contract
    assert (v.agent_view(2, copy=True) == expect(o, 2)).all()
    assert v.agent_view(2, device=True).data_ptr() != p.buf.data_ptr()
    p.step(p.actions()[0])
    p.check('step after a window of another size')
    assert poisoned()
    p.close()


def test_switch_off_returns_to_gathering_on_demand():
    p = Pair('pogo10', 70, 5, True)
    p.step(p.actions()[0])
    p.check('on')
    p.v.set_agent_view(None)
    p.buf.fill_(-77)
    p.step(p.actions()[0])
    p.v.sync()
    assert bool((p.buf == -77).all()), "a step wrote the view buffer with the switch off"
    assert (p.v.agent_view(5, copy=True) == expect(p.o, 5)).all()
    p.buf.fill_(-77)
    assert (p.v.agent_view(5, copy=True) == expect(p.o, 5)).all(), "switched off, every agent_view() gathers"
    p.close()


def test_argument_errors_of_the_entry_point():
    L = _cabi.lib()
    assert L.ngw_agent_view_fuse(None, 5, 1) == _cabi.E_INVALID_ARG and 'NULL' in _cabi.last_error()
    v = VecNovelGridworld(spec=T.build_spec('pogo10'), num_envs=70, seed=4)
    v.reset()
    for V in (0, 128, -1):
        assert L.ngw_agent_view_fuse(v._h, V, 1) == _cabi.E_INVALID_ARG
        assert 'view_size must be in 1..127' in _cabi.last_error()
    assert L.ngw_agent_view_fuse(v._h, 5, 3) == _cabi.E_INVALID_ARG
    for bad in (0, 128, True, 2.5, '5'):
        with pytest.raises(ValueError):
            v.set_agent_view(bad)
    p = C.c_void_p()
    assert L.ngw_agent_view_fuse(v._h, 5, 1) == 0 and L.ngw_agent_view_device_ptr(v._h, C.byref(p)) == 0 and p.value
    assert v.error_flags() == 0
    v.close()
