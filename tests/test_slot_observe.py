"""Slot observations on the MI355X (csrc/ngw_slot_observe.inc, include/ngw.h ngw_snapshot_lidar / _agent_view / _action_mask, snapshot.py
Snapshot.lidar_observation / agent_view / action_masks), held to the CPU oracle applied to a host copy of the slots
(tests/slot_observe_oracle.py) - never to the device's own env-side observation calls."""
import ctypes as C

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import slot_observe_oracle as SO
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.lidar import LidarConfig
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_ALL = sorted(T.CFGS)


def dev_i32(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def grow(v, pool, n, rs, A):
    """Slots 0 .. n-1 := the envs, slots n .. 2n-1 := one generation of children of them: states no env is in."""
    pool.save(slots=np.arange(n))
    pool.expand(rs.randint(0, n, n), rs.randint(0, A, n), n + np.arange(n))


@pytest.mark.parametrize('cfg', CFG_ALL)
def test_every_configuration(cfg):
    """130 envs (two full waves and a partial one) after reset and after ~40 random steps; the pool holds the envs' states and a generation
    of children; 200 random slots with repeats.  Masks and agent view for every configuration, lidar (8 beams, int32) where
    tests/test_lidar.py has the configuration."""
    spec = T.build_spec(cfg)
    n, A = 130, len(spec.actions_id)
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=25)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=25)
    lc = SO.lidar_config(cfg) if cfg in SO.LIDAR_CFGS else None
    if lc is not None:
        v.lidar_configure(lc, dtype=np.int32)
    v.reset(); o.reset()
    pool = v.snapshot(2 * n)
    rs = np.random.RandomState(17)
    for stage in ('after reset', 'after random play'):
        if stage == 'after random play':
            for t in range(40):
                a = rs.randint(0, A, n).astype(np.int32)
                if o.step(a) & 2:                               # a tight map exhausted the placement of an autoreset: stop here
                    break
                v.step(a)
        where = '%s %s' % (cfg, stage)
        grow(v, pool, n, rs, A)
        rows = pool.state()
        slots = rs.randint(0, 2 * n, 200)
        SO.assert_masks(pool.action_masks(slots), spec, rows, slots, where)
        SO.assert_view(pool.agent_view(slots, view_size=5), rows, slots, 5, where)
        if lc is not None:
            got = pool.lidar_observation(slots)
            assert got.dtype == np.int32
            SO.assert_lidar(v, got, spec, lc, rows, slots, where)
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('S', [9, 10, 12, 32])
@pytest.mark.parametrize('count', [1, 63, 65, 200])
def test_map_sizes_and_counts(S, count):
    """One map size per staging form of the lidar gather (odd S*S with its byte tail: 9, dwords: 10, 16-byte pieces: 12) and the size whose
    lidar launch needs the LDS opt-in above 64 KiB (32); counts around the wavefront width and far above num_envs = 5.  Host lists, device
    tensors with the results left on the device, and slots=None on a small snapshot."""
    import torch
    spec = make_spec(T.POGO, S)
    n, A, cap = 5, len(spec.actions_id), 256
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=30)
    lc = LidarConfig(spec, 8)
    v.lidar_configure(lc, dtype=np.int32)
    v.reset()
    rs = np.random.RandomState(S + count)
    for t in range(25):
        v.step(rs.randint(0, A, n).astype(np.int32))
    pool = v.snapshot(cap)
    pool.expand(rs.randint(0, n, cap), rs.randint(0, A, cap), np.arange(cap), from_envs=True)      # every slot a state of its own
    rows = pool.state()
    where = 'S=%d count=%d' % (S, count)
    slots = rs.randint(0, cap, count)
    SO.assert_masks(pool.action_masks(slots), spec, rows, slots, where + ' host list')
    SO.assert_view(pool.agent_view(slots), rows, slots, 5, where + ' host list')
    SO.assert_lidar(v, pool.lidar_observation(slots), spec, lc, rows, slots, where + ' host list')
    slots = rs.randint(0, cap, count)
    d = dev_i32(slots)
    m, w, l = pool.action_masks(d, device=True), pool.agent_view(d, device=True), pool.lidar_observation(d, device=True)
    assert isinstance(m, torch.Tensor) and m.dtype == torch.bool and tuple(m.shape) == (count, A)
    assert w['agent_map'].dtype == torch.int8 and tuple(w['agent_map'].shape) == (count, 11, 11) and w['agent_facing_id'].dtype == torch.int32
    assert l.dtype == torch.int32 and tuple(l.shape) == (count, v.lidar_len)
    SO.assert_masks(m, spec, rows, slots, where + ' device tensor')
    SO.assert_view(w, rows, slots, 5, where + ' device tensor')
    SO.assert_lidar(v, l, spec, lc, rows, slots, where + ' device tensor')
    small = v.snapshot(7)
    small.expand(rs.randint(0, n, 7), rs.randint(0, A, 7), None, from_envs=True)
    srows, every = small.state(), np.arange(7)
    SO.assert_masks(small.action_masks(), spec, srows, every, where + ' every slot')
    SO.assert_view(small.agent_view(), srows, every, 5, where + ' every slot')
    SO.assert_lidar(v, small.lidar_observation(), spec, lc, srows, every, where + ' every slot')
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('cfg,beams', [('pogo10', 8), ('bowaxe16', 12), ('pogo13', 5), ('pogo13', 16), ('add32', 4), ('bow20', 6)])
@pytest.mark.parametrize('dtype', [np.int32, np.int16, 'packed'])
def test_lidar_row_formats_and_marches(cfg, beams, dtype):
    """Every row format x the three marches of the stand-alone form - the constant-offset one (8 beams at 10 x 10), the world-frame table
    (beam counts that are a multiple of 4), the per-lane table (any other count) -, 65 slots with repeats; the env's fused path is on for
    half of them (the slot call runs the LDS march whichever form the env uses)."""
    spec = T.build_spec(cfg)
    n, A = 70, len(spec.actions_id)
    lc = LidarConfig(spec, beams)
    seed = XO.good_seed(spec, n)
    rs = np.random.RandomState(beams)
    for fused in (False, True):
        v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=13)
        v.lidar_configure(lc, fused=fused, dtype=dtype)
        v.reset()
        for t in range(12):
            v.step(rs.randint(0, A, n).astype(np.int32))
        pool = v.snapshot(2 * n)
        grow(v, pool, n, rs, A)
        rows = pool.state()
        slots = rs.randint(0, 2 * n, 65)
        got = pool.lidar_observation(slots)
        if dtype == 'packed':
            assert got[0].dtype == np.uint8 and got[1].dtype == np.int16 and got[0].shape == (65, beams * len(lc.lidar_items_id))
        else:
            assert got.dtype == np.dtype(dtype)
        where = '%s beams=%d fused=%d' % (cfg, beams, fused)
        SO.assert_lidar(v, got, spec, lc, rows, slots, where)
        SO.assert_lidar(v, pool.lidar_observation(dev_i32(slots), device=True), spec, lc, rows, slots, where + ' device')
        assert v.error_flags() == 0
        v.close()


def _everything(v, snaps):
    st = v.get_state()
    reward, done, info = v.get_step_out(copy=True)
    out = {k: st[k].copy() for k in XO.STATE_KEYS}
    out.update(reward=reward, done=done, words=v.action_mask_words(copy=True))
    out.update({'info_' + k: np.asarray(info[k]).copy() for k in ('result', 'step_cost_code', 'message_code', 'message_arg')})
    out.update({'look_' + k: np.asarray(x) for k, x in zip(('reward', 'done', 'result', 'info'), v.lookahead(copy=True))})
    out['lidar'] = v.lidar_observation(copy=True)
    for i, s in enumerate(snaps):
        out.update({'snap%d_%s' % (i, k): x for k, x in s.state().items()})
    return out


def test_nothing_is_committed():
    """Fused lidar, masks-in-step, terminal capture, autoreset under a horizon; after a step and a lookahead (masks and table current)
    the three slot calls leave every recorded byte as it was: the state, the last step's outputs, the env's lidar rows, masks, lookahead
    table, and both snapshots.  The derived buffers stay CURRENT: poisoned through their zero-copy views, they read back poisoned."""
    import torch
    spec = T.build_spec('fire10h')
    n, A, H = 130, len(spec.actions_id), 12
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    lc = LidarConfig(spec, 8)
    v.lidar_configure(lc, fused=True, dtype=np.int32)
    v.set_action_masks(True)
    v.set_terminal_capture(True)
    v.reset()
    rs = np.random.RandomState(23)
    pool, other = v.snapshot(2 * n), v.snapshot(n)
    for t in range(9):
        v.step(rs.randint(0, A, n).astype(np.int32))
    grow(v, pool, n, rs, A)
    other.save()
    v.step(rs.randint(0, A, n).astype(np.int32))
    v.lookahead()
    before = _everything(v, (pool, other))
    rows = pool.state()

    def observe(where):
        slots = rs.randint(0, 2 * n, 150)
        SO.assert_masks(pool.action_masks(slots), spec, rows, slots, where)
        SO.assert_view(pool.agent_view(slots, view_size=3), rows, slots, 3, where)
        SO.assert_lidar(v, pool.lidar_observation(slots), spec, lc, rows, slots, where)
        d = dev_i32(slots)
        pool.action_masks(d, device=True), pool.agent_view(d, device=True), pool.lidar_observation(d, device=True)
        other.action_masks(), other.agent_view(), other.lidar_observation()
    observe('first round')
    after = _everything(v, (pool, other))
    assert sorted(before) == sorted(after)
    for k in before:
        assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), k
    v.lookahead(device=True)['reward'].fill_(-77)                # both derived buffers poisoned through their zero-copy views
    v.action_mask_words(device=True).fill_(-1)
    torch.cuda.synchronize()
    observe('second round')
    assert (v.lookahead(copy=True)['reward'] == -77).all(), "a slot observation made the lookahead table stale"
    assert (v.action_mask_words(copy=True) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "a slot observation made the action masks stale"
    assert v.error_flags() == 0
    v.close()


def test_lookahead_and_masks_answer_the_same_afterwards():
    """lookahead() / action_masks() called again behind the slot calls return what they returned before them."""
    spec = T.build_spec('axe10')
    n, A = 130, len(spec.actions_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n), autoreset=True, horizon=20)
    v.lidar_configure(LidarConfig(spec, 8), fused=True, dtype=np.int32)
    v.set_action_masks(True)
    v.reset()
    rs = np.random.RandomState(2)
    pool = v.snapshot(2 * n)
    grow(v, pool, n, rs, A)
    v.step(rs.randint(0, A, n).astype(np.int32))
    look0, masks0 = [np.asarray(x).copy() for x in v.lookahead(copy=True)], v.action_masks().copy()
    pool.action_masks(), pool.agent_view(), pool.lidar_observation()
    look1, masks1 = v.lookahead(copy=True), v.action_masks()
    assert all((a == np.asarray(b)).all() for a, b in zip(look0, look1)) and (masks0 == masks1).all()
    assert v.error_flags() == 0
    v.close()


def test_bad_indices_give_zero_rows_and_raise_the_flag():
    """Device tensors holding -1 and `capacity` among valid slots (a bad one in each wave): those rows are all zero, the others correct,
    F_BAD_INDEX is raised once per call and is 0 thereafter.  Nothing beyond these two values: the point is the clamp."""
    spec = T.build_spec('axe10')
    n, A, cap = 70, len(spec.actions_id), 140
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n))
    lc = LidarConfig(spec, 8)
    v.lidar_configure(lc, dtype=np.int32)
    v.reset()
    rs = np.random.RandomState(8)
    pool = v.snapshot(cap)
    grow(v, pool, n, rs, A)
    rows = pool.state()
    count = 66
    slots = rs.randint(0, cap, count)
    slots[5], slots[65] = -1, cap
    good = np.ones(count, bool)
    good[[5, 65]] = False
    d = dev_i32(slots)
    assert v.error_flags() == 0
    m = pool.action_masks(d)
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    assert not m[~good].any()
    SO.assert_masks(m[good], spec, rows, slots[good], 'masks beside bad indices')
    w = pool.agent_view(d)
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    assert all(not w[k][~good].any() for k in w)
    SO.assert_view({k: x[good] for k, x in w.items()}, rows, slots[good], 5, 'views beside bad indices')
    l = pool.lidar_observation(d)
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    assert not l[~good].any()
    SO.assert_lidar(v, l[good], spec, lc, rows, slots[good], 'lidar rows beside bad indices')
    v.close()


@pytest.mark.parametrize('view_size', [1, 5, 12])
def test_agent_view_sizes_null_outputs_and_the_border(view_size):
    """Agents on the border ring's neighbours (injected with set_state + save) and in the middle; every subset of the three outputs
    requested at the C-ABI level, the others NULL."""
    import torch
    spec = T.build_spec('pogo10')
    S, n = spec.map_size, 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n))
    v.reset()
    st = v.get_state()
    ring = [(1, 1), (1, S - 2), (S - 2, 1), (S - 2, S - 2), (1, S // 2), (S - 2, S // 2), (S // 2, 1), (S // 2, S - 2), (S // 2, S // 2)]
    loc = np.array([ring[i % len(ring)] for i in range(n)], np.int32)
    v.set_state(0, map=st['map'], loc=loc, facing=(np.arange(n) % 4).astype(np.int32), inv=st['inv'], selected=st['selected'],
                step_count=st['step_count'])
    pool = v.snapshot(n)
    pool.save()
    rows = pool.state()
    assert (rows['loc'] == loc).all()
    rs = np.random.RandomState(view_size)
    slots = rs.randint(0, n, 67)
    where = 'view_size=%d' % view_size
    SO.assert_view(pool.agent_view(slots, view_size=view_size), rows, slots, view_size, where)
    exp = SO.expect_view(rows, slots, view_size)
    W, K, d = 2 * view_size + 1, rows['inv'].shape[1], dev_i32(slots)
    for mask in range(1, 8):
        view = torch.full(((67 * W * W + 3) // 4 * 4,), 99, dtype=torch.int8, device='cuda')
        facing = torch.full((67,), 99, dtype=torch.int32, device='cuda')
        inv = torch.full((67, K), 99, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        ptr = [C.c_void_p(t.data_ptr()) if mask >> i & 1 else None for i, t in enumerate((view, facing, inv))]
        _cabi.check(_cabi.lib().ngw_snapshot_agent_view(v._h, pool._s, C.c_void_p(d.data_ptr()), 67, view_size, *ptr))
        v.sync()
        got = (view[:67 * W * W].view(67, W, W).cpu().numpy(), facing.cpu().numpy(), inv.cpu().numpy())
        for i, k in enumerate(('agent_map', 'agent_facing_id', 'inventory_items_quantity')):
            assert (got[i] == (exp[k] if mask >> i & 1 else 99)).all(), (where, mask, k)
    assert v.error_flags() == 0
    v.close()


def test_errors():
    """lidar_observation before lidar_configure and a closed snapshot raise; each NGW_E_INVALID_ARG case of include/ngw.h; count == 0 is a
    no-op."""
    import torch
    L = _cabi.lib()
    spec = T.build_spec('pogo10')
    n = 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    w = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset(); w.reset()
    s, foreign = v.snapshot(8), w.snapshot(8)
    s.save(slots=np.arange(8), envs=np.arange(8))
    with pytest.raises(ValueError, match='lidar_configure'):
        s.lidar_observation()
    buf = torch.zeros(1 << 16, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    out, E = C.c_void_p(buf.data_ptr()), _cabi.E_INVALID_ARG
    assert L.ngw_snapshot_lidar(v._h, s._s, None, 8, out) == E and 'ngw_lidar_configure' in _cabi.last_error()
    v.lidar_configure(LidarConfig(spec, 8), dtype=np.int32)
    calls = [lambda h, sn, sl, c, o: L.ngw_snapshot_lidar(h, sn, sl, c, o),
             lambda h, sn, sl, c, o: L.ngw_snapshot_agent_view(h, sn, sl, c, 5, o, None, None),
             lambda h, sn, sl, c, o: L.ngw_snapshot_action_mask(h, sn, sl, c, o)]
    for X in calls:
        assert X(None, s._s, None, 8, out) == E and 'NULL' in _cabi.last_error()
        assert X(v._h, None, None, 8, out) == E and 'NULL' in _cabi.last_error()
        assert X(v._h, s._s, None, 8, None) == E and 'NULL' in _cabi.last_error()
        assert X(v._h, foreign._s, None, 8, out) == E and 'not an open snapshot' in _cabi.last_error()
        assert X(v._h, s._s, None, -1, out) == E
        assert X(v._h, s._s, None, 9, out) == E and '8 slots' in _cabi.last_error()       # no list: above the capacity
        assert X(v._h, s._s, None, 0, out) == 0
    assert L.ngw_snapshot_agent_view(v._h, s._s, None, 8, 0, out, None, None) == E and L.ngw_snapshot_agent_view(v._h, s._s, None, 8, 128, out, None, None) == E
    v.sync()
    assert not buf.any()                                         # (nothing ran)
    many = dev_i32(np.arange(20) % 8)                            # with a list the count is not bound by the capacity
    assert s.action_masks(many).shape == (20, len(spec.actions_id))
    handle = s._s
    s.close()
    for call in (s.lidar_observation, s.agent_view, s.action_masks):
        with pytest.raises(ValueError, match='closed'):
            call()
    assert L.ngw_snapshot_action_mask(v._h, handle, None, 1, out) == E
    assert v.error_flags() == 0
    v.close(); w.close()
    huge = VecNovelGridworld(spec=make_spec(T.POGO, 64), num_envs=n, seed=4)      # maps that do not fit LDS: masks and views do not stage them
    huge.reset()
    hs = huge.snapshot(n)
    hs.save()
    rows = hs.state()
    SO.assert_masks(hs.action_masks(), huge.spec, rows, np.arange(n), 'S=64')
    SO.assert_view(hs.agent_view(), rows, np.arange(n), 5, 'S=64')
    huge.close()
