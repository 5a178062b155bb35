"""State keys on the MI355X (csrc/ngw_keys.inc, include/ngw.h ngw_state_keys, Snapshot.keys / unique, VecNovelGridworld.state_keys, the
adapter's state_key), held to the plain-integer oracle (tests/state_key_oracle.py) applied to a host copy of the rows - pool.state() /
get_state() - never to the device's own answer."""
import ctypes as C

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import state_key_oracle as KO
import gym_novel_gridworlds_amd as G
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.lidar import LidarConfig
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_ALL = sorted(T.CFGS)
EVERY_FIELDS = KO.SINGLE + (KO.STATE, KO.ALL)


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
    of children; 200 random slots with repeats under KEY_STATE and KEY_ALL; the envs' own keys; a saved slot's key is its env's."""
    spec = T.build_spec(cfg)
    n, A = 130, len(spec.actions_id)
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=25)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=25)
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
        rows, envs = KO.Table(pool.state()), KO.Table(v.get_state())
        slots = rs.randint(0, 2 * n, 200)
        for fields in (G.KEY_STATE, G.KEY_ALL):
            KO.assert_keys(pool.keys(slots, fields), rows, slots, fields, where + ' slots')
            of_envs = v.state_keys(fields=fields)
            KO.assert_keys(of_envs, envs, np.arange(n), fields, where + ' envs')
            assert (pool.keys(np.arange(n), fields) == of_envs).all(), where + ': a saved slot and its env have different keys'
    assert (v.state_keys() == v.state_keys(fields=G.KEY_STATE)).all()      # (the default selection)
    assert v.error_flags() == 0
    v.close()


def fill_without_expand(v, pool, n, cap, rs, A):
    """Every slot a state of its own where expand is refused: the envs are stepped and saved round after round, and now and then put back
    into states saved earlier (a restore with repeated slots: the fork) so that the pool is not one trajectory per env."""
    for first in range(0, cap, n):
        for t in range(3):
            v.step(rs.randint(0, A, n).astype(np.int32))
        m = min(n, cap - first)
        pool.save(envs=np.arange(m), slots=first + np.arange(m))
        if first and first % (4 * n) == 0:
            pool.restore(slots=rs.randint(0, first, n), envs=np.arange(n))


@pytest.mark.parametrize('S', [9, 10, 12, 32, 48])
@pytest.mark.parametrize('count', [1, 63, 65, 200])
def test_map_sizes_and_counts(S, count):
    """One map size per form of the row reads - odd S*S with unaligned dwords, a byte tail and a last group of one cell: 9; dwords: 10;
    16-byte pieces, fewer pieces than group lanes: 12; several pieces per lane: 32; maps beyond the LDS limit, where expand is refused: 48 -
    and counts around the wavefront width and far above num_envs = 5.  Host lists, device tensors with the keys left on the device, and
    slots=None on a small snapshot, under every single field, KEY_STATE and KEY_ALL."""
    import torch
    spec = make_spec(T.POGO, S)
    n, A, cap = 5, len(spec.actions_id), 256
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=30)
    v.reset()
    rs = np.random.RandomState(S + count)
    for t in range(25):
        v.step(rs.randint(0, A, n).astype(np.int32))
    pool, small = v.snapshot(cap), v.snapshot(7)
    if S == 48:
        with pytest.raises(ValueError, match='64 maps in LDS'):
            pool.expand(rs.randint(0, n, cap), rs.randint(0, A, cap), np.arange(cap), from_envs=True)
        fill_without_expand(v, pool, n, cap, rs, A)
        small.save(envs=np.arange(n), slots=np.arange(n))        # (slots 5 and 6 stay never-saved slots)
    else:
        pool.expand(rs.randint(0, n, cap), rs.randint(0, A, cap), np.arange(cap), from_envs=True)      # every slot a state of its own
        small.expand(rs.randint(0, n, 7), rs.randint(0, A, 7), None, from_envs=True)
    rows, srows = KO.Table(pool.state()), KO.Table(small.state())
    where = 'S=%d count=%d' % (S, count)
    host, on_dev = rs.randint(0, cap, count), rs.randint(0, cap, count)
    d = dev_i32(on_dev)
    for fields in EVERY_FIELDS:
        got = pool.keys(host, fields)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint64 and got.shape == (count,)
        KO.assert_keys(got, rows, host, fields, where + ' host list')
        got = pool.keys(d, fields, device=True)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and tuple(got.shape) == (count,) and got.is_cuda
        KO.assert_keys(got, rows, on_dev, fields, where + ' device tensor')
        KO.assert_keys(small.keys(fields=fields), srows, np.arange(7), fields, where + ' every slot')
    KO.assert_keys(v.state_keys(), KO.Table(v.get_state()), np.arange(n), G.KEY_STATE, where + ' envs')
    assert v.error_flags() == 0
    v.close()


def test_permuted_and_unaligned_rows():
    """S = 9: the rows of slots 1, 2 and 3 start at byte offsets 81, 162 and 243 - with slot 0 all four alignments.  The keys equal those of
    the same states held in slot 0 of a second snapshot (and the oracle's): a key is defined on cell indices, never on addresses."""
    spec = make_spec(T.POGO, 9)
    n, A = 4, len(spec.actions_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n))
    v.reset()
    rs = np.random.RandomState(9)
    for t in range(15):
        v.step(rs.randint(0, A, n).astype(np.int32))
    many, one = v.snapshot(4), v.snapshot(1)
    many.save(envs=[2, 0, 3, 1], slots=[0, 1, 2, 3])             # permuted: slot k does not hold env k
    rows = KO.Table(many.state())
    for k, env in enumerate([2, 0, 3, 1]):
        one.save(envs=[env], slots=[0])
        for fields in EVERY_FIELDS:
            a, b = many.keys([k], fields), one.keys([0], fields)
            assert a[0] == b[0], (k, fields)
            KO.assert_keys(a, rows, [k], fields, 'slot %d' % k)
    order = [3, 1, 2, 0, 2, 3]
    KO.assert_keys(many.keys(order, G.KEY_ALL), rows, order, G.KEY_ALL, 'one call, every alignment')
    assert v.error_flags() == 0
    v.close()


def test_bad_indices_give_zero_keys_and_raise_the_flag():
    """A device list with -1, `capacity` and 2^31 - 1 among good indices, one in each wave: their keys are 0, the others correct,
    F_BAD_INDEX is reported once, and exactly `count` outputs are written - the guard words before and after them are intact.  The same
    through the env rows (s == NULL)."""
    import torch
    spec = T.build_spec('axe10')
    n, A, cap = 70, len(spec.actions_id), 140
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n))
    v.reset()
    rs = np.random.RandomState(8)
    pool = v.snapshot(cap)
    grow(v, pool, n, rs, A)
    rows, envs = KO.Table(pool.state()), KO.Table(v.get_state())
    count, guard = 130, 0x5A5A5A5A5A5A5A5A
    bad_at = [5, 65, 129]
    good = np.ones(count, bool)
    good[bad_at] = False
    for snap, limit, table in ((pool, cap, rows), (None, n, envs)):
        idx = rs.randint(0, limit, count)
        idx[bad_at] = [-1, limit, 2 ** 31 - 1]
        d = dev_i32(idx)
        buf = torch.full((count + 16,), guard, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        assert v.error_flags() == 0
        _cabi.check(_cabi.lib().ngw_state_keys(v._h, snap._s if snap else None, C.c_void_p(d.data_ptr()), count, G.KEY_ALL,
                                               C.c_void_p(buf.data_ptr() + 8 * 8)))
        v.sync()
        assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
        out = buf.cpu().numpy()
        assert (out[:8] == guard).all() and (out[8 + count:] == guard).all(), "stores outside the count outputs"
        got = out[8:8 + count].view(np.uint64)
        assert (got[~good] == 0).all()
        KO.assert_keys(got[good], table, idx[good], G.KEY_ALL, 'keys beside bad indices')
    got = pool.keys(dev_i32([3, cap, 4]))                        # the Python call: the same clamp
    assert got[1] == 0 and v.error_flags() == F_BAD_INDEX
    KO.assert_keys(got[[0, 2]], rows, [3, 4], G.KEY_STATE, 'python call')
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
    """Fused lidar, masks-in-step, terminal capture, autoreset under a horizon, a graph captured beforehand; after a step and a lookahead
    (masks and table current) keys() and state_keys() leave every recorded byte as it was: the state, the last step's outputs, the env's lidar
    rows, masks, lookahead table and both snapshots.  The derived buffers stay CURRENT: poisoned through their zero-copy views, they read
    back poisoned (a following lookahead() launches nothing).  The graph then replays to the oracle's result."""
    import torch
    spec = T.build_spec('fire10h')
    n, A, H = 130, len(spec.actions_id), 12
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.lidar_configure(LidarConfig(spec, 8), fused=True, dtype=np.int32)
    v.set_action_masks(True)
    v.set_terminal_capture(True)
    v.reset(); o.reset()
    rs = np.random.RandomState(23)

    def step():
        a = rs.randint(0, A, n).astype(np.int32)
        assert not o.step(a) & 2
        v.step(a)
    pool, other = v.snapshot(2 * n), v.snapshot(n)
    for t in range(9):
        step()
    grow(v, pool, n, rs, A)
    other.save()
    acts = rs.randint(0, A, (6, n)).astype(np.int32)
    ad = torch.from_numpy(acts).cuda()
    torch.cuda.synchronize()
    v.graph_build(ad.data_ptr(), n, 6)                           # captured before the key calls, replayed after them
    step()
    v.lookahead()
    before = _everything(v, (pool, other))
    rows, envs = KO.Table(pool.state()), KO.Table(v.get_state())

    def key_calls(where):
        slots = rs.randint(0, 2 * n, 150)
        for fields in (G.KEY_STATE, G.KEY_ALL, G.KEY_POSE | G.KEY_INV):
            KO.assert_keys(pool.keys(slots, fields), rows, slots, fields, where)
            KO.assert_keys(pool.keys(dev_i32(slots), fields, device=True), rows, slots, fields, where + ' device')
            KO.assert_keys(v.state_keys(fields=fields), envs, np.arange(n), fields, where + ' envs')
        which = rs.randint(0, n, 77)
        KO.assert_keys(v.state_keys(dev_i32(which), G.KEY_ALL, device=True), envs, which, G.KEY_ALL, where + ' envs, device list')
        other.keys(), other.unique(device=True)
    key_calls('first round')
    after = _everything(v, (pool, other))
    assert sorted(before) == sorted(after)
    for k in before:
        assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), k
    v.lookahead(device=True)['reward'].fill_(-77)                # both derived buffers poisoned through their zero-copy views
    v.action_mask_words(device=True).fill_(-1)
    torch.cuda.synchronize()
    key_calls('second round')
    assert (v.lookahead(copy=True)['reward'] == -77).all(), "a key call made the lookahead table stale"
    assert (v.action_mask_words(copy=True) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "a key call made the action masks stale"
    v.graph_launch(1)
    for t in range(6):
        assert not o.step(acts[t]) & 2
    s = v.get_state()
    for k, ref in zip(XO.STATE_KEYS, (o.st.map, o.st.loc, o.st.facing, o.st.inv, o.st.selected, o.st.step_count, o.st.episode)):
        assert (s[k].reshape(ref.shape) == ref).all(), "graph replay behind the key calls: " + k
    KO.assert_keys(v.state_keys(fields=G.KEY_ALL), s, np.arange(n), G.KEY_ALL, 'after the graph replay')
    assert v.error_flags() == 0
    v.close()


def test_transpositions_have_one_key():
    """From one saved state, Left then Right and Right then Left (two chains of expands): the two grandchildren - and the parent they turn
    back into - share their KEY_STATE key, while under KEY_ALL without the episode counter the grandchildren differ from the parent (two
    steps later) and agree with each other; the states in between differ under both.  unique() groups parents and children as the oracle's
    keys do, on the host and on the device."""
    spec = T.build_spec('pogo10')
    n = 3
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n))
    v.reset()
    left, right = spec.actions_id['Left'], spec.actions_id['Right']
    pool = v.snapshot(5 * n)
    pool.save(slots=np.arange(n))
    base = np.arange(n)
    for parents, action, children in ((base, left, n + base), (n + base, right, 2 * n + base), (base, right, 3 * n + base), (3 * n + base, left, 4 * n + base)):
        pool.expand(parents, np.full(n, action), children)
    rows = KO.Table(pool.state())
    every = np.arange(5 * n)
    timed = G.KEY_ALL & ~G.KEY_EPISODE
    k15, k31 = pool.keys(), pool.keys(fields=timed)
    KO.assert_keys(k15, rows, every, G.KEY_STATE, 'KEY_STATE')
    KO.assert_keys(k31, rows, every, timed, 'KEY_ALL without the episode')
    for e in range(n):
        p, l, lr, r, rl = (e + i * n for i in range(5))
        assert k15[lr] == k15[rl] == k15[p] and k31[lr] == k31[rl] and k31[lr] != k31[p], e
        assert len({int(k15[p]), int(k15[l]), int(k15[r])}) == 3 and len({int(k31[x]) for x in (p, l, lr, r)}) == 4, e
    slots = np.random.RandomState(6).randint(0, 5 * n, 40)
    for fields in (G.KEY_STATE, timed):
        exp = KO.keys_of(rows, slots, fields)
        smallest = np.array([min(i for i in range(40) if exp[i] == exp[j]) for j in range(40)])
        for dev in (False, True):
            first, inverse = pool.unique(slots, fields, device=dev)
            if dev:
                assert first.is_cuda and inverse.is_cuda
                first, inverse = first.cpu().numpy(), inverse.cpu().numpy()
            assert first.shape == (len(set(exp.tolist())),) and inverse.shape == (40,)
            assert (first[inverse] == smallest).all(), (fields, dev)
    assert v.error_flags() == 0
    v.close()


def _adapter_rows(env):
    base = env
    while hasattr(base, 'env') and not hasattr(base, '_backend'):
        base = base.env
    return base._backend().get_state()


def test_single_env_adapter_wrappers_and_limit_actions():
    """state_key() of the single-env adapter, bare (its resident step loop is ended before the env row is read from HBM, and steps go on
    afterwards), under a novelty wrapper stack and under LimitActions, equals the oracle on the adapter's get_state and is a Python int."""
    limited = {'Forward', 'Left', 'Right', 'Break', 'Craft_plank', 'Craft_stick'}
    envs = [G.make('NovelGridworld-Pogostick-v1'), T.make_adapter_env('axe10'), T.make_adapter_env('fence10e'),
            G.LimitActions(G.make('NovelGridworld-Pogostick-v1'), limited), G.LimitActions(T.make_adapter_env('axe10'), limited)]
    rs = np.random.RandomState(3)
    for which, env in enumerate(envs):
        env.reset()
        for i in range(12):
            _, _, done, _ = env.step(int(rs.randint(0, env.action_space.n)))
            if done:
                env.reset()
            if i % 3 == 2:
                fields = (G.KEY_STATE, G.KEY_ALL, G.KEY_POSE | G.KEY_INV)[i // 3 % 3]
                key = env.state_key(fields)
                assert type(key) is int and key == KO.key_of_row(_adapter_rows(env), 0, fields), (which, i)
        assert env.state_key() == env.state_key(G.KEY_STATE) == KO.key_of_row(_adapter_rows(env), 0, KO.STATE), which
        with pytest.raises(ValueError, match='fields'):
            env.state_key(0)
        env.close()


def test_cabi_errors():
    """Each NGW_E_INVALID_ARG case of include/ngw.h returns the code and launches nothing (the output keeps its pattern); count == 0 is a
    no-op; with a list the count is not bound by the row count; a closed snapshot raises; S = 64 is served (nothing is staged in LDS)."""
    import torch
    L = _cabi.lib()
    spec = T.build_spec('pogo10')
    n = 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    w = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset(); w.reset()
    s, foreign = v.snapshot(8), w.snapshot(8)
    s.save(slots=np.arange(8), envs=np.arange(8))
    buf = torch.full((256,), 0x77, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    out, E, X = C.c_void_p(buf.data_ptr()), _cabi.E_INVALID_ARG, L.ngw_state_keys
    assert X(None, s._s, None, 8, 15, out) == E and 'NULL' in _cabi.last_error()
    assert X(v._h, s._s, None, 8, 15, None) == E and 'NULL' in _cabi.last_error()
    assert X(v._h, foreign._s, None, 8, 15, out) == E and 'not an open snapshot' in _cabi.last_error()
    assert X(v._h, s._s, None, -1, 15, out) == E and X(v._h, None, None, -1, 15, out) == E
    for fields in (0, 64, 128, 1 << 31, 63 | 256):
        assert X(v._h, s._s, None, 8, fields, out) == E and 'fields' in _cabi.last_error(), fields
    assert X(v._h, s._s, None, 9, 15, out) == E and '8 slots' in _cabi.last_error()       # no list: above the capacity
    assert X(v._h, None, None, 71, 15, out) == E and '70 envs' in _cabi.last_error()      # ... above n_envs
    assert X(v._h, s._s, None, 0, 15, out) == 0 and X(v._h, None, None, 0, 63, out) == 0
    closed = v.snapshot(4)
    handle = closed._s
    closed.close()
    assert X(v._h, handle, None, 1, 15, out) == E
    with pytest.raises(ValueError, match='closed'):
        closed.keys()
    with pytest.raises(ValueError, match='closed'):
        closed.unique()
    v.sync()
    assert (buf == 0x77).all()                                   # (nothing ran)
    for bad in (0, 64, -1, 1.5):
        with pytest.raises(ValueError, match='fields'):
            s.keys(fields=bad)
        with pytest.raises(ValueError, match='fields'):
            v.state_keys(fields=bad)
    with pytest.raises(ValueError):
        s.keys([8])
    with pytest.raises(ValueError):
        v.state_keys([n])
    rows = s.state()
    many = np.arange(20) % 8                                     # with a list the count is not bound by the row count
    KO.assert_keys(s.keys(dev_i32(many)), rows, many, G.KEY_STATE, 'twenty keys of eight slots')
    assert s.keys([]).shape == (0,) and v.state_keys([]).shape == (0,)
    assert v.error_flags() == 0
    v.close(); w.close()
    huge = VecNovelGridworld(spec=make_spec(T.POGO, 64), num_envs=n, seed=4)      # maps that do not fit LDS: nothing is staged there
    huge.reset()
    hs = huge.snapshot(n)
    hs.save()
    KO.assert_keys(hs.keys(fields=G.KEY_ALL), hs.state(), np.arange(n), G.KEY_ALL, 'S=64')
    KO.assert_keys(huge.state_keys(), huge.get_state(), np.arange(n), G.KEY_STATE, 'S=64 envs')
    huge.close()
