"""The weighted choice among valid actions on the MI355X (csrc/ngw_sample.inc, include/ngw.h ngw_sample_actions, env.sample_actions,
Snapshot.sample_actions, env.step_sampled) and weighted playouts (ngw_snapshot_playout_weighted), held to the CPU oracle
(tests/sample_oracle.py: the oracle's masks, the oracle library's Philox, the oracle's steps, the selection written out in Python - never the
device's own mask or step, never sample.choose_weighted).  Every comparison is exact: action, the bits of the mass, the mask word."""
import ctypes as C

import numpy as np
import pytest

import mask_oracle as M
import ngw_testlib as T
import playout_oracle as PO
import sample_oracle as SO
import slot_rollout_oracle as RO
from gym_novel_gridworlds_amd import LimitActions, VecNovelGridworld, _cabi, limit_actions_vec
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, F_BAD_WEIGHT, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
STATE_KEYS = SO.STATE_KEYS
SEED = 0x5EED0123456789AB                                       # both halves non-zero
COUNTS = (1, 63, 64, 65, 130)                                   # a wave partly filled, exactly filled, just over, two and a bit


def make(cfg, n=20, auto=False, warm=30, limited=None):
    """A device env and its oracle twin `warm` random VALID steps after reset (autoreset with a horizon of 50 where `auto`), so that
    inventories and masks vary."""
    spec = T.build_spec(cfg)
    seed = SO.XO.good_seed(spec, n)
    kw = dict(autoreset=True, horizon=50) if auto else {}
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
    if limited:
        v, old = limit_actions_vec(v, limited), v
        old.close()
        spec = v.spec
    o = Oracle(spec.compile(), n, seed=seed, **kw)
    v.reset(); o.reset()
    rs = np.random.RandomState(n + warm)
    A = len(spec.actions_id)
    for _ in range(warm):
        words = M.oracle_mask_words(spec, o.st)
        a = np.array([rs.choice([i for i in range(A) if (int(w) >> i) & 1] or [0]) for w in words], np.int32)
        v.step(a); o.step(a)
    return spec, v, o


def host(s):
    """A Sampled of device tensors as numpy arrays (the words as uint64)."""
    return s.action.cpu().numpy(), s.mass.cpu().numpy(), s.mask_words.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize('cfg,auto', [('pogo10', False), ('pogo10', True), ('pogo13', False), ('pogo13', True), ('axe10', False), ('axe10', True),
                                      ('fire10h', False), ('fire10h', True)])
def test_configurations_and_counts(cfg, auto):
    """Every count, from the envs (host arrays) and from slots (device tensors used in place, the slot list repeating and permuted); weights
    over 2^-70 .. 2^70 with zeros, bad values in every other call: the flag is raised exactly then."""
    import torch
    spec, v, o = make(cfg, auto=auto)
    n, A = v.num_envs, len(spec.actions_id)
    pool = v.snapshot(n)
    pool.save(slots=np.random.RandomState(1).permutation(n))    # (slot != env)
    rows = pool.state()
    rs = np.random.RandomState(7)
    assert v.error_flags() == 0
    masks_seen = set()
    for i, count in enumerate(COUNTS):
        where = '%s auto=%d count=%d' % (cfg, auto, count)
        bad = bool(i & 1)
        envs = rs.randint(0, n, count)
        x = SO.random_weights(rs, count, A, bad)
        exp = SO.oracle_sample(spec, o.st, envs, x, SEED, 0, i)
        SO.assert_sampled(v.sample_actions(x, SEED, t=i, envs=envs), exp, where + ' from the envs')
        assert v.error_flags() == exp[3] == (F_BAD_WEIGHT if bad else 0), where
        masks_seen |= set(exp[2].tolist())
        slots = np.concatenate([rs.permutation(n), rs.randint(0, n, count)])[:count] if count > 1 else np.array([n - 1])
        x = SO.random_weights(rs, count, A, not bad)
        exp = SO.oracle_sample(spec, rows, slots, x, SEED, 1000, i)
        dev = torch.from_numpy(slots.astype(np.int32)).cuda()
        wdev = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
        torch.cuda.synchronize()
        got = pool.sample_actions(dev, wdev, SEED, first_pair=1000, t=i, device=True)
        assert got.action.dtype == torch.int32 and got.mass.dtype == torch.float32 and got.mask_words.dtype == torch.int64
        SO.assert_sampled(host(got), exp, where + ' from slots, on the device')
        assert v.error_flags() == exp[3] == (0 if bad else F_BAD_WEIGHT), where
        SO.assert_sampled(pool.sample_actions(slots, x, SEED, first_pair=1000, t=i), exp, where + ' from slots, host arrays')
        v.error_flags()
    assert len(masks_seen) > 3, "the states' masks do not vary"
    # every env, no list; all-zero weights: the uniform rule, mass 0
    exp = SO.oracle_sample(spec, o.st, np.arange(n), np.zeros((n, A), np.float32), SEED, 0, 2)
    got = v.sample_actions(np.zeros((n, A), np.float32), SEED, t=2)
    SO.assert_sampled(got, exp, 'all-zero weights')
    assert (got.mass == 0).all() and v.error_flags() == 0
    v.close()


def test_a_large_map_where_playouts_are_refused():
    """48x48 maps are past the rollout kernels' LDS limit: playout() is refused there, sampling reads the map in place and equals the oracle."""
    spec = make_spec(T.POGO, 48)
    n = 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset()
    rs = np.random.RandomState(3)
    A = len(spec.actions_id)
    for _ in range(12):
        v.step(rs.randint(0, A, n).astype(np.int32))
    pool = v.snapshot(n)
    pool.save()
    with pytest.raises(ValueError, match='64 maps in LDS'):
        pool.playout(np.arange(n), 3, SEED, weights=np.ones(A, np.float32))
    rows = v.get_state()
    x = SO.random_weights(rs, n, A)
    SO.assert_sampled(v.sample_actions(x, SEED, t=1), SO.oracle_sample(spec, rows, np.arange(n), x, SEED, 0, 1), '48x48 from the envs')
    slots = rs.randint(0, n, 130)
    x = SO.random_weights(rs, 130, A)
    SO.assert_sampled(pool.sample_actions(slots, x, SEED), SO.oracle_sample(spec, rows, slots, x, SEED), '48x48 from slots')
    assert v.error_flags() == 0
    v.close()


def test_the_draw_depends_on_seed_pair_and_t_alone():
    """The same slot 64 times: identical masks, differing actions; a call split in two with first_pair set equals the whole call; t = 0, 3, 4,
    7 pick the documented word and block (the oracle's Philox); another seed gives another draw."""
    spec, v, o = make('pogo10')
    n, A = v.num_envs, len(spec.actions_id)
    pool = v.snapshot(n)
    pool.save()
    rows = pool.state()
    x = np.tile(np.arange(1, A + 1, dtype=np.float32), (64, 1))
    same = pool.sample_actions(np.full(64, 3), x, SEED)
    SO.assert_sampled(same, SO.oracle_sample(spec, rows, np.full(64, 3), x, SEED), 'one slot, 64 pairs')
    assert len(set(same.mask_words.tolist())) == 1 and len(set(same.mass.tolist())) == 1 and len(set(same.action.tolist())) > 1
    rs = np.random.RandomState(2)
    slots, xs = rs.randint(0, n, 100), SO.random_weights(rs, 100, A)
    drawn = {}
    for t in (0, 3, 4, 7):
        whole = pool.sample_actions(slots, xs, SEED, t=t)
        SO.assert_sampled(whole, SO.oracle_sample(spec, rows, slots, xs, SEED, 0, t), 't = %d' % t)
        part = pool.sample_actions(slots[37:], xs[37:], SEED, first_pair=37, t=t)
        for k in range(3):
            assert (part[k] == whole[k][37:]).all(), (t, k)
        drawn[t] = whole.action
    assert len({tuple(a.tolist()) for a in drawn.values()}) == 4
    other = pool.sample_actions(slots, xs, SEED ^ (1 << 40))
    assert (other.action != drawn[0]).any() and (other.mass.view(np.uint32) == pool.sample_actions(slots, xs, SEED).mass.view(np.uint32)).all()
    assert v.error_flags() == 0
    v.close()


def test_two_ranks_on_one_device_equal_one_unsharded_env():
    from gym_novel_gridworlds_amd.dist import shard_range
    spec, v, o = make('pogo10', n=70, auto=True, warm=6)
    n, A = v.num_envs, len(spec.actions_id)
    x = SO.random_weights(np.random.RandomState(5), n, A)
    whole = v.sample_actions(x, SEED, t=5)
    SO.assert_sampled(whole, SO.oracle_sample(spec, o.st, np.arange(n), x, SEED, 0, 5), 'unsharded')
    for rank in range(2):
        first, m = shard_range(n, 2, rank)
        shard = VecNovelGridworld(spec=spec, num_envs=m, seed=v.seed, autoreset=True, horizon=50, env_index_base=first)
        shard.reset()
        shard.set_state(0, **{k: getattr(o.st, k)[first:first + m] for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count')})
        got = shard.sample_actions(x[first:first + m], SEED, t=5)
        for k in range(3):
            assert (got[k] == whole[k][first:first + m]).all(), (rank, k)
        shard.close()
    v.close()


def test_a_bad_index_from_the_device_gives_minus_one_and_leaves_its_neighbours_alone():
    import torch
    spec, v, o = make('axe10')
    n, A, count = v.num_envs, len(spec.actions_id), 66
    pool = v.snapshot(n)
    pool.save()
    rows = pool.state()
    rs = np.random.RandomState(8)
    slots, x = rs.randint(0, n, count), SO.random_weights(rs, count, A)
    slots[5], slots[65] = n, -3                                 # one past the last slot; a negative slot
    dev = torch.from_numpy(slots.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    assert v.error_flags() == 0
    got = host(pool.sample_actions(dev, x, SEED, device=True))
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    good = np.ones(count, bool)
    good[[5, 65]] = False
    exp = SO.oracle_sample(spec, rows, np.where(good, slots, 0), x, SEED)
    SO.assert_sampled([g[good] for g in got], [e[good] for e in exp[:3]], 'the other pairs')
    assert (got[0][~good] == -1).all() and (got[1][~good] == 0).all() and (got[2][~good] == 0).all()
    envs = torch.tensor([0, n + 4, 1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    got = host(v.sample_actions(x[:3], SEED, envs=envs, device=True))
    assert got[0][1] == -1 and got[0][0] >= 0 and got[0][2] >= 0 and v.error_flags() == F_BAD_INDEX
    v.close()


@pytest.mark.parametrize('auto', [False, True])
def test_nothing_is_committed(auto):
    """Env states, the last step's outputs, the mask words, the lookahead table, the lidar rows, every slot and the prepared episodes are what
    they were: the next real steps equal the oracle's."""
    import test_slot_rollout as TSR
    spec, v, o = make('fire10h', n=130, auto=auto, warm=8)
    n, A = v.num_envs, len(spec.actions_id)
    v.lidar_configure()
    pool = v.snapshot(n)
    pool.save()
    before, lidar0, pool0, cadence = TSR._everything(v), np.array(v.lidar_observation(copy=True)), pool.state(), v.refill_cadence
    rs = np.random.RandomState(3)
    x = SO.random_weights(rs, n, A)
    v.sample_actions(x, SEED)
    v.sample_actions(x[:7], SEED, envs=[3] * 7, device=True)
    pool.sample_actions(None, x, SEED, t=9)
    pool.playout(np.arange(n), 5, SEED, weights=x[0])
    v.playouts(2, 5, SEED, weights=x[1])
    v.sync()
    after = TSR._everything(v)
    for k in before:
        assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), k
    assert v.refill_cadence == cadence and (np.array(v.lidar_observation(copy=True)) == lidar0).all()
    pool1 = pool.state()
    for k in STATE_KEYS:
        assert (pool1[k] == pool0[k]).all(), k
    for t in range(12 if auto else 3):                          # no prepared episode was consumed: the resets are the oracle's
        a = rs.randint(0, A, n).astype(np.int32)
        assert not o.step(a) & 2
        _, reward, done, _ = v.step(a, copy=True)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
    s = v.get_state()
    for k in STATE_KEYS:
        assert (s[k].reshape(getattr(o.st, k).shape) == getattr(o.st, k)).all(), k
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('auto', [False, True])
def test_step_sampled_steps_with_the_sampled_actions(auto):
    """The returned actions equal sample_actions on the pre-step state (and the oracle's); the env afterwards equals the oracle stepped with
    them - over several steps, device weights used in place."""
    import torch
    spec, v, o = make('pogo10', n=130, auto=auto, warm=5)
    n, A = v.num_envs, len(spec.actions_id)
    rs = np.random.RandomState(6)
    for t in range(4):
        x = SO.random_weights(rs, n, A)
        exp = SO.oracle_sample(spec, o.st, np.arange(n), x, SEED, 0, t)
        pre = v.sample_actions(x, SEED, t=t)
        wdev = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
        got = v.step_sampled(wdev if t & 1 else x, SEED, t=t)
        assert all(isinstance(g, torch.Tensor) for g in got)
        got = host(got)
        SO.assert_sampled(got, exp, 'step %d' % t)
        SO.assert_sampled(pre, exp, 'step %d, sample_actions before it' % t)
        assert not o.step(exp[0]) & 2
        reward, done, _ = v.get_step_out(copy=True)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
        s = v.get_state()
        for k in STATE_KEYS:
            assert (s[k].reshape(getattr(o.st, k).shape) == getattr(o.st, k)).all(), (t, k)
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('cfg', ['pogo10', 'fire10h'])
def test_weighted_playouts(cfg):
    """T in {1, 9}, counts 65 and 130: reports, recorded actions and kept children equal the oracle's weighted playout; weights=None equals
    today's oracle_playout; device weights are used in place; a bad weight raises the flag."""
    import torch
    spec, v, o = make(cfg, auto=(cfg == 'fire10h'), warm=10)
    n, A, cap = v.num_envs, len(spec.actions_id), 300
    pool = v.snapshot(cap)
    pool.save(slots=np.arange(n))
    rows = pool.state()
    rs = np.random.RandomState(4)
    heavy = np.ones(A, np.float32)
    for name, a in spec.actions_id.items():
        if name in ('Forward', 'Break') or name.startswith('Craft'):
            heavy[a] = 8
    differs = False
    for count, steps in ((65, 1), (130, 9), (65, 9), (130, 1)):
        where = '%s count=%d T=%d' % (cfg, count, steps)
        parents = rs.randint(0, n, count)
        kids = n + rs.permutation(cap - n)[:count]
        w = heavy if steps == 9 else SO.random_weights(rs, 1, A)[0]
        ends, rep, acts, _ = SO.oracle_weighted_playout(spec, rows, parents, steps, SEED, w, 3, v.autoreset, v.horizon)
        wdev = torch.from_numpy(w).cuda()
        torch.cuda.synchronize()
        p = pool.playout(parents, steps, SEED, kids, first_pair=3, record=True, weights=wdev if count == 65 else w)
        PO.assert_playout(p, rep, acts, where + ' weighted')
        RO.assert_rows(pool.state(), ends, where + ' weighted', idx=kids)
        _, rep0, acts0, _ = PO.oracle_playout(spec, rows, parents, steps, SEED, 3, v.autoreset, v.horizon)
        PO.assert_playout(pool.playout(parents, steps, SEED, first_pair=3, record=True), rep0, acts0, where + ' weights=None')
        differs |= bool((acts0 != acts).any())
    assert differs and v.error_flags() == 0
    both = v.playouts(2, 9, SEED, weights=heavy)
    _, rep, _, _ = SO.oracle_weighted_playout(spec, o.st, np.repeat(np.arange(n), 2), 9, SEED, heavy, 0, v.autoreset, v.horizon)
    for k in PO.REPORTS:
        assert (both[k].reshape(-1) == rep[k]).all(), k
    w = heavy.copy()
    w[1] = -2
    pool.playout(np.arange(3), 1, SEED, weights=w)
    assert v.error_flags() == F_BAD_WEIGHT
    with pytest.raises(ValueError, match='shape'):
        pool.playout(np.arange(3), 1, SEED, weights=np.ones(A + 1, np.float32))
    v.close()


def test_limit_actions_draws_among_its_own_ids():
    """A batched env whose table is a limited list (limit_actions_vec): sampling and weighted playouts over its own ids; the adapter under
    LimitActions: weights over the limited ids, a limited id back."""
    names = ('Break', 'Forward', 'Left')
    spec, v, o = make('pogo10', limited=names, warm=6)
    n, A = v.num_envs, len(spec.actions_id)
    assert A == 3
    rs = np.random.RandomState(1)
    x = SO.random_weights(rs, n, A)
    SO.assert_sampled(v.sample_actions(x, SEED), SO.oracle_sample(spec, o.st, np.arange(n), x, SEED), 'limited table')
    w = np.array([1, 4, 2], np.float32)
    play = v.playouts(3, 5, SEED, weights=w)
    _, rep, _, _ = SO.oracle_weighted_playout(spec, o.st, np.repeat(np.arange(n), 3), 5, SEED, w)
    for k in PO.REPORTS:
        assert (play[k].reshape(-1) == rep[k]).all(), k
    v.close()
    env = T.make_adapter_env('axe10')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    vec = env.unwrapped._backend()
    rows = vec.get_state()
    full = SO.random_weights(rs, 1, vec.n_actions)[0]
    got = env.sample_action(full, SEED, t=2)
    exp = SO.oracle_sample(vec.spec, rows, [0], full[None], SEED, 0, 2)
    assert got == (int(exp[0][0]), float(exp[1][0]), int(exp[2][0]))
    lim = LimitActions(env, set(names))
    got = lim.sample_action(w, SEED, t=2)
    limited_spec = lim.__dict__['_playout_env'][2].spec
    exp = SO.oracle_sample(limited_spec, rows, [0], w[None], SEED, 0, 2)
    assert got == (int(exp[0][0]), float(exp[1][0]), int(exp[2][0])) and 0 <= got[0] < 3
    play = lim.playouts(66, 5, SEED, weights=w)
    _, rep, _, _ = SO.oracle_weighted_playout(limited_spec, rows, np.zeros(66, np.int64), 5, SEED, w)
    for k in PO.REPORTS:
        assert (play[k] == rep[k]).all(), k
    lim.close()


def test_cabi_error_returns():
    import torch
    L = _cabi.lib()
    spec = T.build_spec('pogo10')
    n = 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    w = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset(); w.reset()
    A = len(spec.actions_id)
    s, foreign = v.snapshot(8), w.snapshot(8)
    wt = torch.ones(A * 128, dtype=torch.float32, device='cuda')
    act = torch.full((128,), -7, dtype=torch.int32, device='cuda')
    idx = torch.zeros(128, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    x, a, i, E, X, err = C.c_void_p(wt.data_ptr()), C.c_void_p(act.data_ptr()), C.c_void_p(idx.data_ptr()), _cabi.E_INVALID_ARG, L.ngw_sample_actions, _cabi.last_error
    N = None
    assert X(N, N, N, 1, x, 1, 1, 0, 0, a, N, N) == E and 'NULL' in err()
    assert X(v._h, N, N, 1, N, 1, 1, 0, 0, a, N, N) == E and 'NULL' in err()
    assert X(v._h, N, N, 1, x, 1, 1, 0, 0, N, N, N) == E and 'NULL' in err()
    assert X(v._h, N, N, -1, x, 1, 1, 0, 0, a, N, N) == E
    assert X(v._h, N, N, 8, x, 7, 1, 0, 0, a, N, N) == E and 'weight stride of 7' in err()
    assert X(v._h, foreign._s, N, 8, x, 8, 1, 0, 0, a, N, N) == E and 'not an open snapshot' in err()
    assert X(v._h, N, N, 71, x, 71, 1, 0, 0, a, N, N) == E and '70 envs' in err()
    assert X(v._h, s._s, N, 9, x, 9, 1, 0, 0, a, N, N) == E and '8 slots' in err()
    v.sync()
    assert (act.cpu().numpy() == -7).all()                       # nothing ran
    assert X(v._h, N, N, 0, x, 0, 1, 0, 0, a, N, N) == 0          # count == 0: a no-op
    assert X(v._h, N, i, 128, x, 128, 1, 0, 0, a, N, N) == 0      # a list: count above n_envs; mass and masks may be NULL
    v.sync()
    assert (act.cpu().numpy() >= 0).all() and v.error_flags() == 0
    v.close(); w.close()
