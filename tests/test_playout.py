"""Valid-action random playouts on the MI355X (csrc/ngw_playout.inc, include/ngw.h ngw_snapshot_playout, Snapshot.playout, env.playouts), held
to the CPU oracle (tests/playout_oracle.py: the oracle's masks, the oracle library's Philox, the oracle's steps - never the device's own
mask or step).  All results are integers and compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import playout_oracle as PO
import slot_rollout_oracle as RO
from gym_novel_gridworlds_amd import LimitActions, VecNovelGridworld, _cabi, limit_actions_vec
from gym_novel_gridworlds_amd.playout import choose_actions
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
STATE_KEYS = PO.STATE_KEYS
SEED = 0x5EED0123456789AB                                       # both halves non-zero
SHAPES = ((1, 1), (65, 5), (200, 9))                            # (pairs, T): a lone lane / one past a wave / a ragged last wave; no / one / two block changes
NO_TURN = ('Break', 'Forward')


def make(cfg, n=20, auto=False, limited=None, warm=10):
    """A device env and its oracle twin after `warm` random steps (autoreset with a horizon of 6 where `auto`)."""
    spec = T.build_spec(cfg)
    seed = XO.good_seed(spec, n)
    kw = dict(autoreset=True, horizon=6) if auto else {}
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
    if limited:
        v, old = limit_actions_vec(v, limited), v
        old.close()
        spec = v.spec
    o = Oracle(spec.compile(), n, seed=seed, **kw)
    v.reset(); o.reset()
    rs = np.random.RandomState(n + warm)
    for _ in range(warm):
        a = rs.randint(0, len(spec.actions_id), n).astype(np.int32)
        v.step(a); o.step(a)
    return spec, v, o


def host(p):
    """A Playout of device tensors as numpy arrays ('info' as the uint32 words)."""
    d = {k: p[k].cpu().numpy() for k in PO.REPORTS}
    d['info'] = d['info'].view(np.uint32)
    d['actions'] = None if p.actions is None else p.actions.cpu().numpy()
    return d


def playout_checked(v, spec, snap, rows, parents, steps, children, where, first_pair=0, **kw):
    """One recorded playout held to the oracle: `rows` is a host copy of the source's rows.  -> (Playout, ends, reports, actions, masks)."""
    ends, rep, acts, masks = PO.oracle_playout(spec, rows, parents, steps, SEED, first_pair, v.autoreset, v.horizon)
    p = snap.playout(parents, steps, SEED, children, first_pair=first_pair, record=True, **kw)
    PO.assert_playout(p, rep, acts, where)
    if children is not None:
        RO.assert_rows(snap.state(), ends, where, idx=np.asarray(children))
    return p, ends, rep, acts, masks


@pytest.mark.parametrize('cfg,auto', [('pogo10', False), ('pogo10', True), ('pogo13', False), ('axe10', False), ('fire10h', False), ('fire10h', True),
                                      ('add32', False)])
def test_configurations_counts_and_steps(cfg, auto):
    """Every (pairs, T) shape: parents = slots of the same pool with repeats, children kept (T = 5) or not; from the envs; from another
    pool.  Under autoreset with a horizon of 6 the horizon ends pairs inside T = 9; in fire10h deaths do."""
    spec, v, o = make(cfg, auto=auto)
    n, cap = v.num_envs, 512
    pool, other = v.snapshot(cap), v.snapshot(n)
    pool.save(slots=np.arange(n)); other.save()
    rows = pool.state()
    rs = np.random.RandomState(3)
    cut = died = False
    for count, steps in SHAPES:
        where = '%s auto=%d count=%d T=%d' % (cfg, auto, count, steps)
        parents = rs.randint(0, n, count)
        kids = n + rs.permutation(cap - n)[:count] if steps == 5 else None
        p, _, rep, acts, _ = playout_checked(v, spec, pool, rows, parents, steps, kids, where + ' same pool')
        assert ((acts >= 0).sum(0) == rep['length']).all()
        cut |= bool((rep['ended'] & (rep['length'] < steps) & (((rep['info'] >> 1) & 1) == 0)).any())
        died |= bool((rep['ended'] & (((rep['info'] >> 8) & 255) == 14)).any())
        playout_checked(v, spec, pool, o.st, parents, steps, None if kids is None else kids[::-1].copy(), where + ' from the envs', from_envs=True)
        playout_checked(v, spec, pool, other.state(), parents, steps, kids, where + ' from another pool', source=other)
    assert cut or not auto, "the horizon ended no pair inside T = 9"
    assert died or cfg != 'fire10h' or auto, "no FireWall death inside a playout"
    assert v.error_flags() == 0
    v.close()


def test_the_same_parent_64_times_gives_differing_playouts():
    spec, v, o = make('pogo10')
    pool = v.snapshot(v.num_envs)
    pool.save()
    p, _, rep, acts, _ = playout_checked(v, spec, pool, pool.state(), np.full(64, 3), 9, None, 'one parent, 64 pairs')
    assert len({tuple(acts[:, j]) for j in range(64)}) > 32 and len(set(rep['first_action'].tolist())) > 1
    v.close()


def test_no_turn_action_lists_meet_empty_and_full_masks():
    """LimitActions lists without a turn: with Break and Forward an agent facing the border has no valid action (every action is then a
    candidate, the step fails and the pair stays where it is); with Forward alone the mask is either empty or full.  The oracle says that
    both kinds were executed - otherwise the inputs are wrong - and the device agrees pair by pair."""
    empty = full = 0
    for names in (NO_TURN, ('Forward',)):
        spec, v, o = make('pogo10', limited=names, warm=0)          # (right after reset: warm-up steps without a turn would park every agent against a block)
        A = len(spec.actions_id)
        assert A == len(names)
        pool = v.snapshot(400)
        for count, steps in SHAPES:
            where = 'limited %s count=%d T=%d' % ('+'.join(names), count, steps)
            parents = np.random.RandomState(count).randint(0, v.num_envs, count)
            kids = np.arange(count) if steps == 9 else None
            _, _, _, acts, masks = playout_checked(v, spec, pool, o.st, parents, steps, kids, where, from_envs=True)
            ran = acts >= 0
            empty += int((masks[ran] == 0).sum())
            full += int((masks[ran] == np.uint64((1 << A) - 1)).sum())
            assert names != NO_TURN or steps < 9 or (masks[ran] == 0).any(), "Break + Forward met no empty mask"
        assert v.error_flags() == 0
        v.close()
    assert empty > 0 and full > 0, (empty, full)


def test_recorded_actions_replay_through_rollout_and_equal_the_host_contract():
    """record=True, device=True: rollout() on the recorded device tensor returns the same reports and bit-identical child rows (the -1 of a
    step that was not executed comes after the pair's end, where rollout ignores it); and the first actions are choose_actions() of the
    device's own mask words of the parents."""
    import torch
    spec, v, o = make('axe10', auto=True)
    n, count, steps = v.num_envs, 200, 9
    pool = v.snapshot(n + 2 * count)
    pool.save(slots=np.arange(n))
    parents = np.random.RandomState(1).randint(0, n, count)
    dev = torch.from_numpy(parents.astype(np.int32)).cuda()
    kids_a, kids_b = torch.arange(n, n + count, dtype=torch.int32).cuda(), torch.arange(n + count, n + 2 * count, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    play = pool.playout(dev, steps, SEED, kids_a, record=True, device=True)
    assert all(isinstance(x, torch.Tensor) for x in play) and tuple(play.actions.shape) == (steps, count) and play.actions.dtype == torch.int32
    assert play.ended.dtype == torch.bool and play.info.dtype == torch.int32 and play.first_action.dtype == torch.int32
    again = pool.rollout(dev, play.actions, kids_b, device=True)
    for k in ('ret', 'length', 'ended', 'info'):
        assert torch.equal(play[k], again[k]), k
    st = pool.state()
    for k in STATE_KEYS:
        assert st[k][n:n + count].tobytes() == st[k][n + count:].tobytes(), k
    got = host(play)
    ends, rep, acts, _ = PO.oracle_playout(spec, st, parents, steps, SEED, 0, True, 6)
    PO.assert_playout(got, rep, acts, 'device tensors')
    RO.assert_rows(st, ends, 'device tensors', idx=np.arange(n, n + count))
    assert (got['length'] < steps).any() and (got['actions'][-1] == -1).any()
    words = pool.action_masks(dev, device=True)
    packed = (words.cpu().numpy().astype(np.uint64) << np.arange(words.shape[1], dtype=np.uint64)).sum(1)
    assert (choose_actions(packed, SEED, np.arange(count), 0, len(spec.actions_id)) == got['first_action']).all()
    assert v.error_flags() == 0
    v.close()


def test_a_bad_index_from_the_device_skips_its_pair():
    """Index tensors on the device with one parent and one child out of range: those pairs get zero reports, -1 actions and no slot, the
    flag is raised, the other pairs are the oracle's."""
    import torch
    spec, v, o = make('axe10')
    n, count, steps, cap = v.num_envs, 66, 5, 90
    pool, dst = v.snapshot(n), v.snapshot(cap)
    pool.save()
    dst.save(slots=np.arange(n))
    rows, dst0 = pool.state(), dst.state()
    rs = np.random.RandomState(8)
    parents, children = rs.randint(0, n, count), rs.permutation(cap)[:count]
    parents[5], children[65] = n, -3                            # one past the last slot; a negative slot
    dev = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in (parents, children)]
    torch.cuda.synchronize()
    assert v.error_flags() == 0
    got = host(dst.playout(dev[0], steps, SEED, dev[1], source=pool, record=True, device=True))
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    good = np.ones(count, bool)
    good[[5, 65]] = False
    where = np.nonzero(good)[0]
    exp = [PO.oracle_playout(spec, rows, parents[j:j + 1], steps, SEED, int(j)) for j in where]    # (pair numbers are positions in the call)
    for k in PO.REPORTS:
        assert (got[k][good] == np.concatenate([e[1][k] for e in exp])).all(), k
    assert (got['actions'][:, good] == np.concatenate([e[2] for e in exp], 1)).all()
    for k in ('ret', 'length', 'ended', 'info'):
        assert (got[k][~good] == 0).all(), k
    assert (got['first_action'][~good] == -1).all() and (got['actions'][:, ~good] == -1).all()
    dst1 = dst.state()
    RO.assert_rows(dst1, {k: np.concatenate([e[0][k] for e in exp]) for k in STATE_KEYS}, 'the other pairs', idx=children[good])
    rest = np.setdiff1d(np.arange(cap), children[good])
    for k in STATE_KEYS:
        assert (dst1[k][rest] == dst0[k][rest]).all(), k
    v.close()


@pytest.mark.parametrize('auto', [False, True])
def test_nothing_is_committed(auto):
    """Env states, the last step's outputs, the mask words, the lookahead table, every slot but the children and the prepared episodes
    are what they were: the next real steps equal the oracle's."""
    import test_slot_rollout as TSR
    spec, v, o = make('fire10h', n=130, auto=auto)
    n, A, cap = v.num_envs, len(spec.actions_id), 400
    pool, other = v.snapshot(cap), v.snapshot(n)
    pool.save(slots=np.arange(n)); other.save()
    before, pool0, other0, cadence = TSR._everything(v), pool.state(), other.state(), v.refill_cadence
    kids = n + np.arange(200)
    pool.playout(np.arange(200) % n, 9, SEED, kids)
    pool.playout(np.arange(n), 9, SEED, from_envs=True)
    pool.playout(np.arange(n), 5, SEED, source=other)
    v.playouts(3, 9, SEED)
    after = TSR._everything(v)
    for k in before:
        assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), k
    assert v.refill_cadence == cadence
    untouched = np.setdiff1d(np.arange(cap), kids)
    pool1, other1 = pool.state(), other.state()
    for k in STATE_KEYS:
        assert (pool1[k][untouched] == pool0[k][untouched]).all() and (other1[k] == other0[k]).all(), k
    rs = np.random.RandomState(5)
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


def test_pair_numbering_first_pair_playouts_and_shards():
    """first_pair shifts the numbering; env.playouts(P) is playout(repeat(arange(N), P), from_envs=True) shaped [N, P]; two shards on one
    device (env_index_base = the shard's first env) return what the unsharded env returns."""
    from gym_novel_gridworlds_amd.dist import shard_range
    spec, v, o = make('pogo10', n=70, auto=True, warm=3)
    n, steps, P = v.num_envs, 9, 3
    pool = v.snapshot(n)
    pool.save()
    parents = np.random.RandomState(2).randint(0, n, 100)
    whole = pool.playout(parents, steps, SEED, record=True)
    part = pool.playout(parents[32:], steps, SEED, first_pair=32, record=True)
    for k in PO.REPORTS:
        assert (part[k] == whole[k][32:]).all(), k
    assert (part.actions == whole.actions[:, 32:]).all() and (whole.first_action == whole.actions[0]).all()
    flat = pool.playout(np.repeat(np.arange(n), P), steps, SEED, from_envs=True)
    ends, rep, acts, _ = PO.oracle_playout(spec, o.st, np.repeat(np.arange(n), P), steps, SEED, 0, True, 6)
    both = v.playouts(P, steps, SEED)
    assert both.actions is None and both.ret.shape == (n, P) and both.goal.shape == (n, P)
    for k in PO.REPORTS:
        assert (both[k].reshape(-1) == flat[k]).all() and (flat[k] == rep[k]).all(), k
    import torch
    on_dev = v.playouts(P, steps, SEED, device=True)
    assert isinstance(on_dev.ret, torch.Tensor) and (on_dev.first_action.cpu().numpy() == both.first_action).all()
    for rank in range(2):
        first, m = shard_range(n, 2, rank)
        shard = VecNovelGridworld(spec=spec, num_envs=m, seed=v.seed, autoreset=True, horizon=6, env_index_base=first)
        shard.reset()
        shard.set_state(0, **{k: getattr(o.st, k)[first:first + m] for k in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count')})
        got = shard.playouts(P, steps, SEED)
        for k in PO.REPORTS:
            assert (got[k] == both[k][first:first + m]).all(), (rank, k)
        shard.close()
    assert v.error_flags() == 0
    v.close()


def test_adapter_wrappers_and_limit_actions_agree_with_the_batched_call():
    """The single-env adapter under a novelty wrapper: [P] fields, the oracle's for its state.  LimitActions on top: ids in its own space,
    the oracle's for the limited action list."""
    env = T.make_adapter_env('axe10')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    P, steps = 66, 5
    vec = env.unwrapped._backend()
    rows = vec.get_state()
    play = env.playouts(P, steps, SEED)
    _, rep, _, _ = PO.oracle_playout(vec.spec, rows, np.zeros(P, np.int64), steps, SEED)
    assert play.ret.shape == (P,) and play.actions is None
    for k in PO.REPORTS:
        assert (play[k] == rep[k]).all(), k
    lim = LimitActions(env, set(NO_TURN))
    got = lim.playouts(P, steps, SEED)
    limited_spec = lim.__dict__['_playout_env'][2].spec
    assert list(limited_spec.actions_id) == sorted(NO_TURN)
    _, rep, _, _ = PO.oracle_playout(limited_spec, rows, np.zeros(P, np.int64), steps, SEED)
    for k in PO.REPORTS:
        assert (got[k] == rep[k]).all(), k
    assert set(got.first_action.tolist()) <= {0, 1}
    lim.close()


def test_cabi_errors_and_the_map_size_limit():
    import torch
    L = _cabi.lib()
    spec = T.build_spec('pogo10')
    n = 70
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    w = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset(); w.reset()
    s, foreign = v.snapshot(8), w.snapshot(8)
    out = torch.zeros(2 * 128, dtype=torch.int32, device='cuda')
    idx = torch.zeros(128, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    r, i, E, X, err = C.c_void_p(out.data_ptr()), C.c_void_p(idx.data_ptr()), _cabi.E_INVALID_ARG, L.ngw_snapshot_playout, _cabi.last_error
    N = None
    assert X(N, N, N, 1, 1, 1, 0, N, N, r, N, N, N, N, N, 0) == E and 'NULL' in err()
    assert X(v._h, N, N, 1, 0, 1, 0, N, N, r, N, N, N, N, N, 0) == E and '0 steps' in err()
    assert X(v._h, N, N, -1, 1, 1, 0, N, N, r, N, N, N, N, N, 0) == E
    assert X(v._h, N, N, 8, 2, 1, 0, N, N, N, N, N, N, N, r, 7) == E and 'action stride of 7' in err()
    assert X(v._h, N, N, 8, 1, 1, 0, N, i, r, N, N, N, N, N, 0) == E and 'without a destination snapshot' in err()
    assert X(v._h, N, N, 8, 1, 1, 0, foreign._s, N, r, N, N, N, N, N, 0) == E and 'not an open snapshot' in err()
    assert X(v._h, foreign._s, N, 8, 1, 1, 0, N, N, r, N, N, N, N, N, 0) == E and 'not an open snapshot' in err()
    assert X(v._h, N, N, 9, 1, 1, 0, s._s, N, N, N, N, N, N, N, 0) == E and '8 slots' in err()
    assert X(v._h, N, N, 71, 1, 1, 0, N, N, r, N, N, N, N, N, 0) == E and '70 envs' in err()
    assert X(v._h, N, N, 0, 1, 1, 0, N, N, N, N, N, N, N, N, 0) == 0                                # count == 0: a no-op
    assert X(v._h, N, N, 8, 2, 1, 0, N, N, N, N, N, N, N, N, 0) == 0                                # every output may be NULL
    assert X(v._h, N, i, 128, 2, 1, 0, N, N, N, N, N, N, N, r, 128) == 0                            # a list: count above n_envs, only the actions
    v.sync()
    assert (out[:256].cpu().numpy() >= 0).all() and v.error_flags() == 0
    v.close(); w.close()
    big = VecNovelGridworld(spec=make_spec(T.POGO, 48), num_envs=n, seed=4)
    big.reset()
    bs = big.snapshot(n)
    with pytest.raises(ValueError, match='64 maps in LDS') as ex:
        bs.rollout(None, np.zeros((n, 3), np.int64), from_envs=True)
    with pytest.raises(ValueError, match='64 maps in LDS') as ex2:
        bs.playout(np.arange(n), 3, SEED, from_envs=True)
    assert str(ex2.value).replace('ngw_snapshot_playout', 'ngw_snapshot_rollout') == str(ex.value) and 'map_size 48' in str(ex2.value)
    with pytest.raises(ValueError, match='64 maps in LDS'):
        big.playouts(2, 3, SEED)
    big.close()
